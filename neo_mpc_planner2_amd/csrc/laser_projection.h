// laser_projection.h -- K11: the LaserScan ranges of every scanner of every robot projected into global-frame hit points and
// sensor origins, the input of K10's rays (the contract: include/neo_mpc.h, neo_mpc_laser_batch).  Part of libneo_mpc.so's
// device code (included by neo_mpc_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "neo_mpc_device.h"

namespace neo_mpc {
namespace {

constexpr int kLaserThreads = 256;

// Steps 6 and 7 of the contract: a base-frame point into the global frame of a robot at (x, y) with (S, C) = sincos(yaw)
__device__ __forceinline__ double2 laser_to_global(double x, double y, double S, double C, double bx, double by) {
#pragma clang fp contract(off)
  return make_double2((x + bx * C) - by * S, (y + bx * S) + by * C);
}

// K11: grid (robot, source), a workgroup loops over the beams of one scan, a beam per lane and trip.  The robot's one sincos
// is paid once per thread, not once per beam; a beam's cos and sin come from the host's table, which the whole fleet shares
// and which stays in L2 (16 bytes a beam and source).  Per beam: 4 bytes of ranges read as coalesced float32, 16 bytes of
// table read and 16 bytes of point written per lane, 1 KiB per wave and instruction (points_out is 16-byte aligned: checked
// by the host).  What bounds it: the 16 bytes written and 4 read per beam against HBM -- a dozen float64 operations per 20
// bytes is far below the machine's balance -- and, for small fleets, the launch.  Plain vector stores, no atomics, no LDS;
// a workgroup writes the points and the origin of its own (robot, source) and nobody reads them in this launch.
__global__ __launch_bounds__(kLaserThreads) void k_laser_project(const LaserArgs a) {
#pragma clang fp contract(off)
  const uint32_t k = blockIdx.x, s = blockIdx.y;   // k < count, s < sources: the grid
  const LaserSource& src = a.source[s];
  const double x = a.poses[3 * (size_t)k], y = a.poses[3 * (size_t)k + 1];
  double S, C;
  sincos(a.poses[3 * (size_t)k + 2], &S, &C);
  const size_t scan = (size_t)k * a.sources + s;
  if (threadIdx.x == 0) {
    const double2 o = laser_to_global(x, y, S, C, src.mount_x, src.mount_y);
    a.origins[2 * scan] = o.x; a.origins[2 * scan + 1] = o.y;
  }
  const float* ranges = a.ranges + scan * a.beams;
  const double2* table = reinterpret_cast<const double2*>(a.table) + (size_t)s * a.beams;
  double2* points = reinterpret_cast<double2*>(a.points) + scan * a.beams;
  for (uint32_t i = threadIdx.x; i < a.beams; i += kLaserThreads) {   // i < beams: inside this scan's ranges, table and points
    double r = (double)ranges[i];
    if (r == (double)INFINITY && src.inf_is_valid) r = src.inf_range;
    double2 g = make_double2((double)NAN, (double)NAN);
    if (r >= src.range_min && r < src.range_max) {
      const double2 cs = table[i];
      g = laser_to_global(x, y, S, C, src.mount_x + r * cs.x, src.mount_y + r * cs.y);
    }
    points[i] = g;
  }
}

}  // namespace
}  // namespace neo_mpc
