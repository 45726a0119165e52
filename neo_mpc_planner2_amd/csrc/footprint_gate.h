// footprint_gate.h -- K6: footprintCostAtPose for a fleet (src/NeoMpcPlanner.cpp:218-219) on the device map(s)
// Part of libneo_mpc.so's device code (included by neo_mpc_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "costmap.h"

namespace neo_mpc {
namespace {

constexpr int kGateWaves = 4;   // robots per workgroup: one wave each, no LDS and no barrier between them

// inclusive prefix sum over the 16 lanes of each DPP row (the polygon's vertices sit in lanes 0-15)
__device__ __forceinline__ int row_scan_i(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true);  // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, true);  // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, true);  // row_shr:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, true);  // row_shr:8
  return v;
}
// bitwise OR over the 64 lanes, every lane returns it (the ladder of wave_max)
__device__ __forceinline__ int wave_or(int v) {
  v |= __builtin_amdgcn_update_dpp(v, v, 0x111, 0xf, 0xf, false);
  v |= __builtin_amdgcn_update_dpp(v, v, 0x112, 0xf, 0xf, false);
  v |= __builtin_amdgcn_update_dpp(v, v, 0x114, 0xf, 0xf, false);
  v |= __builtin_amdgcn_update_dpp(v, v, 0x118, 0xf, 0xf, false);
  v |= __builtin_amdgcn_update_dpp(v, v, 0x142, 0xa, 0xf, false);
  v |= __builtin_amdgcn_update_dpp(v, v, 0x143, 0xc, 0xf, false);
  return __builtin_amdgcn_readlane(v, 63);
}

// Where robot `b` stands -- its row of `poses`, else cur_xy and the yaw of cur_q of its request -- and one base-frame vertex
// placed there.  K6 and K8 (fleet_stamp.h) both go through these two, so the polygons K6 writes as footprints_out are bit
// for bit the ones K8 stamps for the same inputs.
__device__ __forceinline__ void footprint_pose(const double* poses, const neo_mpc_problem* problems, size_t b, double& x,
                                               double& y, double& th) {
  if (poses) {
    x = poses[3 * b]; y = poses[3 * b + 1]; th = poses[3 * b + 2];
  } else {
    const double* P = reinterpret_cast<const double*>(problems + b);
    x = P[P_CUR_X]; y = P[P_CUR_Y]; th = yaw_of(P + P_CUR_Q);
  }
}
__device__ __forceinline__ void orient_vertex(double x, double y, double sn, double cs, double px, double py, double& X,
                                              double& Y) {
  const double ox = x + px * cs - py * sn, oy = y + px * sn + py * cs;
  X = ox; Y = oy;
}

// Costmap2D::worldToMap's rule for a point (X, Y) against a map of sx x sy cells (its TRUE size) -> whether the point is off the
// map, and its cell.  cell_of equals the exact division wherever the result is >= 0; NaN fails both >= tests, +inf saturates
// beyond every size.  K6's vertices and K15's vertices and plan poses (plan_check.h) all go through it.
__device__ __forceinline__ bool off_map_cell(double X, double Y, double ox, double oy, double res, double inv, int sx, int sy,
                                             int& mx, int& my) {
  mx = cell_of(X, ox, res, inv);
  my = cell_of(Y, oy, res, inv);
  return !(X >= ox) || !(Y >= oy) || mx >= sx || my >= sy;
}

// nav2_util::LineIterator's walk from cell (x0, y0) to (x1, y1) in closed form: cell k of the edge, k = 0 .. max(dx, dy), as a
// function of k alone (K6 deals the cells of a whole outline over the lanes, K15 walks one outline per lane).
__device__ __forceinline__ void line_cell(int x0, int y0, int x1, int y1, int k, int& cx, int& cy) {
  const int dx = x1 >= x0 ? x1 - x0 : x0 - x1, dy = y1 >= y0 ? y1 - y0 : y0 - y1;
  const int sx = x1 >= x0 ? 1 : -1, sy = y1 >= y0 ? 1 : -1;
  const int major = dx >= dy ? dx : dy, minor = dx >= dy ? dy : dx;
  // (major / 2 + k * minor) / major in integers: the numerator stays below 2^41 for maps of up to 2^20 cells a side
  // and the quotient below 2^21, so the float64 division, truncated, is the integer division (a quotient that is not
  // whole is 1 / major >= 2^-20 from the next integer, the division's rounding error below 2^-31)
  const int q = major ? (int)((double)((long)(major >> 1) + (long)k * minor) / (double)major) : 0;
  cx = dx >= dy ? x0 + sx * k : x0 + sx * q;
  cy = dx >= dy ? y0 + sy * q : y0 + sy * k;
}

// K6: nav2's FootprintCollisionChecker::footprintCostAtPose on raw cell values (the contract: include/neo_mpc.h,
// neo_mpc_footprint_batch), one wavefront per robot.  Vertices go one per lane (<= 16: one DPP row): oriented in float64,
// turned into cells by worldToMap's rule against the map's TRUE size.  LineIterator's walk has a closed form -- cell k of an
// edge is a function of k alone -- so the cells of the WHOLE outline are dealt over the lanes (a prefix sum of the edges'
// lengths says which edge a lane's cell belongs to) and read in one byte gather per 64 cells: a 0.7 m x 0.5 m outline at
// 5 cm is 52 cells, one round.  nav2's fold over the edges is order-dependent, but only through three facts per edge --
// it holds a 254, it holds a 255, its largest other value -- and any vertex off the map ends every path through the fold
// at 254: two 16-bit edge masks and one maximum, reduced over the wave, give the fold's answer exactly.
__global__ __launch_bounds__(kLanes * kGateWaves) void k_footprint_gate(const FootprintGateArgs a) {
  const int lane = threadIdx.x & (kLanes - 1);
  const size_t b = (size_t)blockIdx.x * kGateWaves + (size_t)uniform_int((int)(threadIdx.x >> 6));
  if (b >= a.count) return;
  const int n = (int)a.footprint_points;   // 3 .. 16 (neo_mpc_capi.cpp refuses anything else)
  double x, y, th;
  footprint_pose(a.poses, a.problems, b, x, y, th);
  DevMap m = a.map;
  if (m.pool_count > 0) {   // (select_map's rule: an index outside the pool is clamped into it)
    int idx = a.map_indices ? a.map_indices[b] : a.problems ? a.problems[b].map_index : 0;
    idx = uniform_int(idx < 0 ? 0 : (idx >= m.pool_count ? m.pool_count - 1 : idx));
    m.cells += (long)idx * m.pool_stride;
    m.origin_x = m.pool_origins[2 * idx];
    m.origin_y = m.pool_origins[2 * idx + 1];
  }
  // vertex `lane` (lanes beyond the polygon carry vertex 0 and take no part)
  const bool has = lane < n;
  const double* poly = a.footprint + (a.per_robot ? b * 2 * (size_t)n : 0) + 2 * (has ? lane : 0);
  const double px = poly[0], py = poly[1];
  double sn, cs;
  sincos(th, &sn, &cs);
  double X, Y;
  orient_vertex(x, y, sn, cs, px, py, X, Y);
  if (a.footprints_out && has) {
    double* out = a.footprints_out + (b * (size_t)n + lane) * 2;
    out[0] = X; out[1] = Y;
  }
  int mx, my;
  const bool off = off_map_cell(X, Y, m.origin_x, m.origin_y, m.resolution, m.inv_resolution, m.size_x, m.size_y, mx, my);
  int cost = 254;   // a vertex off the map: nav2's fold returns LETHAL_OBSTACLE at that vertex, or did so before it
  if (__ballot(has && off) == 0ull) {
    // edge `lane` runs from vertex `lane` to the next one (the last edge closes the polygon); every vertex is on the map,
    // so every cell of every edge is: a line between two cells stays inside their bounding box
    const int next = lane + 1 < n ? lane + 1 : 0;
    const int nx = __shfl(mx, next), ny = __shfl(my, next);
    const int ex = nx >= mx ? nx - mx : mx - nx, ey = ny >= my ? ny - my : my - ny;
    const int len = has ? (ex > ey ? ex : ey) + 1 : 0;   // cells of this edge, end points included
    const int incl = row_scan_i(len);                    // lanes 0-15: cells of edges 0 .. lane
    const int total = __builtin_amdgcn_readlane(incl, 15);
    int bits = 0, worst = 0;   // bit e: edge e holds a 254; bit 16 + e: it holds a 255; worst: largest value below 254
    for (int t0 = 0; t0 < total; t0 += kLanes) {
      const int t = t0 + lane;   // this lane's cell of the outline
      int e = 0;                 // ... belongs to the first edge whose cells end beyond t
      for (int j = 0; j < n - 1; ++j) e += t >= __builtin_amdgcn_readlane(incl, j) ? 1 : 0;
      const int x0 = __shfl(mx, e), y0 = __shfl(my, e), x1 = __shfl(nx, e), y1 = __shfl(ny, e);
      const int k = t - __shfl(incl - len, e);
      int cx, cy;
      line_cell(x0, y0, x1, y1, k, cx, cy);
      if (t < total) {
        // (the bounds test cannot fail -- see above; it keeps a wrong index from ever becoming a read outside the map)
        const bool inside = (unsigned)cx < (unsigned)m.size_x && (unsigned)cy < (unsigned)m.size_y;
        const int raw = inside ? m.cells[(long)cy * m.pitch + cx] : 254;
        if (raw == 254) bits |= 1 << e;
        else if (raw == 255) bits |= 0x10000 << e;
        else worst = raw > worst ? raw : worst;
      }
    }
    bits = wave_or(bits);
    worst = (int)wave_max_f((float)worst);
    // nav2's fold: edges 0 .. n-2 in order with a running maximum that returns the moment it EQUALS 254 -- which it does
    // at the first edge costing 254 unless an edge costing 255 came before it; then the maximum with the closing edge
    const int lethal = bits & 0xffff, unknown = (bits >> 16) & ~lethal;   // an edge holding both costs 254
    const int head = (1 << (n - 1)) - 1;
    const int first_lethal = __ffs(lethal & head), first_unknown = __ffs(unknown & head);   // 1-based, 0: none
    if (first_lethal && (!first_unknown || first_lethal < first_unknown)) cost = 254;
    else cost = unknown ? 255 : lethal ? 254 : worst;
  }
  if (lane == 0) {
    a.footprint_costs[b] = (double)cost;
    if (a.problems) a.problems[b].footprint_cost = cost >= 254 ? 1.0 : 0.0;   // the normalised form
  }
}

}  // namespace
}  // namespace neo_mpc
