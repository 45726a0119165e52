// plan_check.h -- K15: which of a fleet's global plans the live world map blocks (the contract: include/neo_mpc.h,
// neo_mpc_plan_check_batch), and the closest-pose stream it shares with K4 (k_carrot)
// Part of libneo_mpc.so's device code (included by neo_mpc_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "costmap.h"
#include "footprint_gate.h"

namespace neo_mpc {
namespace {

// The plan's closest pose to (rx, ry), first minimum (min_by, cpp:83-88), for a wave that holds one plan of np >= 1 poses:
// lanes stride over the poses (24 B each, consecutive lanes read consecutive poses: one contiguous 1.5 KB segment per wave
// load), four independent pose loads in flight per lane.  K4 and K15 start from the same pose because they both call this.
__device__ __forceinline__ uint32_t closest_pose(const double* poses, uint32_t np, double rx, double ry, int lane) {
  const double fx = poses[0] - rx, fy = poses[1] - ry;   // (the first pose: loaded ahead of the stream, looked at behind it)
  double best = INFINITY;
  uint32_t besti = 0xffffffffu;
  uint32_t k = lane;
  for (; k + 3 * kLanes < np; k += 4 * kLanes) {  // four independent pose loads in flight per lane
#define NT(p) __builtin_nontemporal_load(p)
    const double x0 = NT(poses + 3 * k), y0 = NT(poses + 3 * k + 1);
    const double x1 = NT(poses + 3 * (k + kLanes)), y1 = NT(poses + 3 * (k + kLanes) + 1);
    const double x2 = NT(poses + 3 * (k + 2 * kLanes)), y2 = NT(poses + 3 * (k + 2 * kLanes) + 1);
    const double x3 = NT(poses + 3 * (k + 3 * kLanes)), y3 = NT(poses + 3 * (k + 3 * kLanes) + 1);
#undef NT
    const double d0 = hypot(x0 - rx, y0 - ry), d1 = hypot(x1 - rx, y1 - ry);
    const double d2 = hypot(x2 - rx, y2 - ry), d3 = hypot(x3 - rx, y3 - ry);
    if (d0 < best) { best = d0; besti = k; }
    if (d1 < best) { best = d1; besti = k + kLanes; }
    if (d2 < best) { best = d2; besti = k + 2 * kLanes; }
    if (d3 < best) { best = d3; besti = k + 3 * kLanes; }
  }
  for (; k < np; k += kLanes) {
    const double d = hypot(poses[3 * k] - rx, poses[3 * k + 1] - ry);
    if (d < best) { best = d; besti = k; }
  }
  const double gmin = wave_min(best);
  uint32_t begin = (uint32_t)wave_min((best == gmin) ? (double)besti : 4.0e9);
  // min_by starts at the first pose and moves on a strict `<` alone: nothing is below a first distance of NaN, and where no
  // distance is below infinity no lane holds an index
  // (a NaN component alone does not make the first distance NaN: hypot(NaN, inf) is inf, and the search moves on from it;
  // the component test only keeps hypot off the common path)
  if (!(gmin < INFINITY) || ((fx != fx || fy != fy) && isnan(hypot(fx, fy)))) begin = 0;
  return begin;
}

// One raw cell of the world map (row-major, wsx bytes a row).  The bounds test keeps a wrong index from ever becoming a read
// outside the map: such a cell reads as lethal.
__device__ __forceinline__ int world_raw(const PlanCheckArgs& a, int cx, int cy) {
  const bool inside = (unsigned)cx < (unsigned)a.wsx && (unsigned)cy < (unsigned)a.wsy;
  return inside ? a.world[(long)cy * a.wsx + cx] : 254;
}

// lineCost on the world map: 254 as soon as a cell of the edge holds it, else the largest raw value among its cells (which may
// be 255).  At most 2^20 cells: both end points are cells of the map.
__device__ __forceinline__ int world_edge_cost(const PlanCheckArgs& a, int x0, int y0, int x1, int y1) {
  const int dx = x1 >= x0 ? x1 - x0 : x0 - x1, dy = y1 >= y0 ? y1 - y0 : y0 - y1;
  const int cells = (dx >= dy ? dx : dy) + 1;
  int cost = 0;
  for (int k = 0; k < cells; ++k) {
    int cx, cy;
    line_cell(x0, y0, x1, y1, k, cx, cy);
    const int raw = world_raw(a, cx, cy);
    if (raw == 254) return 254;
    cost = raw > cost ? raw : cost;
  }
  return cost;
}

// neo_mpc_footprint_batch's outline cost at (x, y, yaw) on the world map, one lane on its own: nav2's fold statement by
// statement -- K6 reduces the same fold over a wave, this walks it -- with the first and the previous vertex's cell kept and
// the base-frame vertices re-read from the one shared polygon (the same address in every lane).
__device__ __forceinline__ int world_outline_cost(const PlanCheckArgs& a, double x, double y, double th) {
  const int n = (int)a.footprint_points;   // 3 .. 16 (neo_mpc_capi.cpp refuses anything else)
  double sn, cs;
  sincos(th, &sn, &cs);
  double X, Y;
  int fx, fy;
  orient_vertex(x, y, sn, cs, a.footprint[0], a.footprint[1], X, Y);
  if (off_map_cell(X, Y, a.wox, a.woy, a.wres, a.winv, a.wsx, a.wsy, fx, fy)) return 254;
  int cost = 0, px = fx, py = fy;
  for (int j = 1; j < n; ++j) {
    int mx, my;
    orient_vertex(x, y, sn, cs, a.footprint[2 * j], a.footprint[2 * j + 1], X, Y);
    if (off_map_cell(X, Y, a.wox, a.woy, a.wres, a.winv, a.wsx, a.wsy, mx, my)) return 254;
    const int edge = world_edge_cost(a, px, py, mx, my);
    cost = edge > cost ? edge : cost;
    px = mx; py = my;
    if (cost == 254) return 254;
  }
  const int edge = world_edge_cost(a, px, py, fx, fy);   // the closing edge
  return edge > cost ? edge : cost;
}

// K15, one wavefront per plan.  The start pose comes from K4's stream (or is pose 0); then lanes stride [begin, end), 64 poses
// a round: point mode is one byte gather from the map per round, footprint mode one outline per lane.  A ballot of "blocks"
// ends the scan at the first round that has one -- its lowest set bit is the first blocked pose, every earlier round held
// none --, and where no round has one the running maximum of the values below 255 is reduced over the wave.  Rounds:
// (end - begin + 63) / 64; no loop waits on a value another wave writes.
template <bool kFootprint>
__global__ __launch_bounds__(kLanes) void k_plan_check(const PlanCheckArgs a) {
  const int lane = threadIdx.x;
  const size_t b = blockIdx.x;
  if (b >= a.count) return;
  const uint32_t o0 = a.plan_offsets[b], np = a.plan_offsets[b + 1] - o0;
  const double* poses = a.plan_poses + 3 * (size_t)o0;
  neo_mpc_plan_check out;
  out.begin = 0; out.end = 0; out.first_blocked = 0; out.status = 0; out.value = 0; out.reserved = 0;
  if (np == 0) {   // nav2 calls an empty path invalid
    out.status = 2;
    if (lane == 0) a.results[b] = out;
    return;
  }
  uint32_t begin = 0;
  if (a.robot_poses) begin = closest_pose(poses, np, a.robot_poses[3 * b], a.robot_poses[3 * b + 1], lane);
  const uint32_t end = (a.max_poses != 0 && a.max_poses < np - begin) ? begin + a.max_poses : np;
  int widest = 0;   // largest value below 255 this lane has met
  uint32_t first = end;
  for (uint64_t base = begin; base < end; base += kLanes) {   // (64 bits: the last round of a plan that ends near 2^32 poses)
    const uint64_t k = base + lane;
    int v = 0;
    bool blocks = false;
    if (k < end) {
      const double x = __builtin_nontemporal_load(poses + 3 * k), y = __builtin_nontemporal_load(poses + 3 * k + 1);
      if (kFootprint) {
        v = world_outline_cost(a, x, y, __builtin_nontemporal_load(poses + 3 * k + 2));
      } else {
        int mx, my;
        const bool off = off_map_cell(x, y, a.wox, a.woy, a.wres, a.winv, a.wsx, a.wsy, mx, my);
        v = off ? (int)a.outside : world_raw(a, mx, my);
      }
      blocks = v == 255 ? a.unknown_blocks != 0 : v >= (int)a.max_cost;
      if (v < 255 && v > widest) widest = v;
    }
    const unsigned long long hit = __ballot(blocks);
    if (hit) {
      const int at = (int)__ffsll((long long)hit) - 1;
      first = (uint32_t)base + (uint32_t)at;
      out.status = 1;
      out.value = (uint32_t)__shfl(v, at);
      break;
    }
  }
  if (out.status == 0) out.value = (uint32_t)wave_max_f((float)widest);   // (0 .. 254: exact in float32)
  out.begin = begin; out.end = end; out.first_blocked = first;
  if (lane == 0) a.results[b] = out;
}

}  // namespace
}  // namespace neo_mpc
