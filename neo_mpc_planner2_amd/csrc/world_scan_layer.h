// world_scan_layer.h -- K12: one obstacle layer for the whole fleet on the world map's lattice -- cleared along every robot's
// rays, marked at their end points, freed under the robots' own outlines, merged into a copy of the world map and inflated
// there, so that the roll cuts every window from what the whole fleet saw (the contract: include/neo_mpc.h,
// neo_mpc_fleet_clear and neo_mpc_update_world_scan_layer).  Part of libneo_mpc.so's device code (included by
// neo_mpc_kernels.hip).
//
// Three buffers of one role each, all WSX bytes a row like the world map: `layer` persists between updates and is written in
// place by the rays and the footprints; `world` is the static map, read only; `live` is rewritten whole by every update and is
// what the roll reads.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "footprint_gate.h"
#include "inflation.h"
#include "neo_mpc_device.h"
#include "scan_layer.h"
#include "wave_ops.h"

namespace neo_mpc {
namespace {

// K12a, steps 1 and 2 of the contract: K10b's ray (scan_ray) on the world's geometry, grid (point chunks, robot).  K10b's
// argument carries over to rays of different robots: within a launch every writer of a byte writes the same value.
template <bool kMark>
__global__ __launch_bounds__(kScanRayThreads) void k_world_scan_rays(const WorldScanArgs a) {
  scan_ray<kMark>(a.s, blockIdx.y, blockIdx.x * kScanRayThreads + threadIdx.x, a.wox, a.woy, a.wres, a.wsx, a.wsy, a.wsx, a.layer);
}

// robot j's vertex v in the global frame: taken as given, or the base-frame footprint placed by K6's own routine (compiled
// as K6 and K8a compile it, so that the gate's footprints_out is bit for bit what is cleared)
__device__ __forceinline__ void world_clear_vertex(const WorldScanArgs& a, size_t j, int v, double& X, double& Y) {
  const size_t n = a.points;
  if (a.polygons) { X = a.polygons[(j * n + v) * 2]; Y = a.polygons[(j * n + v) * 2 + 1]; return; }
  double x, y, th, sn, cs;
  footprint_pose(a.poses, a.problems, j, x, y, th);
  sincos(th, &sn, &cs);
  const double* src = a.footprint + (a.per_robot ? j * 2 * n : 0) + 2 * v;
  orient_vertex(x, y, sn, cs, src[0], src[1], X, Y);
}

// K12b, step 3 of the contract: one wave per robot.  Lane e holds edge e: its start, its direction and padding * L_e go to
// LDS.  The cells the rule can clear lie within D = padding / sin(theta / 2) of the polygon's bounding box, theta its sharpest
// interior angle (either arm of the rule is an intersection of half planes whose unit normals are those of the edges: from a
// point of the polygon it reaches no further than padding / max_e (n_e . u) along u, and the minimum of that maximum over u
// is sin(theta / 2)); the wave walks that box with a little slack, clamped to the world in float64, a cell per lane, and
// evaluates the rule unfused.  A corner too sharp for the bound to be computed safely makes the box the world.  Every writer
// writes 0: robots whose boxes overlap need no order.  No atomics, one unconditional barrier.
__global__ __launch_bounds__(kLanes) void k_world_scan_footprints(const WorldScanArgs a) {
#pragma clang fp contract(off)
  __shared__ double edge[5 * NEO_MPC_MAX_FOOTPRINT_POINTS];   // a.x, a.y, ex, ey, padding * L_e
  const int lane = threadIdx.x, n = (int)a.points;
  const size_t j = blockIdx.x;
  const bool has = lane < n;
  double X = 0.0, Y = 0.0, X1 = 0.0, Y1 = 0.0, X0 = 0.0, Y0 = 0.0;
  if (has) {
    world_clear_vertex(a, j, lane, X, Y);
    world_clear_vertex(a, j, lane + 1 < n ? lane + 1 : 0, X1, Y1);
    world_clear_vertex(a, j, lane > 0 ? lane - 1 : n - 1, X0, Y0);
  }
  const double ex = X1 - X, ey = Y1 - Y, len = sqrt(ex * ex + ey * ey);
  if (has) {
    double* e = edge + 5 * lane;
    e[0] = X; e[1] = Y; e[2] = ex; e[3] = ey; e[4] = a.padding * len;
  }
  // the sharpest corner: at this lane's vertex the boundary turns by phi, and sin(theta / 2) = cos(phi / 2)
  const double px = X - X0, py = Y - Y0, plen = sqrt(px * px + py * py);
  double half = sqrt(fmax(0.0, 0.5 * (1.0 + (px * ex + py * ey) / (plen * len))));
  if (!(half == half)) half = 0.0;                      // (an edge without length: no bound, the box is the world)
  const bool finite = __ballot(has && !(isfinite(X) && isfinite(Y))) == 0ull;
  const double sharpest = wave_min(has ? half : 1.0);
  const double bx0 = wave_min(has ? X : INFINITY), bx1 = wave_max(has ? X : -INFINITY);
  const double by0 = wave_min(has ? Y : INFINITY), by1 = wave_max(has ? Y : -INFINITY);
  __syncthreads();
  if (!finite) return;                                  // a vertex that is not finite: nothing is cleared
  const int sx = a.wsx, sy = a.wsy;
  const double res = a.wres, ox = a.wox, oy = a.woy;
  double lox = 0.0, loy = 0.0, hix = (double)(sx - 1), hiy = (double)(sy - 1);
  if (a.padding == 0.0 || sharpest >= 1e-3) {
    // a centre ox + (i + 0.5) res inside [x0, x1] has floor((x0 - ox) / res) - 1 <= i <= floor((x1 - ox) / res) + 1
    const double reach = a.padding == 0.0 ? 0.0 : a.padding / sharpest * 1.001 + res;
    lox = fmax(floor((bx0 - reach - ox) / res) - 1.0, lox); hix = fmin(floor((bx1 + reach - ox) / res) + 1.0, hix);
    loy = fmax(floor((by0 - reach - oy) / res) - 1.0, loy); hiy = fmin(floor((by1 + reach - oy) / res) + 1.0, hiy);
  }
  if (!(lox <= hix && loy <= hiy)) return;              // (clamped in float64: the conversions below cannot overflow)
  const int i_lo = (int)lox, l_lo = (int)loy;
  const int64_t w = (int64_t)((int)hix - i_lo + 1), total = w * (int64_t)((int)hiy - l_lo + 1);
  for (int64_t idx = lane; idx < total; idx += kLanes) {
    const int dl = (int)(idx / w), l = l_lo + dl, i = i_lo + (int)(idx - (int64_t)dl * w);
    const double cx = ox + ((double)i + 0.5) * res, cy = oy + ((double)l + 0.5) * res;
    bool pos = true, neg = true;
    for (int e = 0; e < n; ++e) {
      const double* g = edge + 5 * e;
      const double ce = g[2] * (cy - g[1]) - g[3] * (cx - g[0]);
      pos = pos && ce >= -g[4];
      neg = neg && ce <= g[4];
    }
    // 0 <= i < wsx, 0 <= l < wsy: inside the layer
    if (pos || neg) a.layer[(int64_t)l * sx + i] = 0;
  }
}

// K12c, step 4 of the contract, K9's and K10c's tile scheme on the world: grid (tile column, tile row), one workgroup of four
// waves per tile of 64 x 64 cells.
//   1  The tile's halo of `layer` becomes a bitmask of seeds in LDS (inflation_tile_seeds).
//   2  Every cell of the tile: the world's value, the layer's put over it by updateWithMax, goes to `live`.
//   3  A tile with a seed in its halo has T in LDS and every cell takes T[N] by nav2's rule (inflation_tile_distance,
//      inflation_combine); a tile without one never loads T.
// `layer` and `world` are read and not written; a byte of `live` is written, and in step 3 read back, by the one lane that owns
// its cell, step 2 before step 3 in program order.  Rows are WSX bytes apart, whatever WSX is: every access is a byte.  No atomics.
__global__ __launch_bounds__(kLanes * kInflateWaves) void k_world_scan_compose(const WorldScanArgs a) {
  __shared__ uint64_t masks[kInflateRows * 3];
  __shared__ uint8_t table[kInflationTableBytes];
  __shared__ int seen[kInflateWaves];
  const int lane = threadIdx.x & (kLanes - 1), wave = uniform_int((int)(threadIdx.x >> 6));
  const int R = a.s.reach, sx = a.wsx, sy = a.wsy;
  const int tx = (int)blockIdx.x * kInflateTile, ty = (int)blockIdx.y * kInflateTile;
  const bool some = inflation_tile_seeds(masks, table, seen, a.layer, sx, sx, sy, tx, ty, R, a.s.table, lane, wave);
  const int i = tx + lane;
  for (int j = wave; j < kInflateTile && ty + j < sy; j += kInflateWaves) {
    const int l = ty + j, r0 = j + R;
    if (i >= sx) continue;                             // (nothing below is a wave operation)
    // 0 <= i < wsx, 0 <= l < wsy: this tile's own cell, in the layer, the world map and `live`
    const int64_t at = (int64_t)l * sx + i;
    const int v = a.layer[at], old = a.world[at];
    uint8_t* p = a.live + at;
    *p = (uint8_t)((v != 255 && (old == 255 || old < v)) ? v : old);
    if (!some) continue;
    const int best = inflation_tile_distance(masks, R, r0, lane);
    if (best <= R * R) inflation_combine(p, table, best);
  }
}

}  // namespace
}  // namespace neo_mpc
