// scan_layer.h -- K10: a persistent obstacle layer per rolling window, fed from sensor points -- rolled with its window,
// cleared along this tick's rays, marked at their end points, combined into the window and inflated (the contract:
// include/neo_mpc.h, neo_mpc_scan_batch).  Part of libneo_mpc.so's device code (included by neo_mpc_kernels.hip).
//
// Two layer buffers of one role each, so that an update captured in a graph can be replayed: `layer` holds the layers
// between updates, `work` this update's.  k_scan_shift reads `layer` at the roll's offset and writes `work`; k_scan_rays
// clears and marks in `work`; k_scan_apply reads `work`, rewrites the windows and hands `work` back to `layer`.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "inflation.h"
#include "neo_mpc_device.h"
#include "wave_ops.h"

namespace neo_mpc {
namespace {

constexpr int kScanShiftRows = 16;  // rows of one window a workgroup of k_scan_shift moves
constexpr int kScanRayThreads = 256;

// K10a, step 1 of the contract (and its reset): grid (row chunks, window), four cells per thread and store.  A workgroup
// reads `layer` and the two origins, which no launch of this update has written yet, and writes rows of `work` that are its
// own: nobody reads what another workgroup writes.  The columns from size_x up to the pitch are filled and never read.
__global__ __launch_bounds__(256) void k_scan_shift(const ScanArgs a) {
#pragma clang fp contract(off)
  const uint32_t k = blockIdx.y;
  const int sx = a.size_x, sy = a.size_y, lp = a.layer_pitch;
  bool wipe = a.reset != 0;
  int cx = 0, cy = 0;
  if (!wipe) {
    const double qx = (a.origins[2 * (size_t)k] - a.layer_origins[2 * (size_t)k]) / a.res;
    const double qy = (a.origins[2 * (size_t)k + 1] - a.layer_origins[2 * (size_t)k + 1]) / a.res;
    if (fabs(qx) < (double)sx && fabs(qy) < (double)sy) { cx = (int)rint(qx); cy = (int)rint(qy); }   // (nearest, ties to even)
    else wipe = true;                                                                                // (NaN and infinity too)
  }
  const uint8_t* src = a.layer + (int64_t)k * a.layer_stride;
  uint8_t* dst = a.work + (int64_t)k * a.layer_stride;
  const uint32_t unknown = a.unknown;
  const int groups = lp >> 2, r0 = (int)blockIdx.x * kScanShiftRows;
  for (int idx = threadIdx.x; idx < kScanShiftRows * groups; idx += 256) {
    const int dr = idx / groups, l = r0 + dr, i0 = (idx - dr * groups) << 2;
    if (l >= sy) break;
    const int sl = l + cy;
    uint32_t word = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int si = i0 + b + cx;
      uint32_t v = unknown;
      // 0 <= sl < size_y and 0 <= si < size_x: inside this window's layer
      if (!wipe && i0 + b < sx && (unsigned)sl < (unsigned)sy && (unsigned)si < (unsigned)sx) v = src[(int64_t)sl * lp + si];
      word |= v << (8 * b);
    }
    // l < size_y, i0 + 3 < pitch (a multiple of 4): inside this window's layer, 4-byte aligned
    *reinterpret_cast<uint32_t*>(dst + (int64_t)l * lp + i0) = word;
  }
}

// worldToMap of the contract on window geometry (ox, oy, res, sx, sy)
__device__ __forceinline__ bool scan_world_to_map(double wx, double wy, double ox, double oy, double res, int sx, int sy,
                                                  int& mx, int& my) {
#pragma clang fp contract(off)
  if (!isfinite(wx) || !isfinite(wy) || wx < ox || wy < oy) return false;
  const double qx = trunc((wx - ox) / res), qy = trunc((wy - oy) / res);
  if (!(qx < (double)sx && qy < (double)sy)) return false;
  mx = (int)qx; my = (int)qy;
  return true;
}
// cellDistance of the contract
__device__ __forceinline__ uint32_t scan_cell_distance(double d, double res) {
#pragma clang fp contract(off)
  return (uint32_t)fmin(fmax(0.0, ceil(d / res)), 2147483647.0);
}

// One ray of steps 2 and 3 of the contract: point p of robot k of the batch `a`, on a grid of sx x sy cells of `res` at (ox, oy)
// whose cell (0, 0) is at `layer`, rows lp bytes apart (kMark false: the clearing walk; true: the mark).  The one copy of the
// clips, raytraceLine and the mark test: K10b runs it on a window's geometry and layer, K12a (world_scan_layer.h) on the world's.
// kStamp (K14c alone, world_scan_decay.h): the mark also writes `now` into `stamp`, a word per cell with rows lp words apart;
// without it the two arguments are dead and every kernel comes out as it did before they were there.
template <bool kMark, bool kStamp = false>
__device__ __forceinline__ void scan_ray(const ScanArgs& a, uint32_t k, uint32_t p, double ox, double oy, double res, int sx,
                                         int sy, int lp, uint8_t* layer, uint32_t* stamp = nullptr, uint32_t now = 0u) {
#pragma clang fp contract(off)
  uint32_t np = a.max_points;
  if (a.point_counts) { const uint32_t c = a.point_counts[k]; np = c < np ? c : np; }
  if (p >= np) return;
  const size_t src = (size_t)k * a.sources + p / a.points_per_source;   // (K10: sources 1, points_per_source max_points: k)
  const double sx0 = a.sensor_origins[2 * src], sy0 = a.sensor_origins[2 * src + 1];
  const double* pt = a.points + ((size_t)k * a.max_points + p) * 2;
  double wx = pt[0], wy = pt[1];
  if (!isfinite(wx) || !isfinite(wy)) return;
  if (kMark) {
    const double s = (wx - sx0) * (wx - sx0) + (wy - sy0) * (wy - sy0);
    if (s >= a.obstacle_max * a.obstacle_max || s < a.obstacle_min * a.obstacle_min) return;
    int mx, my;
    if (!scan_world_to_map(wx, wy, ox, oy, res, sx, sy, mx, my)) return;
    layer[(int64_t)my * lp + mx] = 254;   // 0 <= mx < sx, 0 <= my < sy by worldToMap
    if (kStamp) stamp[(int64_t)my * lp + mx] = now;
    return;
  }
  int x0, y0, x1, y1;
  if (!scan_world_to_map(sx0, sy0, ox, oy, res, sx, sy, x0, y0)) return;
  const double ex = ox + (double)sx * res, ey = oy + (double)sy * res;
  const double da = wx - sx0, db = wy - sy0;
  if (wx < ox) { const double t = (ox - sx0) / da; wx = ox; wy = sy0 + db * t; }
  if (wy < oy) { const double t = (oy - sy0) / db; wx = sx0 + da * t; wy = oy; }
  if (wx > ex) { const double t = (ex - sx0) / da; wx = ex - 0.001; wy = sy0 + db * t; }
  if (wy > ey) { const double t = (ey - sy0) / db; wx = sx0 + da * t; wy = ey - 0.001; }
  if (!scan_world_to_map(wx, wy, ox, oy, res, sx, sy, x1, y1)) return;
  // raytraceLine: everything from here on is integers but the three float64 lines the contract names
  const uint32_t M = scan_cell_distance(a.raytrace_max, res), m = scan_cell_distance(a.raytrace_min, res);
  const int Dx = x1 - x0, Dy = y1 - y0;
  const double dist = sqrt((double)((int64_t)Dx * Dx + (int64_t)Dy * Dy));
  if (dist < (double)m) return;
  int u0 = x0, v0 = y0;
  if (dist > 0.0) {
    u0 = (int)(uint32_t)((double)x0 + (double)Dx / dist * (double)m);
    v0 = (int)(uint32_t)((double)y0 + (double)Dy / dist * (double)m);
  }
  const int dx = x1 - u0, dy = y1 - v0;
  const int step_x = dx > 0 ? 1 : -1, step_y = dy > 0 ? 1 : -1;
  const uint32_t adx = (uint32_t)(dx < 0 ? -dx : dx), ady = (uint32_t)(dy < 0 ? -dy : dy);
  const double scale = dist == 0.0 ? 1.0 : fmin(1.0, (double)M / dist);
  const bool x_major = adx >= ady;
  const uint32_t A = x_major ? adx : ady, B = x_major ? ady : adx;
  const uint32_t reach = (uint32_t)(scale * (double)A), n = M < reach ? M : reach;
  int x = u0, y = v0, e = (int)(A / 2);
  for (uint32_t t = 0; t < n; ++t) {
    // (the contract's walk stays inside the grid; the comparison keeps a store inside the layer whatever comes)
    if ((unsigned)x < (unsigned)sx && (unsigned)y < (unsigned)sy) layer[(int64_t)y * lp + x] = 0;
    if (x_major) x += step_x; else y += step_y;
    e += (int)B;
    if ((uint32_t)e >= A) {
      if (x_major) y += step_y; else x += step_x;
      e -= (int)A;
    }
  }
  if ((unsigned)x < (unsigned)sx && (unsigned)y < (unsigned)sy) layer[(int64_t)y * lp + x] = 0;
}

// K10b, steps 2 and 3 of the contract: one launch per phase (kMark false: clear, then true: mark -- the launch boundary is
// what puts every mark behind every clear), grid (point chunks, window), a lane per ray.  No atomics: within a launch every
// writer of a byte writes the same value -- 0 in the clearing launch, 254 in the marking one -- so whichever of two colliding
// byte stores lands last the byte is the same; byte stores merge into their line by byte mask and touch no neighbour.
// With several sources (K11) a window's points are those of all its sources, point p seen from source p / points_per_source,
// and the argument still holds: one clearing launch over all sources, then one marking launch over all sources, puts every
// mark of every source behind every clear of every source with no new synchronisation.
// Nothing is read back from the layer.  The trip counts of the walk diverge between lanes; nothing ballots inside it.
template <bool kMark>
__global__ __launch_bounds__(kScanRayThreads) void k_scan_rays(const ScanArgs a) {
  const uint32_t k = blockIdx.y;
  scan_ray<kMark>(a, k, blockIdx.x * kScanRayThreads + threadIdx.x, a.origins[2 * (size_t)k], a.origins[2 * (size_t)k + 1], a.res,
                  a.size_x, a.size_y, a.layer_pitch, a.work + (int64_t)k * a.layer_stride);
}

// K10c, steps 4 and 5 of the contract, K9's scheme per window: grid (tile column, tile row, window), one workgroup of four
// waves per tile of 64 x 64 cells.
//   1  The tile's halo of `work` becomes a bitmask of seeds in LDS (inflation_tile_seeds).
//   2  Every cell of the tile: the layer's value goes back to `layer`, and into the window by updateWithMax.
//   3  A tile with a seed in its halo has T in LDS and every cell takes T[N] by nav2's rule (inflation_tile_distance,
//      inflation_combine); a tile without one never loads T.
// Seeds are read from `work`, which this launch does not write, so the in-place hazard K9 argues away does not arise here.
// `layer` is written and not read.  A window byte is read and written by the one lane that owns its cell, step 2 before
// step 3 in program order.  The layer's new origin is the window's: written by the window's first tile, read by nobody in
// this launch.  No atomics.
__global__ __launch_bounds__(kLanes * kInflateWaves) void k_scan_apply(const ScanArgs a) {
  __shared__ uint64_t masks[kInflateRows * 3];
  __shared__ uint8_t table[kInflationTableBytes];
  __shared__ int seen[kInflateWaves];
  const int lane = threadIdx.x & (kLanes - 1), wave = uniform_int((int)(threadIdx.x >> 6));
  const uint32_t k = blockIdx.z;
  const int R = a.reach, sx = a.size_x, sy = a.size_y, lp = a.layer_pitch;
  const int tx = (int)blockIdx.x * kInflateTile, ty = (int)blockIdx.y * kInflateTile;
  const uint8_t* work = a.work + (int64_t)k * a.layer_stride;
  uint8_t* keep = a.layer + (int64_t)k * a.layer_stride;
  uint8_t* cells = a.cells + (int64_t)k * a.stride;
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < 2) a.layer_origins[2 * (size_t)k + threadIdx.x] = a.origins[2 * (size_t)k + threadIdx.x];
  const bool some = inflation_tile_seeds(masks, table, seen, work, lp, sx, sy, tx, ty, R, a.table, lane, wave);
  const int i = tx + lane;
  for (int j = wave; j < kInflateTile && ty + j < sy; j += kInflateWaves) {
    const int l = ty + j, r0 = j + R;
    if (i >= sx) continue;                             // (nothing below is a wave operation)
    // 0 <= i < size_x, 0 <= l < size_y: this tile's own cell, in the layers and in the window
    const int v = work[(int64_t)l * lp + i];
    keep[(int64_t)l * lp + i] = (uint8_t)v;
    uint8_t* p = cells + (int64_t)l * a.pitch + i;
    if (v != 255) {
      const int old = *p;
      if (old == 255 || old < v) *p = (uint8_t)v;
    }
    if (!some) continue;
    const int best = inflation_tile_distance(masks, R, r0, lane);
    if (best <= R * R) inflation_combine(p, table, best);
  }
}

}  // namespace
}  // namespace neo_mpc
