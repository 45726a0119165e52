// fleet_stamp.h -- K8: a fleet's robots stamped into each other's rolling windows, with nav2's inflation ring
// (the contract: include/neo_mpc.h, neo_mpc_stamp_batch).  Part of libneo_mpc.so's device code (included by
// neo_mpc_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "footprint_gate.h"
#include "inflation.h"
#include "neo_mpc_device.h"
#include "wave_ops.h"

namespace neo_mpc {
namespace {

constexpr int kStampTile = 64;   // a stamp is built 64 x 64 lattice cells at a time: lane = row, one 64-bit word per row

// K8a: one thread per robot.  The polygon in the global frame -- taken as given, or the base-frame footprint oriented by K6's
// own routine into the handle's buffer -- and its bounding box, which is all the search of K8b reads of a robot that is
// out of reach.  A polygon with a vertex that is not finite gets the empty box: it is in reach of no window.
__global__ __launch_bounds__(256) void k_stamp_boxes(const StampArgs a) {
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.count) return;
  const int n = (int)a.points;
  double x = 0.0, y = 0.0, sn = 0.0, cs = 1.0;
  if (!a.polygons) {
    double th;
    footprint_pose(a.poses, a.problems, j, x, y, th);
    sincos(th, &sn, &cs);
  }
  const double* src = a.polygons ? a.polygons + j * 2 * (size_t)n : a.footprint + (a.per_robot ? j * 2 * (size_t)n : 0);
  double x0 = INFINITY, y0 = INFINITY, x1 = -INFINITY, y1 = -INFINITY;
  bool finite = true;
  for (int v = 0; v < n; ++v) {
    double X = src[2 * v], Y = src[2 * v + 1];
    if (!a.polygons) {
      orient_vertex(x, y, sn, cs, X, Y, X, Y);
      double* out = a.polys + (j * (size_t)n + v) * 2;
      out[0] = X; out[1] = Y;
    }
    finite = finite && isfinite(X) && isfinite(Y);
    x0 = fmin(x0, X); x1 = fmax(x1, X); y0 = fmin(y0, Y); y1 = fmax(y1, Y);
  }
  double* box = a.boxes + 4 * j;
  box[0] = finite ? x0 : INFINITY; box[1] = finite ? y0 : INFINITY;
  box[2] = finite ? x1 : -INFINITY; box[3] = finite ? y1 : -INFINITY;
}

// distance along a row from column `c` (any integer) to the nearest set bit of `m` (not zero; bit b = column b)
__device__ __forceinline__ int stamp_row_distance(uint64_t m, int c) {
  const int first = __ffsll((long long)m) - 1, last = 63 - __clzll((long long)m);
  if (c <= first) return first - c;
  if (c >= last) return c - last;
  const uint64_t left = m & (~0ull >> (63 - c));   // bits 0 .. c  (0 < c < 63 here)
  const uint64_t right = m >> c;                   // bits c .. 63, bit c first
  const int dl = c - (63 - __clzll((long long)left));   // (`first` < c: left is not zero)
  const int dr = __ffsll((long long)right) - 1;         // (`last` > c: right is not zero)
  return dl < dr ? dl : dr;
}

// K8b: one workgroup of one wave per window.  The wave searches the whole fleet, 64 bounding boxes at a time, for robots in
// reach of its window (float64, one cell of slack: the cull lets extra robots through and never drops one) and handles
// each survivor the moment it is found, so no neighbour list and no cap exist; a window without neighbours -- most of a
// spread-out fleet -- leaves without touching LDS or the map.  Per survivor the stamp is built 64 x 64 lattice cells at a
// time (a larger polygon simply takes more tiles): lane = lattice row, bit = column, the contract's edge functions unfused.
// Then every window cell within R of the tile takes the minimum over the rows dy in [-R, R] of dy^2 + hd^2, hd the distance
// to the row's nearest set bit (ffs / clz), the scan ending when dy^2 reaches the best so far; T[that] from LDS; one byte
// read, combined, written back where it changed.  The combination is monotone in the cost and T does not increase, so
// applying tiles and robots one after another equals applying the minimum distance once.  A cell belongs to one lane within
// a pass and to different lanes in different passes: a workgroup barrier stands between them.  No atomics (a window is
// written by its own workgroup only), every barrier unconditional, every trip count around one wave-uniform.
__global__ __launch_bounds__(kLanes) void k_stamp_fleet(const StampArgs a) {
#pragma clang fp contract(off)
  __shared__ uint64_t rows[kStampTile];
  __shared__ double verts[2 * NEO_MPC_MAX_FOOTPRINT_POINTS];
  __shared__ uint8_t table[kInflationTableBytes];
  const int lane = threadIdx.x;
  const uint32_t k = blockIdx.x;
  const int n = (int)a.points, R = a.reach, sx = a.size_x, sy = a.size_y;
  const double res = a.res, ox = a.origins[2 * (size_t)k], oy = a.origins[2 * (size_t)k + 1];
  // what is in reach: the window, R cells around it, and one more for the rounding of everything below
  const double slack = (double)(R + 1) * res;
  const double wx0 = ox - slack, wx1 = ox + (double)sx * res + slack;
  const double wy0 = oy - slack, wy1 = oy + (double)sy * res + slack;
  const double* polys = a.polygons ? a.polygons : a.polys;
  uint8_t* cells = a.cells + (int64_t)k * a.stride;
  bool have_table = false;
  for (uint32_t base = 0; base < a.count; base += kLanes) {
    const uint32_t j = base + lane;
    bool in_reach = false;
    if (j < a.count && j != k) {
      const double* box = a.boxes + 4 * (size_t)j;
      in_reach = box[0] <= wx1 && box[2] >= wx0 && box[1] <= wy1 && box[3] >= wy0;   // (the empty box fails)
    }
    uint64_t todo = __ballot(in_reach);
    while (todo) {
      const uint32_t r = base + (uint32_t)(__ffsll((long long)todo) - 1);
      todo &= todo - 1;
      if (!have_table) {
        inflation_stage_table(table, a.table, R, lane, kLanes);
        have_table = true;
      }
      if (lane < n) {
        verts[2 * lane] = polys[((size_t)r * n + lane) * 2];
        verts[2 * lane + 1] = polys[((size_t)r * n + lane) * 2 + 1];
      }
      __syncthreads();
      // the lattice cells whose centre can lie in the robot's box, among those within R of the window: a centre
      // ox + (i + 0.5) res inside [bx0, bx1] has floor((bx0 - ox) / res) - 1 <= i <= floor((bx1 - ox) / res) + 1
      const double* box = a.boxes + 4 * (size_t)r;
      const double lox = fmax(floor((box[0] - ox) / res) - 1.0, (double)-R), hix = fmin(floor((box[2] - ox) / res) + 1.0, (double)(sx - 1 + R));
      const double loy = fmax(floor((box[1] - oy) / res) - 1.0, (double)-R), hiy = fmin(floor((box[3] - oy) / res) + 1.0, (double)(sy - 1 + R));
      const bool some = lox <= hix && loy <= hiy;   // (clamped in float64: the conversions below cannot overflow)
      const int i_lo = uniform_int(some ? (int)lox : 0), i_hi = uniform_int(some ? (int)hix : -1);
      const int l_lo = uniform_int(some ? (int)loy : 0), l_hi = uniform_int(some ? (int)hiy : -1);
      for (int ty = l_lo; ty <= l_hi; ty += kStampTile)
        for (int tx = i_lo; tx <= i_hi; tx += kStampTile) {
          // the stamp's tile: row ty + lane, columns tx .. tx + w - 1
          const int w = i_hi - tx + 1 < kStampTile ? i_hi - tx + 1 : kStampTile;
          uint64_t inside = 0;
          if (ty + lane <= l_hi) {
            const double cy = oy + ((double)(ty + lane) + 0.5) * res;
            uint64_t pos = ~0ull, neg = ~0ull;   // bit c: every edge so far has c_e >= 0 / c_e <= 0 at column tx + c
            for (int e = 0; e < n; ++e) {
              const int f = e + 1 < n ? e + 1 : 0;
              const double ax = verts[2 * e], ay = verts[2 * e + 1];
              const double ex = verts[2 * f] - ax, ey = verts[2 * f + 1] - ay;
              const double along = ex * (cy - ay);
              uint64_t ge = 0, le = 0;
              for (int c = 0; c < w; ++c) {
                const double cx = ox + ((double)(tx + c) + 0.5) * res;
                const double ce = along - ey * (cx - ax);
                ge |= (uint64_t)(ce >= 0.0) << c;
                le |= (uint64_t)(ce <= 0.0) << c;
              }
              pos &= ge; neg &= le;
            }
            inside = pos | neg;   // (columns from w on are zero in ge and le)
          }
          rows[lane] = inside;
          const bool any = __ballot(inside != 0) != 0;
          __syncthreads();
          if (any) {
            // the window's cells within R of the tile
            const int ti0 = tx - R > 0 ? tx - R : 0, ti1 = tx + kStampTile - 1 + R < sx - 1 ? tx + kStampTile - 1 + R : sx - 1;
            const int tl0 = ty - R > 0 ? ty - R : 0, tl1 = ty + kStampTile - 1 + R < sy - 1 ? ty + kStampTile - 1 + R : sy - 1;
            const int tw = ti1 - ti0 + 1, th = tl1 - tl0 + 1;
            const int total = tw > 0 && th > 0 ? tw * th : 0;   // <= (64 + 2 * 64)^2
            for (int idx = lane; idx < total; idx += kLanes) {
              const int dl = idx / tw;
              const int l = tl0 + dl, i = ti0 + (idx - dl * tw);
              const int c = i - tx, r0 = l - ty;
              // (inflation.h's scan, written out: through inflation_scan() this kernel measured 6 to 7 % slower, NOTEBOOK A.16)
              int best = R * R + 1;
              for (int d = 0; d <= R && d * d < best; ++d) {
                const int up = r0 + d, down = r0 - d;
                if ((unsigned)up < (unsigned)kStampTile) {
                  const uint64_t m = rows[up];
                  if (m) { const int hd = stamp_row_distance(m, c), v = d * d + hd * hd; best = v < best ? v : best; }
                }
                if (d > 0 && (unsigned)down < (unsigned)kStampTile) {
                  const uint64_t m = rows[down];
                  if (m) { const int hd = stamp_row_distance(m, c), v = d * d + hd * hd; best = v < best ? v : best; }
                }
              }
              // 0 <= i < size_x, 0 <= l < size_y: this window's own cell
              if (best <= R * R) inflation_combine(cells + (int64_t)l * a.pitch + i, table, best);
            }
          }
          __syncthreads();
        }
    }
  }
}

}  // namespace
}  // namespace neo_mpc
