// inflation.h -- what K8 (fleet_stamp.h), K9 (world_inflation.h) and K10 (scan_layer.h) share of nav2's inflation by squared cell distance: the cost
// table T in LDS, the rule that combines T[N] with a cell, and the scan over rows of seeds for N, a cell's squared distance to
// the nearest one -- K9's and K10's; K8 keeps a written-out copy that measured faster there -- and K9's and K10's tiled pass:
// the tile constants, a tile's halo as rows of three 64-bit words of seeds in LDS, and a cell's N from those rows.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "neo_mpc_device.h"

namespace neo_mpc {
namespace {

constexpr int kInflationTableBytes = (NEO_MPC_MAX_INFLATION_CELLS * NEO_MPC_MAX_INFLATION_CELLS + 1 + 15) & ~15;   // T[0 .. R^2] in LDS

// T -> LDS, by the `threads` threads of a workgroup (`tid`: this one); the caller's barrier stands behind it
__device__ __forceinline__ void inflation_stage_table(uint8_t* lds, const uint8_t* table, int R, int tid, int threads) {
  for (int t = tid; t <= R * R; t += threads) lds[t] = table[t];
}

// The squared distance from a cell to the nearest seed within R rows, or R^2 + 1: the minimum over the rows dy = 0, +-1, ...
// of dy^2 + hd^2, ending when dy^2 reaches the best so far.  `row(dy, found)`: if the row dy away from the cell's has a seed,
// calls found(hd), hd the distance along it to the nearest one.
template <class Row>
__device__ __forceinline__ int inflation_scan(int R, Row&& row) {
  int best = R * R + 1;
  for (int d = 0; d <= R && d * d < best; ++d) {
    const auto found = [&](int hd) { const int v = d * d + hd * hd; best = v < best ? v : best; };
    row(d, found);
    if (d > 0) row(-d, found);
  }
  return best;
}

constexpr int kInflateFar = 1 << 12;   // "no seed in this row": its square is beyond every R^2, and fits an int with d^2 added

// Distance along a row from column 64 + c of a 192-column row (m0: columns 0 .. 63, m1: 64 .. 127, m2: 128 .. 191; bit b of
// a word = its column b; 0 <= c < 64) to the row's nearest set bit -- K8's stamp_row_distance over three words.  Exact up to 64,
// which is all a reach of at most 64 cells can ask for; kInflateFar where no bit is that near.
__device__ __forceinline__ int inflate_row_distance(uint64_t m0, uint64_t m1, uint64_t m2, int c) {
  // the 64 columns that end at the column, the nearest in bit 63; the 64 that start at it, the nearest in bit 0
  const uint64_t left = (m1 << (63 - c)) | ((m0 >> c) >> 1);
  const uint64_t right = (m1 >> c) | ((m2 << (63 - c)) << 1);
  // (a distance of exactly 64 is the one column on either side that those windows leave out)
  const int dl = left ? __clzll((long long)left) : ((m0 >> c) & 1 ? 64 : kInflateFar);
  const int dr = right ? __ffsll((long long)right) - 1 : ((m2 >> c) & 1 ? 64 : kInflateFar);
  return dl < dr ? dl : dr;
}

constexpr int kInflateTile = 64;    // a workgroup owns 64 x 64 cells: lane = column, one 64-bit word per row and 64 columns
constexpr int kInflateWaves = 4;    // ... its waves take the rows in turn
constexpr int kInflateLoads = 8;    // ... each with this many row words in flight
constexpr int kInflateRows = kInflateTile + 2 * NEO_MPC_MAX_INFLATION_CELLS;   // the tile's rows and the largest halo

// Step 1 of K9 and K10, by a workgroup of kInflateWaves waves (`lane`, `wave`: this thread's) for the tile at column tx, row ty
// of the sx x sy map at `src`, rows `pitch` bytes apart.  The tile's halo -- the tile and R cells on every side, clipped to the
// map -- becomes a bitmask of seeds in LDS: a wave reads 64 consecutive bytes of a row and __ballot(cell == 254) is that row's
// word; masks[3 * rr + w] is map row ty - R + rr, columns tx + 64 (w - 1) ... (the tile's columns and the 64 on either side, of
// which the R nearest are read), at most kInflateRows rows: 4.5 KB.  Then, if any wave saw a seed (`seen`: a vote per wave), T
// goes to `lds_table`.  Returns whether one did, the same in every lane of the workgroup, behind the second of two barriers.
// Both barriers are unconditional, and the trip counts of the loops that ballot are wave-uniform: all 64 lanes of a wave run
// every turn.  A wave's words go kInflateLoads at a time: the loads of a batch are in flight together -- one after the other,
// a tile without a seed, which does little else, is the sum of their latencies.
__device__ __forceinline__ bool inflation_tile_seeds(uint64_t* masks, uint8_t* lds_table, int* seen, const uint8_t* src, int pitch,
                                                     int sx, int sy, int tx, int ty, int R, const uint8_t* table, int lane, int wave) {
  const int rows = kInflateTile + 2 * R;
  const int c_lo = tx - R > 0 ? tx - R : 0;            // the halo's columns that exist: [c_lo, c_hi)
  const int c_hi = tx + kInflateTile + R < sx ? tx + kInflateTile + R : sx;
  bool any = false;
  for (int t0 = wave; t0 < rows * 3; t0 += kInflateWaves * kInflateLoads) {
    int cell[kInflateLoads];
#pragma unroll
    for (int u = 0; u < kInflateLoads; ++u) {
      const int t = t0 + u * kInflateWaves, rr = t / 3, w = t - 3 * rr;
      const int r = ty - R + rr, col = tx + (w - 1) * kInflateTile + lane;
      cell[u] = 0;
      if (t < rows * 3 && r >= 0 && r < sy && col >= c_lo && col < c_hi) cell[u] = src[(int64_t)r * pitch + col];   // inside the map
    }
#pragma unroll
    for (int u = 0; u < kInflateLoads; ++u) {
      const int t = t0 + u * kInflateWaves;
      const uint64_t m = __ballot(cell[u] == 254);
      if (t < rows * 3 && lane == 0) masks[t] = m;     // (t < kInflateRows * 3: inside masks)
      any = any || m != 0;
    }
  }
  if (lane == 0) seen[wave] = any ? 1 : 0;
  __syncthreads();
  const bool some = (seen[0] | seen[1] | seen[2] | seen[3]) != 0;
  if (some) inflation_stage_table(lds_table, table, R, (int)threadIdx.x, kLanes * kInflateWaves);
  __syncthreads();
  return some;
}

// The squared distance from the cell in column `lane` of the tile, row r0 of `masks` (R <= r0 < R + kInflateTile, so that
// 0 <= r0 - R and r0 + R < the halo's rows), to the nearest seed of the halo, or R^2 + 1; a row without a seed is skipped
__device__ __forceinline__ int inflation_tile_distance(const uint64_t* masks, int R, int r0, int lane) {
  return inflation_scan(R, [&](int dy, auto&& found) {
    const uint64_t* m = masks + 3 * (r0 + dy);
    const uint64_t m0 = m[0], m1 = m[1], m2 = m[2];
    if (m0 | m1 | m2) found(inflate_row_distance(m0, m1, m2, lane));
  });
}

// nav2's inflation rule, inflate_unknown false, on the cell at `p` for the squared distance `best` <= R^2: one byte read,
// combined, written back where it changed
__device__ __forceinline__ void inflation_combine(uint8_t* p, const uint8_t* table, int best) {
  const int cost = table[best], old = *p;
  const int now = old == 255 ? (cost >= 253 ? cost : 255) : (cost > old ? cost : old);
  if (now != old) *p = (uint8_t)now;
}

}  // namespace
}  // namespace neo_mpc
