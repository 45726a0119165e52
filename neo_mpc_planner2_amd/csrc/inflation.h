// inflation.h -- what K8 (fleet_stamp.h), K9 (world_inflation.h) and K10 (scan_layer.h) share of nav2's inflation by squared cell distance: the cost
// table T in LDS, the rule that combines T[N] with a cell, and the scan over rows of seeds for N, a cell's squared distance to
// the nearest one -- K9's and K10's; K8 keeps a written-out copy that measured faster there -- and the distance along a row of
// three 64-bit words of seeds, which K9 (world_inflation.h) and K10 (scan_layer.h) share.
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

// nav2's inflation rule, inflate_unknown false, on the cell at `p` for the squared distance `best` <= R^2: one byte read,
// combined, written back where it changed
__device__ __forceinline__ void inflation_combine(uint8_t* p, const uint8_t* table, int best) {
  const int cost = table[best], old = *p;
  const int now = old == 255 ? (cost >= 253 ? cost : 255) : (cost > old ? cost : old);
  if (now != old) *p = (uint8_t)now;
}

}  // namespace
}  // namespace neo_mpc
