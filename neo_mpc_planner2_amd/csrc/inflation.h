// inflation.h -- what K8 (fleet_stamp.h) and K9 (world_inflation.h) share of nav2's inflation by squared cell distance: the cost
// table T in LDS, the rule that combines T[N] with a cell, and the scan over rows of seeds for N, a cell's squared distance to
// the nearest one -- K9's; K8 keeps a written-out copy that measured faster there.  What a row looks like stays with the kernels.
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

// nav2's inflation rule, inflate_unknown false, on the cell at `p` for the squared distance `best` <= R^2: one byte read,
// combined, written back where it changed
__device__ __forceinline__ void inflation_combine(uint8_t* p, const uint8_t* table, int best) {
  const int cost = table[best], old = *p;
  const int now = old == 255 ? (cost >= 253 ? cost : 255) : (cost > old ? cost : old);
  if (now != old) *p = (uint8_t)now;
}

}  // namespace
}  // namespace neo_mpc
