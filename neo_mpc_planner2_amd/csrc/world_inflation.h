// world_inflation.h -- K9: nav2's inflation layer applied to the handle's copy of the world map, in place (the contract:
// include/neo_mpc.h, neo_mpc_inflate_world_map).  Part of libneo_mpc.so's device code (included by neo_mpc_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "inflation.h"
#include "neo_mpc_device.h"
#include "wave_ops.h"

namespace neo_mpc {
namespace {

constexpr int kInflateTile = 64;    // a workgroup owns 64 x 64 cells: lane = column, one 64-bit word per row and 64 columns
constexpr int kInflateWaves = 4;    // ... its waves take the rows in turn
constexpr int kInflateLoads = 8;    // ... each with this many row words in flight
constexpr int kInflateRows =kInflateTile + 2 * NEO_MPC_MAX_INFLATION_CELLS;   // the tile's rows and the largest halo

// K9: one workgroup of four waves per tile of 64 x 64 cells, one fused pass.
//   1  The tile's halo -- the tile and R cells on every side, clipped to the map -- becomes a bitmask of seeds in LDS: a wave
//      reads 64 consecutive bytes of a row and __ballot(cell == 254) is that row's word; three words per row (the tile's columns
//      and the 64 on either side, of which the R nearest are read), at most 192 rows: 4.5 KB.
//   2  A tile without a seed in its halo -- most of a yard -- is done: it reads nothing a second time and never loads the table.
//   3  Otherwise T goes to LDS and every cell of the tile takes the minimum over the rows dy = 0, +-1, ... of dy^2 + hd^2, hd the
//      distance to the row's nearest seed, the scan ending when dy^2 reaches the best so far and skipping rows without a seed;
//      one byte read, combined by nav2's rule, written back where it changed.
// IN PLACE, without a snapshot of the map.  A workgroup reads bytes of its neighbours' tiles (its halo) while their owners may
// be rewriting them, and that is safe because the only thing it reads of a foreign byte is whether it equals 254, and no write
// of this kernel changes that: a cell that is 254 has N = 0 and stays max(254, T[0]) = 254, and a cell that is not gets
// T[N >= 1] <= 253, the maximum of that with a value other than 254, or keeps 255.  So step 1 sees the seeds of the map as it
// was when the launch started whichever value of a foreign byte -- old or new, from whatever cache -- it is served: the kernel
// depends on no visibility of another workgroup's write, on any XCD.  The value of a cell (step 3's `old`) is read by the one
// lane that owns the cell, whose workgroup is the only writer of the tile: each byte has one reader of its value and one
// writer, the same lane, once.  Byte stores merge into their line by byte mask; no two lanes write one byte.
// No atomics; both barriers are unconditional; the trip counts of the loops that ballot are wave-uniform (all 64 lanes of a
// wave run every turn of step 1's loop).
__global__ __launch_bounds__(kLanes * kInflateWaves) void k_inflate_world(const InflateArgs a) {
  __shared__ uint64_t masks[kInflateRows * 3];
  __shared__ uint8_t table[kInflationTableBytes];
  __shared__ int seen[kInflateWaves];
  const int lane = threadIdx.x & (kLanes - 1), wave = uniform_int((int)(threadIdx.x >> 6));
  const int R = a.reach, sx = a.wsx, sy = a.wsy;
  const int tx = (int)blockIdx.x * kInflateTile, ty = (int)blockIdx.y * kInflateTile;   // the tile's first column and row
  const int rows = kInflateTile + 2 * R;               // masks[3 * rr + w]: map row ty - R + rr, columns tx + 64 (w - 1) ...
  const int c_lo = tx - R > 0 ? tx - R : 0;            // the halo's columns that exist: [c_lo, c_hi)
  const int c_hi = tx + kInflateTile + R < sx ? tx + kInflateTile + R : sx;
  bool any = false;
  // (a wave's words, kInflateLoads at a time: the loads of a batch are in flight together -- one after the other, a tile
  // without a seed, which does nothing else, is the sum of their latencies)
  for (int t0 = wave; t0 < rows * 3; t0 += kInflateWaves * kInflateLoads) {
    int cell[kInflateLoads];
#pragma unroll
    for (int u = 0; u < kInflateLoads; ++u) {
      const int t = t0 + u * kInflateWaves, rr = t / 3, w = t - 3 * rr;
      const int r = ty - R + rr, col = tx + (w - 1) * kInflateTile + lane;
      cell[u] = 0;
      if (t < rows * 3 && r >= 0 && r < sy && col >= c_lo && col < c_hi) cell[u] = a.world[(int64_t)r * sx + col];   // inside the map
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
  const bool some = (seen[0] | seen[1] | seen[2] | seen[3]) != 0;   // the same in every lane of the workgroup
  if (some) inflation_stage_table(table, a.table, R, (int)threadIdx.x, kLanes * kInflateWaves);
  __syncthreads();
  if (!some) return;
  const int i = tx + lane;
  for (int k = wave; k < kInflateTile && ty + k < sy; k += kInflateWaves) {
    const int l = ty + k, r0 = k + R;                  // the cell's row in the map and in the masks
    const int best = inflation_scan(R, [&](int dy, auto&& found) {   // (0 <= r0 - R and r0 + R < rows)
      const uint64_t* m = masks + 3 * (r0 + dy);
      const uint64_t m0 = m[0], m1 = m[1], m2 = m[2];
      if (m0 | m1 | m2) found(inflate_row_distance(m0, m1, m2, lane));   // (a row without a seed is skipped)
    });
    // 0 <= i < wsx, 0 <= l < wsy: this tile's own cell
    if (best <= R * R && i < sx) inflation_combine(a.world + (int64_t)l * sx + i, table, best);
  }
}

}  // namespace
}  // namespace neo_mpc
