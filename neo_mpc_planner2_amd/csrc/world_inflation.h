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

// K9: one workgroup of four waves per tile of 64 x 64 cells, one fused pass.
//   1  The tile's halo becomes a bitmask of seeds in LDS (inflation_tile_seeds).
//   2  A tile without a seed in its halo -- most of a yard -- is done: it reads nothing a second time and never loads the table.
//   3  Otherwise every cell of the tile takes T[N], N its squared distance to the nearest seed (inflation_tile_distance): one
//      byte read, combined by nav2's rule, written back where it changed.
// IN PLACE, without a snapshot of the map.  A workgroup reads bytes of its neighbours' tiles (its halo) while their owners may
// be rewriting them, and that is safe because the only thing it reads of a foreign byte is whether it equals 254, and no write
// of this kernel changes that: a cell that is 254 has N = 0 and stays max(254, T[0]) = 254, and a cell that is not gets
// T[N >= 1] <= 253, the maximum of that with a value other than 254, or keeps 255.  So step 1 sees the seeds of the map as it
// was when the launch started whichever value of a foreign byte -- old or new, from whatever cache -- it is served: the kernel
// depends on no visibility of another workgroup's write, on any XCD.  The value of a cell (step 3's `old`) is read by the one
// lane that owns the cell, whose workgroup is the only writer of the tile: each byte has one reader of its value and one
// writer, the same lane, once.  Byte stores merge into their line by byte mask; no two lanes write one byte.  No atomics.
__global__ __launch_bounds__(kLanes * kInflateWaves) void k_inflate_world(const InflateArgs a) {
  __shared__ uint64_t masks[kInflateRows * 3];
  __shared__ uint8_t table[kInflationTableBytes];
  __shared__ int seen[kInflateWaves];
  const int lane = threadIdx.x & (kLanes - 1), wave = uniform_int((int)(threadIdx.x >> 6));
  const int R = a.reach, sx = a.wsx, sy = a.wsy;
  const int tx = (int)blockIdx.x * kInflateTile, ty = (int)blockIdx.y * kInflateTile;   // the tile's first column and row
  if (!inflation_tile_seeds(masks, table, seen, a.world, sx, sx, sy, tx, ty, R, a.table, lane, wave)) return;
  const int i = tx + lane;
  for (int k = wave; k < kInflateTile && ty + k < sy; k += kInflateWaves) {
    const int l = ty + k, r0 = k + R;                  // the cell's row in the map and in the masks
    const int best = inflation_tile_distance(masks, R, r0, lane);
    // 0 <= i < wsx, 0 <= l < wsy: this tile's own cell
    if (best <= R * R && i < sx) inflation_combine(a.world + (int64_t)l * sx + i, table, best);
  }
}

}  // namespace
}  // namespace neo_mpc
