// world_scan_denoise.h -- K13: the speckle filter of the fleet's shared obstacle layer, step 3b of the contract of
// neo_mpc_update_world_scan_layer (include/neo_mpc.h, neo_mpc_set_world_scan_denoise): a mark whose group of occupied cells
// has fewer than G members reaches the composition as a free cell.  One launch between K12's footprints and its composition,
// enqueued only while the filter is on.  Part of libneo_mpc.so's device code (included by neo_mpc_kernels.hip).
//
// `layer` and `world` are read and not written; `denoised` (D), WSX bytes a row like them, is rewritten whole.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "inflation.h"
#include "neo_mpc_device.h"
#include "wave_ops.h"

namespace neo_mpc {
namespace {

constexpr int kDenoiseMaxHalo = (int)NEO_MPC_MAX_DENOISE_GROUP - 1;        // H = G - 1 cells on every side of the tile
constexpr int kDenoiseRows = kInflateTile + 2 * kDenoiseMaxHalo;           // the tile's rows and the largest halo: 94
constexpr int kDenoiseOwnRows = kInflateTile / kInflateWaves;              // the rows of the tile a wave owns: 16

// The occupancy of the halo around the tile at column tx, row ty -- the tile and H cells on every side, clipped to the world --
// as rows of three 64-bit words in LDS, laid out as inflation_tile_seeds lays out its seeds: masks[3 * rr + w] is world row
// ty - H + rr, columns tx + 64 (w - 1) ..., bit b = column b of the word; a cell is occupied when the layer or the world map
// holds 254 there.  The middle words of the tile's own rows are NOT loaded here: the caller has written them from the bytes
// it read anyway.  Every trip count is wave-uniform and all 64 lanes run every __ballot; kInflateLoads words of a wave are in
// flight together, two loads each.  The caller's barrier stands behind it.
__device__ __forceinline__ void denoise_tile_occupancy(uint64_t* masks, const uint8_t* layer, const uint8_t* world, int sx, int sy,
                                                       int tx, int ty, int H, int lane, int wave) {
  const int rows = kInflateTile + 2 * H;
  const int c_lo = tx - H > 0 ? tx - H : 0;            // the halo's columns that exist: [c_lo, c_hi)
  const int c_hi = tx + kInflateTile + H < sx ? tx + kInflateTile + H : sx;
  for (int t0 = wave; t0 < rows * 3; t0 += kInflateWaves * kInflateLoads) {
    int a[kInflateLoads], b[kInflateLoads];
#pragma unroll
    for (int u = 0; u < kInflateLoads; ++u) {
      const int t = t0 + u * kInflateWaves, rr = t / 3, w = t - 3 * rr;
      const int r = ty - H + rr, col = tx + (w - 1) * kInflateTile + lane;
      const bool own = w == 1 && rr >= H && rr < H + kInflateTile;
      a[u] = 0; b[u] = 0;
      if (t < rows * 3 && !own && r >= 0 && r < sy && col >= c_lo && col < c_hi) {   // inside the world
        const int64_t at = (int64_t)r * sx + col;
        a[u] = layer[at]; b[u] = world[at];
      }
    }
#pragma unroll
    for (int u = 0; u < kInflateLoads; ++u) {
      const int t = t0 + u * kInflateWaves, rr = t / 3, w = t - 3 * rr;
      const bool own = w == 1 && rr >= H && rr < H + kInflateTile;
      const uint64_t m = __ballot(a[u] == 254 || b[u] == 254);
      if (t < rows * 3 && !own && lane == 0) masks[t] = m;   // (t < kDenoiseRows * 3: inside masks)
    }
  }
}

// Bits [s, s + 32) of the 192-column row (m0, m1, m2), 1 <= s <= 127
__device__ __forceinline__ uint32_t denoise_row_window(uint64_t m0, uint64_t m1, uint64_t m2, int s) {
  const uint64_t lo = s < 64 ? m0 : m1, hi = s < 64 ? m1 : m2;
  const int k = s & 63;
  return (uint32_t)((lo >> k) | ((hi << (63 - k)) << 1));
}

// Whether the group of the occupied cell in column `lane` of the tile, row r0 of `masks` (H <= r0 < H + kInflateTile), has
// fewer than G = H + 1 cells.  B_k: the occupied cells within k neighbour steps of the cell through occupied cells.  B_k gains
// at least one cell per step until the group is exhausted, and B_H lies inside the (2 H + 1)^2 window around the cell, so the
// group has at least G cells iff |B_H| >= G: at most H masked dilations of a bitmask of 2 kH + 1 rows of as many bits, kH >= H
// the compiled window (the rows live in registers: every index below is a constant once unrolled).  Rows further than H from
// the cell are never read; columns further than H are, and cannot be reached in H steps.  Ends early once the count
// reaches G or stops growing.  No wave operation in here: lanes come and go as their cells ask.
template <int kH>
__device__ __forceinline__ bool denoise_group_is_small(const uint64_t* masks, int H, int r0, int lane, bool eight) {
  constexpr int kW = 2 * kH + 1;
  constexpr uint32_t kBits = (uint32_t)((1ull << kW) - 1ull);
  const int s = kInflateTile + lane - kH;              // the window's first column in the row of 192: 49 .. 126
  uint32_t occ[kW], ball[kW];
#pragma unroll
  for (int k = 0; k < kW; ++k) { occ[k] = 0u; ball[k] = 0u; }
  const auto row = [&](int dy) {                        // -H <= dy <= H, so that 0 <= r0 + dy < the halo's rows
    const uint64_t* m = masks + 3 * (r0 + dy);
    return denoise_row_window(m[0], m[1], m[2], s) & kBits;
  };
  occ[kH] = row(0);
  ball[kH] = 1u << kH;                                  // B_0: the cell itself
  int count = 1;
  // (`step` is the same in every lane that is still here: the tests on it below are scalar branches)
  for (int step = 0; step < H; ++step) {
    uint32_t prev = 0u;                                 // the row above as it was before this step
    int now = 0;
#pragma unroll
    for (int k = 0; k < kW; ++k) {
      const int dy = k - kH, far = dy < 0 ? -dy : dy;
      const uint32_t cur = ball[k], next = k + 1 < kW ? ball[k + 1] : 0u;
      // B_step lies within `step` rows of the cell: a row further than step + 1 stays empty, and the row step + 1 away is
      // read from LDS only now -- a cell in a large group reads the few rows its ball needs to reach G, not all 2 H + 1
      if (far <= step + 1) {
        if (far == step + 1) occ[k] = row(dy);          // (step + 1 <= H)
        const uint32_t up_down = prev | next;
        const uint32_t wide = eight ? (cur | up_down) : cur;
        const uint32_t grown = (wide | (wide << 1) | (wide >> 1) | up_down) & occ[k];
        ball[k] = grown;
        now += __popc(grown);
      }
      prev = cur;
    }
    if (now > H) return false;                          // G cells or more
    if (now == count) return true;                      // the group is exhausted below G
    count = now;
  }
  return count <= H;
}

// K13, step 3b of the contract, on K9's and K12's tile scheme: grid (tile column, tile row), one workgroup of four waves per
// tile of 64 x 64 cells, lane = column, a wave owns every fourth row.
//   1  Every cell of the tile: its layer byte goes to D, the occupancy of its row to LDS, and the lane remembers whether the
//      cell is a candidate (layer 254 over a world cell that is not 254).  A vote per wave.
//   2  A tile with a candidate loads the occupancy of its halo (denoise_tile_occupancy); a tile without one is done.
//   3  A candidate whose group is small (denoise_group_is_small) gets D = 0.
// A byte of D is written, in step 1 and again in step 3, by the one lane that owns its cell, in program order.  Both barriers
// are unconditional; every loop is bounded by G or by the tile; no atomics.  kH: the compiled window, >= a.group - 1.
template <int kH>
__global__ __launch_bounds__(kLanes * kInflateWaves) void k_world_scan_denoise(const WorldScanArgs a) {
  __shared__ uint64_t masks[kDenoiseRows * 3];
  __shared__ int seen[kInflateWaves];
  const int lane = threadIdx.x & (kLanes - 1), wave = uniform_int((int)(threadIdx.x >> 6));
  const int H = (int)a.group - 1, sx = a.wsx, sy = a.wsy;
  const int tx = (int)blockIdx.x * kInflateTile, ty = (int)blockIdx.y * kInflateTile;
  const int i = tx + lane;
  const bool eight = a.connectivity == 8u;
  uint32_t candidates = 0u;                             // bit u: this lane's cell in row wave + 4 u is one
  bool any = false;
  for (int u0 = 0; u0 < kDenoiseOwnRows; u0 += kInflateLoads) {
    int v[kInflateLoads], w[kInflateLoads];
#pragma unroll
    for (int u = 0; u < kInflateLoads; ++u) {
      const int l = ty + wave + kInflateWaves * (u0 + u);
      v[u] = 0; w[u] = 0;
      // 0 <= i < wsx, 0 <= l < wsy: this tile's own cell, in the layer and the world map
      if (i < sx && l < sy) { const int64_t at = (int64_t)l * sx + i; v[u] = a.layer[at]; w[u] = a.world[at]; }
    }
#pragma unroll
    for (int u = 0; u < kInflateLoads; ++u) {
      const int j = wave + kInflateWaves * (u0 + u), l = ty + j;
      const uint64_t m = __ballot(v[u] == 254 || w[u] == 254);
      if (lane == 0) masks[3 * (j + H) + 1] = m;        // (j + H < kDenoiseRows)
      // ... and in D
      if (i < sx && l < sy) a.denoised[(int64_t)l * sx + i] = (uint8_t)v[u];
      const bool candidate = v[u] == 254 && w[u] != 254;
      candidates |= candidate ? 1u << (u0 + u) : 0u;
      any = any || __ballot(candidate) != 0ull;
    }
  }
  if (lane == 0) seen[wave] = any ? 1 : 0;
  __syncthreads();
  const bool some = (seen[0] | seen[1] | seen[2] | seen[3]) != 0;   // the same in every lane of the workgroup
  if (some) denoise_tile_occupancy(masks, a.layer, a.world, sx, sy, tx, ty, H, lane, wave);
  __syncthreads();
  if (!some) return;
  for (int u = 0; u < kDenoiseOwnRows; ++u) {
    if (!((candidates >> u) & 1u)) continue;            // (nothing below is a wave operation)
    const int j = wave + kInflateWaves * u;
    // a candidate: 0 <= i < wsx, 0 <= ty + j < wsy
    if (denoise_group_is_small<kH>(masks, H, j + H, lane, eight)) a.denoised[(int64_t)(ty + j) * sx + i] = 0;
  }
}

}  // namespace
}  // namespace neo_mpc
