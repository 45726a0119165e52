// grid_planner.h -- K16: detours for a fleet's blocked plans, searched on the live world map (the contract: include/neo_mpc.h,
// neo_mpc_replan_batch; its executable form: tests/grid_planner_reference.py).  Integers alone; one workgroup per robot that
// waits for no other; every loop bounded by the window.
// Part of libneo_mpc.so's device code (included by neo_mpc_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "footprint_gate.h"

namespace neo_mpc {
namespace {

constexpr int kReplanThreads = 256;
constexpr uint32_t kNoPath = 0xffffffffu;   // G of a cell no path leaves
constexpr uint32_t kReplanWall = 255;       // the tile's marker of a cell that is not traversable (costs are 0 .. 253)

// The LDS of one workgroup for windows of up to kMaxW cells, in dwords: G with its one-cell border, the walked path as tile
// indices (16 bits each: 130 * 130 < 2^16), the tile's bytes, the walk's two result words.  kMaxW 128: 117 276 B of 160 KiB
// (__syncthreads_or adds a word of its own).
template <int kMaxW> struct ReplanLds {
  static constexpr int kPitch = kMaxW + 2;
  static constexpr int kG = 0;
  static constexpr int kPath = kG + kPitch * kPitch;
  static constexpr int kTile = kPath + kMaxW * kMaxW / 2;
  static constexpr int kWalk = kTile + (kPitch * kPitch + 3) / 4;
  static constexpr int kDwords = kWalk + 2;
};

__device__ __forceinline__ uint32_t lds_load(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void lds_store(uint32_t* p, uint32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// min over the eight moves that leave tile cell `at` of step + G(target) -> that minimum (kNoPath: none) and, in `to`, the
// target of the first direction that reaches it.  Pitch P; the border and every wall hold kReplanWall, so no index is
// tested.  The sixteen LDS reads do not depend on one another; what a diagonal needs of its two side cells is among them.
__device__ __forceinline__ uint32_t best_move(const uint32_t* G, const uint8_t* tile, int at, int P, uint32_t neutral, int& to) {
  const int off[8] = {1, P + 1, P, P - 1, -1, -P - 1, -P, -P + 1};   // E, NE, N, NW, W, SW, S, SE
  uint32_t m[8], g[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) { m[k] = tile[at + off[k]]; g[k] = lds_load(G + at + off[k]); }
  uint32_t best = kNoPath;
  to = at;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    bool ok = m[k] != kReplanWall && g[k] != kNoPath;
    if (k & 1) ok = ok && m[k - 1] != kReplanWall && m[(k + 1) & 7] != kReplanWall;
    const uint32_t cand = ((k & 1) ? 14u : 10u) * (neutral + m[k]) + g[k];
    if (ok && cand < best) { best = cand; to = at + off[k]; }   // (strict: the lowest k keeps a tie)
  }
  return best;
}

// The centre of cell `cell` along one axis: one rounded multiply, one rounded add.  (HIP's *_rn intrinsics are a plain
// product and sum to this compiler, which then fuses them: contraction is switched off for these two operations instead.)
__device__ __forceinline__ double cell_centre(double origin, int cell, double res) {
#pragma clang fp contract(off)
  const double across = ((double)cell + 0.5) * res;
  return origin + across;
}

// The move between two neighbouring tile cells as its direction k
__device__ __forceinline__ int direction_of(int from, int to, int P) {
  const int dy = to / P - from / P, dx = to % P - from % P;
  // (dy + 1) * 3 + (dx + 1) -> k, four bits each: SW S SE / W - E / NW N NE
  return (int)((0x123004765ull >> (4 * ((dy + 1) * 3 + dx + 1))) & 7);
}

template <int kMaxW>
__global__ __launch_bounds__(kReplanThreads) void k_replan(const ReplanArgs a) {
  using L = ReplanLds<kMaxW>;
  __shared__ uint32_t lds[L::kDwords];
  uint32_t* G = lds + L::kG;
  uint16_t* path = reinterpret_cast<uint16_t*>(lds + L::kPath);
  uint8_t* tile = reinterpret_cast<uint8_t*>(lds + L::kTile);
  uint32_t* walk = lds + L::kWalk;
  const int lane = threadIdx.x;
  const size_t b = blockIdx.x;
  if (b >= a.count) return;
  // ---- 1: the cells, the window, the early statuses: the same in every lane, and every return in front of the first barrier
  neo_mpc_replan out;
  out.status = 0; out.length = 0; out.cost = 0; out.window_x0 = 0; out.window_y0 = 0; out.reserved = 0;
  if (a.checks && a.checks[b].status != 1) {
    out.status = 4;
    if (lane == 0) a.results[b] = out;
    return;
  }
  int sx, sy, gx, gy;
  const bool s_off = off_map_cell(a.starts[2 * b], a.starts[2 * b + 1], a.wox, a.woy, a.wres, a.winv, a.wsx, a.wsy, sx, sy);
  const bool g_off = off_map_cell(a.goals[2 * b], a.goals[2 * b + 1], a.wox, a.woy, a.wres, a.winv, a.wsx, a.wsy, gx, gy);
  if (s_off || g_off) {
    out.status = 3;
    if (lane == 0) a.results[b] = out;
    return;
  }
  const int W = (int)a.window < kMaxW ? (int)a.window : kMaxW, P = W + 2;   // (the launch picks kMaxW >= window)
  const int x_last = a.wsx - W > 0 ? a.wsx - W : 0, y_last = a.wsy - W > 0 ? a.wsy - W : 0;
  int x0 = (sx + gx) / 2 - W / 2, y0 = (sy + gy) / 2 - W / 2;
  x0 = x0 < 0 ? 0 : (x0 > x_last ? x_last : x0);
  y0 = y0 < 0 ? 0 : (y0 > y_last ? y_last : y0);
  out.window_x0 = x0; out.window_y0 = y0;
  const uint32_t max_cost = a.max_cost, unknown_cost = a.unknown_cost, neutral = a.neutral_cost;
  // (s and g are cells of the map; the window's far side alone is left to test)
  const bool in_window = sx >= x0 && sx < x0 + W && sy >= y0 && sy < y0 + W && gx >= x0 && gx < x0 + W && gy >= y0 && gy < y0 + W;
  if (!in_window) {
    out.status = 3;
    if (lane == 0) a.results[b] = out;
    return;
  }
  int32_t* cells_out = a.path_cells + 2 * (b * (size_t)a.max_path_cells);
  double* poses_out = a.path_poses ? a.path_poses + 3 * (b * (size_t)a.max_path_cells) : nullptr;
  if (sx == gx && sy == gy) {   // the robot stands on its goal: one cell, whatever it holds
    out.length = 1;
    if (lane == 0) {
      cells_out[0] = sx; cells_out[1] = sy;
      if (poses_out) {
        poses_out[0] = cell_centre(a.wox, sx, a.wres);
        poses_out[1] = cell_centre(a.woy, sy, a.wres);
        poses_out[2] = 0.0;
      }
      a.results[b] = out;
    }
    return;
  }
  {
    const uint32_t v = a.world[(long)gy * a.wsx + gx];
    if (!(v == 255 ? unknown_cost > 0 : v < max_cost)) {
      out.status = 2;
      if (lane == 0) a.results[b] = out;
      return;
    }
  }
  const int s_at = (sy - y0 + 1) * P + (sx - x0 + 1), g_at = (gy - y0 + 1) * P + (gx - x0 + 1);
  // ---- 2, 3: the window's bytes as costs or walls inside a border of walls; G = none, the goal 0
  for (int at = lane; at < P * P; at += kReplanThreads) {
    const int ly = at / P, lx = at - ly * P;
    const int mx = x0 + lx - 1, my = y0 + ly - 1;   // (>= 0 wherever lx, ly >= 1)
    uint32_t m = kReplanWall;
    if (lx >= 1 && lx <= W && ly >= 1 && ly <= W && mx < a.wsx && my < a.wsy) {
      const uint32_t v = a.world[(long)my * a.wsx + mx];
      if (v == 255) m = unknown_cost > 0 ? unknown_cost : kReplanWall;
      else if (v < max_cost) m = v;
    }
    tile[at] = (uint8_t)m;
    G[at] = at == g_at ? 0u : kNoPath;
  }
  __syncthreads();
  // ---- 4: relax to the fixpoint.  Lanes stride over the window's W * W cells, 256 cells a round; a cell pulls the minimum
  // over its moves and is written by its own lane alone.  In place: a value read is either this sweep's or the last one's,
  // both a real path's cost, and values only fall -- the fixpoint is Jacobi's.  A sweep without a change saw one state of G
  // from end to end: that state is the fixpoint.  Bellman-Ford needs at most W * W - 1 sweeps; the loop has W * W.
  const int rows_a_round = kReplanThreads / W, cols_a_round = kReplanThreads % W;
  const int ly0 = lane / W, lx0 = lane % W;
  for (int sweep = 0; sweep < W * W; ++sweep) {
    int changed = 0;
    int ly = ly0, lx = lx0;
    for (int c = lane; c < W * W; c += kReplanThreads) {
      const int at = (ly + 1) * P + lx + 1;
      if ((tile[at] != kReplanWall || at == s_at) && at != g_at) {   // moves leave a traversable cell, and the start cell
        int to;
        const uint32_t best = best_move(G, tile, at, P, neutral, to);
        if (best < lds_load(G + at)) { lds_store(G + at, best); changed = 1; }
      }
      ly += rows_a_round; lx += cols_a_round;
      if (lx >= W) { lx -= W; ++ly; }
    }
    if (!__syncthreads_or(changed)) break;
  }
  // ---- 5: the walk, one lane: at most W * W - 1 moves.  (The sweeps ended at a barrier.)
  if (lane == 0) {
    uint32_t length = 0;
    const uint32_t cost = G[s_at];
    if (cost != kNoPath) {
      int at = s_at;
      path[0] = (uint16_t)at;
      length = 1;
      for (int moves = 0; moves < W * W - 1 && at != g_at; ++moves) {
        int to;
        if (best_move(G, tile, at, P, neutral, to) == kNoPath) break;   // (no cell with a G is without a move)
        at = to;
        path[length++] = (uint16_t)at;
      }
      if (at != g_at) length = 0;
    }
    walk[0] = length;
    walk[1] = length ? cost : 0;
  }
  __syncthreads();
  // ---- 6: the path out, all lanes; the record, lane 0
  const uint32_t length = walk[0];
  out.length = length; out.cost = walk[1];
  out.status = length == 0 ? 1 : (length > a.max_path_cells ? 5 : 0);
  const uint32_t n = length < a.max_path_cells ? length : a.max_path_cells;
  for (uint32_t j = lane; j < n; j += kReplanThreads) {
    const int at = path[j];
    const int mx = x0 + at % P - 1, my = y0 + at / P - 1;
    cells_out[2 * (size_t)j] = mx; cells_out[2 * (size_t)j + 1] = my;
    if (poses_out) {
      int k = 0;
      if (j + 1 < length) k = direction_of(at, path[j + 1], P);
      else if (j > 0) k = direction_of(path[j - 1], at, P);
      // the header's table: k * (pi / 4) for k <= 4, (k - 8) * (pi / 4) beyond -- a product with a power of two times pi
      // rounds like pi's own multiple, so the one multiply gives the table's bits
      poses_out[3 * (size_t)j] = cell_centre(a.wox, mx, a.wres);
      poses_out[3 * (size_t)j + 1] = cell_centre(a.woy, my, a.wres);
      poses_out[3 * (size_t)j + 2] = (double)(k <= 4 ? k : k - 8) * 0.7853981633974483;
    }
  }
  if (lane == 0) a.results[b] = out;
}

}  // namespace
}  // namespace neo_mpc
