// rolling_window.h -- K7: a fleet's rolling costmap windows, cut from one world map on the device
// (the contract: include/neo_mpc.h, neo_mpc_window_batch).  Part of libneo_mpc.so's device code (included by
// neo_mpc_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "costmap_ingest.h"
#include "neo_mpc_device.h"
#include "wave_ops.h"

namespace neo_mpc {
namespace {

constexpr int kRollWaves = 4;        // windows per workgroup of k_roll_index: one wave each, no LDS, no barrier
constexpr int kRollUnroll = 4;       // 16-byte chunks per thread of k_roll_fill
constexpr int kRollOutside = -1;     // index table: worldToMap refuses this column / row -> outside_value
constexpr int kRollLethal = -2;      // index table: a column beyond the window's right edge (table padding) -> 254

// The contract's float64 expressions, one correctly rounded operation each: hipcc contracts a * b + c into an fma by
// default, and on a window lattice half a cell off the world's a fused ox + (i + 0.5) * res lands in another world cell.
// updateOrigin along one axis: the window's new origin for a robot at `x`.
__device__ __forceinline__ double roll_origin(double x, double o, int size, double res) {
#pragma clang fp contract(off)
  const double s = ((double)(size - 1) + 0.5) * res;   // getSizeInMetersX
  const double n = x - s / 2.0;
  const double q = (n - o) / res;
  const int c = fabs(q) < 2147483648.0 ? (int)q : 0;   // (NaN and infinities compare false: no move)
  return o + (double)c * res;
}
// mapToWorld of the window's cell `i`, then worldToMap on the world map: its column / row there, or kRollOutside
__device__ __forceinline__ int roll_cell(double o, int i, double res, double wo, double wres, int wsize) {
#pragma clang fp contract(off)
  const double w = o + ((double)i + 0.5) * res;
  if (w < wo) return kRollOutside;
  const double q = (w - wo) / wres;
  if (!(q < (double)wsize)) return kRollOutside;       // (compared in float64: NaN and +inf are outside too)
  return (int)q;                                       // 0 <= q < wsize
}

// K7a: one wave per window.  Writes the window's new origin -- final before any workgroup of k_roll_fill (the next launch on
// the stream) reads it -- and the two index tables of the fill: the cell indices are separable, the world column depends
// on the window and its column alone and the world row on the window and its row, so a window costs size_x + size_y float64
// divisions instead of size_x * size_y.  tables[k] = tab_x column entries (size_x rounded up to 16, the rest kRollLethal:
// the fill reads them sixteen at a time), then size_y row entries.
__global__ __launch_bounds__(kLanes * kRollWaves) void k_roll_index(const RollArgs a) {
  const int lane = threadIdx.x & (kLanes - 1);
  const size_t k = (size_t)blockIdx.x * kRollWaves + (size_t)uniform_int((int)(threadIdx.x >> 6));
  if (k >= a.count) return;
  double ox = a.origins[2 * k], oy = a.origins[2 * k + 1];
  if (a.poses || a.problems) {
    const double x = a.poses ? a.poses[3 * k] : a.problems[k].cur_xy[0];
    const double y = a.poses ? a.poses[3 * k + 1] : a.problems[k].cur_xy[1];
    ox = roll_origin(x, ox, a.size_x, a.res);
    oy = roll_origin(y, oy, a.size_y, a.res);
    if (lane == 0) { a.origins[2 * k] = ox; a.origins[2 * k + 1] = oy; }
  }
  int32_t* tx = a.tables + k * (size_t)a.tab_stride;
  int32_t* ty = tx + a.tab_x;
  for (int i = lane; i < a.tab_x; i += kLanes)
    tx[i] = i < a.size_x ? roll_cell(ox, i, a.res, a.wox, a.wres, a.wsx) : kRollLethal;
  for (int j = lane; j < a.size_y; j += kLanes) ty[j] = roll_cell(oy, j, a.res, a.woy, a.wres, a.wsy);
}

// K7b: the fill, K3's stream (costmap_ingest.h: stream_padded_map) -- 254 in the border and the pitch padding -- with gathered
// bytes of the world map (a few MB: it stays in cache) as the source.
typedef int32_t roll_i32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ u32x4 roll_chunk(const RollArgs& a, const int32_t* tx, int my, int mx0) {
  // (the border is a multiple of 16: a chunk never straddles column 0)
  u32x4 v = {0xFEFEFEFEu, 0xFEFEFEFEu, 0xFEFEFEFEu, 0xFEFEFEFEu};
  if (my >= 0 && my < a.size_y && mx0 >= 0 && mx0 < a.size_x) {
    const int wy = tx[a.tab_x + my];
    const uint8_t* wrow = a.world + (int64_t)(wy < 0 ? 0 : wy) * a.wsx;
    const roll_i32x4* t4 = reinterpret_cast<const roll_i32x4*>(tx + mx0);   // (mx0 + 16 <= tab_x; 16-byte aligned)
    uint32_t w[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const roll_i32x4 c = t4[g];
      const int cx[4] = {c.x, c.y, c.z, c.w};
      uint32_t word = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        uint32_t cell = cx[e] == kRollLethal ? 254u : a.outside;
        if (cx[e] >= 0 && wy >= 0) cell = wrow[cx[e]];
        word |= cell << (8 * e);
      }
      w[g] = word;
    }
    v = u32x4{w[0], w[1], w[2], w[3]};
  }
  return v;
}
__global__ __launch_bounds__(256) void k_roll_fill(const RollArgs a) {
  const int32_t* tx = a.tables + (size_t)blockIdx.y * a.tab_stride;   // blockIdx.y: which window
  stream_padded_map<kRollUnroll>(a, blockDim.x, [&](int my, int mx0) { return roll_chunk(a, tx, my, mx0); });
}

}  // namespace
}  // namespace neo_mpc
