// costmap_ingest.h -- K3: raw nav2 costmaps -> the bordered, pitched device maps, and the stream over a padded map that K3 and
// K7's fill (rolling_window.h) share.  Part of libneo_mpc.so's device code (included by neo_mpc_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "neo_mpc_device.h"

namespace neo_mpc {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));   // a 16-byte chunk of a padded map

// The stream over map blockIdx.y of a.dst (a.rows rows of a.pitch bytes, a.dst_stride apart): one 16-byte store per lane and
// chunk, `chunk(my, mx0)` the sixteen bytes from column mx0 of the map's row my on -- lethal in the border and the pitch
// padding --, kUnroll chunks per thread with every load issued before the first store (memory-level parallelism: the kernels
// are pure streams).  `threads`: blockDim.x, read in the kernel -- only there does the compiler fold it to the launch's size.
template <int kUnroll, class Args, class Chunk>
__device__ __forceinline__ void stream_padded_map(const Args& a, unsigned threads, Chunk&& chunk) {
  u32x4* dst = reinterpret_cast<u32x4*>(a.dst + (int64_t)blockIdx.y * a.dst_stride);
  const unsigned chunks_per_row = (unsigned)a.pitch >> 4;
  const unsigned total = (unsigned)a.rows * chunks_per_row;   // (< 2^31: PaddedMap::check on the host)
  const unsigned stride = gridDim.x * threads;
  for (unsigned base = blockIdx.x * threads + threadIdx.x; base < total; base += kUnroll * stride) {
    u32x4 v[kUnroll];
#pragma unroll
    for (int k = 0; k < kUnroll; ++k)
      if (base + k * stride < total) {
        const int row = (int)((base + k * stride) / chunks_per_row);
        v[k] = chunk(row - a.border, (int)(base + k * stride - (unsigned)row * chunks_per_row) * 16 - a.border);
      }
    // streamed once, read back sparsely (reach tiles): non-temporal, so the stream does not wait for
    // L2 lines to be allocated (measured: 3.0 -> 4.3 TB/s over a pool of 4096 windows)
#pragma unroll
    for (int k = 0; k < kUnroll; ++k)
      if (base + k * stride < total) __builtin_nontemporal_store(v[k], dst + (base + k * stride));
  }
}
// ... and its grid of 256-thread workgroups: `unroll` chunks per thread (one-chunk threads make the launch dispatch-bound for
// pools of small maps), at most 2048 workgroups per map
inline dim3 padded_map_grid(int rows, int pitch, int unroll, unsigned maps) {
  const long total = (long)rows * (pitch >> 4);
  const long blocks = (total + 256L * unroll - 1) / (256L * unroll);
  return dim3((unsigned)(blocks > 2048 ? 2048 : blocks), maps);
}

// K3: raw nav2 costmap -> bordered, pitched device map
constexpr int kIngestUnroll = 4;
__device__ __forceinline__ u32x4 ingest_chunk(const IngestArgs& a, int my, int mx0) {
  u32x4 v = {0xFEFEFEFEu, 0xFEFEFEFEu, 0xFEFEFEFEu, 0xFEFEFEFEu};
  if (my >= 0 && my < a.size_y && mx0 >= 0 && mx0 + 16 <= a.size_x && (a.size_x & 7) == 0) {
    // interior chunk of a map whose rows are 8-byte aligned (mx0 is a multiple of 16): two 8-byte loads
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    const u32x2* src8 = reinterpret_cast<const u32x2*>(a.src + (long)my * a.size_x + mx0);
    const u32x2 lo = __builtin_nontemporal_load(src8), hi = __builtin_nontemporal_load(src8 + 1);
    v = u32x4{lo.x, lo.y, hi.x, hi.y};
  } else if (my >= 0 && my < a.size_y && mx0 >= 0 && mx0 + 16 <= a.size_x && (a.size_x & 3) == 0) {
    const uint32_t* src4 = reinterpret_cast<const uint32_t*>(a.src + (long)my * a.size_x + mx0);
    v = u32x4{src4[0], src4[1], src4[2], src4[3]};
  } else if (my >= 0 && my < a.size_y && mx0 >= 0 && mx0 < a.size_x && (a.size_x & 3) == 0) {
    // the chunk that straddles the right edge of a map whose width is a multiple of 4 (200-cell windows: 8 of its 16
    // bytes): whole dwords, lethal beyond the edge
    const uint32_t* src4 = reinterpret_cast<const uint32_t*>(a.src + (long)my * a.size_x + mx0);
    const int valid = (a.size_x - mx0) >> 2;   // 1..3 dwords
    v = u32x4{src4[0], valid > 1 ? src4[1] : 0xFEFEFEFEu, valid > 2 ? src4[2] : 0xFEFEFEFEu, 0xFEFEFEFEu};
  } else if (my >= 0 && my < a.size_y && mx0 + 16 > 0 && mx0 < a.size_x) {
    uint8_t bytes[16];
    const uint8_t* src = a.src + (long)my * a.size_x;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int mx = mx0 + k;
      bytes[k] = (mx >= 0 && mx < a.size_x) ? src[mx] : (uint8_t)254;
    }
    v = *reinterpret_cast<const u32x4*>(bytes);
  }
  return v;
}
__global__ __launch_bounds__(256) void k_ingest(const IngestArgs args) {
  IngestArgs a = args;   // blockIdx.y: which map of a pool
  a.src += (long)blockIdx.y * a.size_x * a.size_y;
  stream_padded_map<kIngestUnroll>(a, blockDim.x, [&](int my, int mx0) { return ingest_chunk(a, my, mx0); });
}

}  // namespace
}  // namespace neo_mpc
