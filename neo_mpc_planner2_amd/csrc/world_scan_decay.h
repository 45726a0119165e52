// world_scan_decay.h -- K14: old marks of the fleet's shared obstacle layer expire, step 2b of the contract of
// neo_mpc_update_world_scan_layer (include/neo_mpc.h, neo_mpc_set_world_scan_decay): a mark that no scan update has made again
// for max_age scan updates becomes unknown_value in the layer itself.  Enqueued only while decay is on: the tick in front of
// the marking launch, the stamped marking launch in place of K12a's, the sweep between the marks and K12's footprints, and --
// on the first update behind switching it on -- the fill in front of them all.  Part of libneo_mpc.so's device code (included
// by neo_mpc_kernels.hip).
//
// `stamp`, a uint32_t per world cell, row-major like the layer: the value of `clock` when the cell was last marked, read only
// under a cell that is 254.  `clock`, one uint32_t: the scan updates so far.  It lives in device memory and is advanced by
// device code, so that a captured update that is replayed advances it; every difference is an unsigned 32-bit subtraction.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "neo_mpc_device.h"
#include "scan_layer.h"

namespace neo_mpc {
namespace {

constexpr int kDecayThreads = 256;
constexpr int kDecayCells = 16;     // cells a lane of the sweep owns: one aligned 16-byte load of the layer

// K14a: a scan update begins.  One lane, a plain read-modify-write: the launch boundary puts it behind everything that read the
// clock before and in front of everything that reads it in this update.
__global__ __launch_bounds__(kLanes) void k_world_scan_tick(const WorldScanArgs a) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *a.clock = *a.clock + 1u;
}

// K14b, the first update with decay on: every cell's stamp becomes the clock as it stands -- a mark that is in the layer counts
// as made by the last scan update before this one.  Four stamps per lane and store; the last cells % 4 one by one.
__global__ __launch_bounds__(kDecayThreads) void k_world_scan_stamp_fill(const WorldScanArgs a) {
  const uint32_t now = *a.clock;
  const int64_t cells = (int64_t)a.wsx * a.wsy, quads = cells >> 2;
  const int64_t t = (int64_t)blockIdx.x * kDecayThreads + threadIdx.x;
  // 4 t + 3 < cells: inside `stamp`, whose base is the allocator's, 16-byte aligned
  if (t < quads) reinterpret_cast<uint4*>(a.stamp)[t] = make_uint4(now, now, now, now);
  else if (t < quads + (cells & 3)) a.stamp[(quads << 2) + (t - quads)] = now;   // quads * 4 <= index < cells
}

// K14c, step 2 of the contract with decay on: K12a's marking launch, and stamp[cell] = clock wherever it writes 254.  The tick
// lies a launch in front: every lane reads the advanced clock, so every writer of a stamp of this launch writes the same
// value, as every writer of a layer byte does -- K10b's argument, for both arrays.  (The world's rows are wsx cells apart in
// the layer and in `stamp` alike.)
__global__ __launch_bounds__(kScanRayThreads) void k_world_scan_marks_stamped(const WorldScanArgs a) {
  scan_ray<true, true>(a.s, blockIdx.y, blockIdx.x * kScanRayThreads + threadIdx.x, a.wox, a.woy, a.wres, a.wsx, a.wsy, a.wsx, a.layer,
                       a.stamp, *a.clock);
}

// bytes of the word equal to 254 -> their top bits (exact for "any": a false positive needs a true one below it)
__device__ __forceinline__ uint32_t decay_marks_in(uint32_t word) {
  const uint32_t x = word ^ 0xFEFEFEFEu;
  return (x - 0x01010101u) & ~x & 0x80808080u;
}

// K14d, step 2b of the contract: a flat sweep over the wsx * wsy bytes of the layer, kDecayCells cells per lane by one aligned
// 16-byte load (the layer's base is the allocator's), the last cells % 16 a byte per lane.  A lane whose cells hold no mark
// is done after that load; stamps are fetched only under marks, and a byte is stored only into a cell that expired.  Each
// cell is read and written by the one lane that owns it: no atomics, no barrier, no wave operation.
__global__ __launch_bounds__(kDecayThreads) void k_world_scan_decay(const WorldScanArgs a) {
  const int64_t cells = (int64_t)a.wsx * a.wsy, groups = cells / kDecayCells;
  const int64_t t = (int64_t)blockIdx.x * kDecayThreads + threadIdx.x;
  const uint32_t now = *a.clock, age = a.max_age;
  const uint8_t gone = (uint8_t)a.s.unknown;
  if (t < groups) {
    const int64_t at = t * kDecayCells;               // at + 15 < cells: inside the layer and `stamp`
    const uint4 q = *reinterpret_cast<const uint4*>(a.layer + at);
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
    if ((decay_marks_in(w[0]) | decay_marks_in(w[1]) | decay_marks_in(w[2]) | decay_marks_in(w[3])) == 0u) return;
#pragma unroll
    for (int b = 0; b < kDecayCells; ++b) {
      if (((w[b >> 2] >> (8 * (b & 3))) & 0xFFu) != 254u) continue;
      if (now - a.stamp[at + b] >= age) a.layer[at + b] = gone;
    }
    return;
  }
  const int64_t at = groups * kDecayCells + (t - groups);
  if (at < cells && a.layer[at] == 254 && now - a.stamp[at] >= age) a.layer[at] = gone;   // the tail: at < cells
}

}  // namespace
}  // namespace neo_mpc
