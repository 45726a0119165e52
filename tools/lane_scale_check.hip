// the lane step multipliers the old way (lane_scale, computed lane by lane on the device) against the compile-time tables
// (kLaneScales, csrc/feasible_set.h) the tame three-stage stage-wise kernels fetch theirs from: byte for byte, on the GPU
// build+run: hipcc --offload-arch=gfx950 -O3 -std=c++17 -Ineo_mpc_planner2_amd/csrc -Iinclude tools/lane_scale_check.hip -o /tmp/lane_scale_check && /tmp/lane_scale_check
// (tests/test_constant_sources_gpu.py runs it; exit status 0: all 128 pairs equal)
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "feasible_set.h"

using namespace neo_mpc;

// out[0..63] lane_scale<true>, [64..127] lane_scale<false>, [128..191] kLaneScales<true>, [192..255] kLaneScales<false>
__global__ void k_lane_scales(double* out) {
  const int lane = threadIdx.x;
  out[lane] = lane_scale<true>(lane);
  out[64 + lane] = lane_scale<false>(lane);
  out[128 + lane] = kLaneScales<true>.v[lane];
  out[192 + lane] = kLaneScales<false>.v[lane];
}

#define CHECK(call)                                                                  \
  do {                                                                               \
    hipError_t e_ = (call);                                                          \
    if (e_ != hipSuccess) { printf("%s: %s\n", #call, hipGetErrorString(e_)); return 2; } \
  } while (0)

int main() {
  double* d = nullptr;
  double h[256];
  CHECK(hipMalloc(&d, sizeof(h)));
  CHECK(hipMemset(d, 0xff, sizeof(h)));
  k_lane_scales<<<1, 64>>>(d);
  CHECK(hipGetLastError());
  CHECK(hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost));
  CHECK(hipFree(d));
  static constexpr LaneScaleTable host_long = make_lane_scale_table<true>(), host_plain = make_lane_scale_table<false>();
  int bad = 0;
  for (int k = 0; k < 2; ++k) {
    for (int lane = 0; lane < 64; ++lane) {
      uint64_t old_w, new_w, host_w;
      memcpy(&old_w, &h[64 * k + lane], 8);
      memcpy(&new_w, &h[128 + 64 * k + lane], 8);
      memcpy(&host_w, k == 0 ? &host_long.v[lane] : &host_plain.v[lane], 8);
      if (old_w != new_w || new_w != host_w) {
        printf("lane_scale<%s>(%d): computed %016llx, device table %016llx, host table %016llx\n", k == 0 ? "true" : "false", lane,
               (unsigned long long)old_w, (unsigned long long)new_w, (unsigned long long)host_w);
        ++bad;
      }
    }
  }
  printf("lane multipliers: %d of 128 pairs differ\n", bad);
  return bad ? 1 : 0;
}
