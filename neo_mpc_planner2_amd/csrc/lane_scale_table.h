// lane_scale_table.h -- the 64 candidate step multipliers of one iteration as compile-time tables
// Plain C++ (no HIP): feasible_set.h includes it for the device code, tests/test_lane_scale_table.py compiles it for the host.
#pragma once

namespace neo_mpc {

// candidate step multipliers: lanes 0..31 scale the proximal-gradient step by 2^(-12 + l/2),
// lanes 32..63 are step lengths along the L-BFGS direction
#define NEO_QN_STEPS                                                                                  \
  1.0, 0.84, 1.19, 0.71, 1.41, 0.59, 1.68, 0.5, 2.0, 0.42, 2.38, 0.35, 2.83, 0.25, 4.0, 0.177,         \
  0.125, 0.088, 0.0625, 0.044, 0.03125, 0.0156, 0.0078, 0.0039, 0.00195, 0.00098, 4.9e-4, 2.4e-4,    \
  1.2e-4, 6e-5, 3e-5, 1.5e-5

// What lane_scale<kLongShots>(lane) (feasible_set.h) returns, lane by lane, bit for bit: a power of two is exact, and the one
// float64 product of the odd proximal lanes rounds at compile time as v_mul_f64 rounds it (IEEE, to nearest even).
struct LaneScaleTable { double v[64]; };
constexpr double lane_scale_pow2(int e) {
  double r = 1.0;
  for (; e > 0; --e) r *= 2.0;
  for (; e < 0; ++e) r *= 0.5;
  return r;
}
template <bool kLongShots>
constexpr LaneScaleTable make_lane_scale_table() {
  constexpr double steps[32] = {NEO_QN_STEPS};
  LaneScaleTable t{};
  for (int lane = 0; lane < 64; ++lane) {
    if (kLongShots && lane >= 61) t.v[lane] = lane_scale_pow2(lane - 58);
    else if (lane >= 32) t.v[lane] = steps[lane - 32];
    else {
      const double s = lane_scale_pow2(-12 + (lane >> 1));
      t.v[lane] = (lane & 1) ? s * 1.4142135623730951 : s;
    }
  }
  return t;
}

}  // namespace neo_mpc
