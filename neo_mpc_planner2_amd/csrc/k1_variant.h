// k1_variant.h -- what one variant of K1 is: K1Variant, the record of a kernel's template parameters and of every constant
// derived from them, each exactly once; and the helpers by which a phase of K1 gets its operands afresh (fresh_args,
// own_loop_params, ctx_from_lds, lane_again).  The kernels (k1_solve.h) build the record from their own parameters; the
// phase functions (k1_solve.h) take it as `template <class V>`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "neo_mpc_device.h"
#include "wave_ops.h"
#include "solver_context.h"
#include "tangent_cone.h"

namespace neo_mpc {
namespace {

// (the stop rules and their constants: solver_rules.h, shared with the host side and with the CPU mirror)
// largest control_steps the run-time-sized Newton kernel takes (a 24 x 24 system: rows in registers)
constexpr int kNewtonMaxSteps = 8;

// kRouted: the stage-wise branch of the routed control_steps-3 kernel (k_solve_routed).  Its LDS carve-up is the stage-wise
// one for three stages laid INSIDE the dense kernel's (records, tolerance block, term table, iterate and gradients sit at the
// same offsets in both; the reach tile stays where the set-up staged it), control_steps is the constant 3 -- the run-time-sized
// code below folds to three stages -- and the prox-only zone around the kink is the stage-wise direction's.
constexpr int kRoutedSteps = 3;
constexpr LdsLayout make_routed_stagewise_layout() {
  LdsLayout l = make_lds_layout(kRoutedSteps, 0, true, true);
  constexpr LdsLayout dense = make_lds_layout(kRoutedSteps, 4, false);
  l.tile = dense.tile;
  l.total_bytes = dense.total_bytes;
  return l;
}
static_assert(make_lds_layout(kRoutedSteps, 0, true, true).tile <= make_lds_layout(kRoutedSteps, 4, false).tile,
              "the stage-wise arrays of three stages fit in front of the dense kernel's reach tile");
static_assert(make_lds_layout(kRoutedSteps, 0, true, true).gr == make_lds_layout(kRoutedSteps, 4, false).gr,
              "records, iterate and gradients share their offsets");
// The tame routed stage-wise search keeps its 64 lane step multipliers (feasible_set.h kLaneScales) in LDS, one double per
// lane, written once at the search's entry: behind the last stage-wise array and in front of the reach tile -- room the
// dense carve-up leaves and no stage-wise phase, cell scan included, addresses (every other offset of the routed layout lies
// below it).  The kernel's LDS size does not change.
constexpr int kRoutedLaneScales = make_lds_layout(kRoutedSteps, 0, true, true).tile;
static_assert(kRoutedLaneScales + kLanes <= make_lds_layout(kRoutedSteps, 4, false).tile,
              "the lane multipliers fit between the stage-wise arrays and the reach tile");

// ---------------------------------------------------------------- K1: template parameters of the phase functions and the kernels
// kSteps > 0: specialisation for control_steps == kSteps -- every lane keeps its candidate's controls and sin/cos in
// registers, so the winner is stored without being recomputed and the next adjoint sweep needs no trigonometry.
// kSteps == 0: any control_steps (LDS-only path).
// kDir: search direction of lanes 32-63 -- 0 projected L-BFGS, 1 projected Newton with the dense system: control_steps ==
// kSteps, or with kSteps == 0 any control_steps <= kNewtonMaxSteps (measured against L-BFGS on the 1000^2 map, 65 536
// instances: +28 % at control_steps 1, +54 % at 2, +50 % at 4, +38 % at 5-7, +42 % at 8), 2 projected Newton solved stage by
// stage (riccati.h; kSteps == 0 only, any control_steps).
// kTame: instantiation for parameter sets (the README's among them) whose max_vel_trans disc lies inside the vx/vy box --
// the box/disc corner cases of the projection and of the tangent cone drop out -- and whose heading cannot leave
// [-pi/4, pi/4] within the horizon -- no range reduction in the rollout's sin/cos.
// kStaticTile > 0: LDS is a static array sized for the compile-time layout plus a reach
// tile of at most kStaticTile bytes -- every LDS address is then an instruction immediate instead of a
// "dynamic LDS base + offset" value that lives in (and gets spilled from) a scalar register.
// kRouted: the stage-wise branch of k_solve_routed (above).  kMinWavesPerSimd: the occupancy a variant is built for.
template <int kMinWavesPerSimd_, int kSteps_, int kDir_, bool kTame_, int kStaticTile_, bool kRouted_ = false>
struct K1Variant {
  static constexpr int kMinWavesPerSimd = kMinWavesPerSimd_, kSteps = kSteps_, kDir = kDir_, kStaticTile = kStaticTile_;
  static constexpr bool kTame = kTame_, kRouted = kRouted_;
  // ---- the LDS carve-up
  // (the run-time-sized Newton kernel carves LDS for its largest system and no L-BFGS pairs)
  static constexpr int kLayoutSteps = kSteps ? kSteps : kNewtonMaxSteps;
  // compile-time LDS offsets (lbfgs_memory is 4 in the specialisations' layout)
  static constexpr bool kStaticOffsets = kSteps || kStaticTile;
  static constexpr LdsLayout kStaticLayout = make_lds_layout(kLayoutSteps, kSteps ? 4 : 0, false);
  // what a phase of this variant addresses LDS by, wherever the offsets are compile-time ones (fresh_args)
  // (kRouted implies kSteps == kRoutedSteps -- the static_assert below -- and fresh_args relies on it: it sets the
  // stage count from kSteps for the routed branch too)
  static constexpr LdsLayout kLayout = kRouted ? make_routed_stagewise_layout() : kStaticLayout;
  // the static array of the kStaticTile kernels, in doubles (two, never addressed, where LDS is dynamic)
  static constexpr int kStaticDoubles = kStaticTile ? (kStaticLayout.total_bytes + kStaticTile) / 8 : 2;
  static constexpr bool kCovered = kStaticTile > 0;   // the reach tile is there and covers every lookup (costmap.h cell_raw)
  // ---- the direction
  static constexpr bool kNewton = kDir == 1;    // dense system in registers
  static constexpr bool kRiccati = kDir == 2;   // stage-wise recursion
  static constexpr bool kSecond = kDir != 0;    // either: Newton stop rules, no quasi-Newton state
  // the control_steps-3 stop rules of the dense direction -- the window rule on every run of three iterations, the blocked-run
  // rule, closing-in behind two blocked iterations -- also end the stage-wise searches of the routed kernel: what ends a search
  // depends on the horizon, not on how the direction was computed (solver_rules.h neo_rules_derive_routed)
  static constexpr bool kBlockedRule = kNewton || kRouted;
  static_assert(!kRiccati || kSteps == 0 || kRouted, "the stage-wise direction: run-time-sized, or the routed kernel's control_steps-3 branch");
  static_assert(!kRouted || (kRiccati && kSteps == kRoutedSteps), "the routed branch is the stage-wise one, three stages in registers");
  // (kSteps > 0 with the stage-wise direction -- the routed branch: candidates in registers, unrolled rollouts, the winner
  // stored without being recomputed like the dense specialisation; gradient and sweep run lane = stage on three lanes)
  static constexpr int kFew = (kRiccati && kSteps > 0) ? kSteps : 0;
  // three stages: the sweep hands each lane its own stage's step in registers, riccati_finish writes d once and hands the
  // step test its maximum (riccati.h SweepHandOff)
  static constexpr bool kHandOff = kFew > 0;
  // three TAME stages -- kernels that never sweep twice with another active set -- switch five things (four of them were
  // flags of their own with this one expression, the fifth had it spelled out at its use):
  //   the scalar case   each stage's case is known as a scalar before the sweep starts (solve_search's direction phase,
  //                     riccati_sweep);
  //   the kept gains    sweeping once per iteration, the sweep keeps its gains in registers from its backward to its
  //                     forward half (riccati_sweep);
  //   the stage carry   lane = stage fetches what the tangent-cone pass reads of its block at the END of the adjoint pass
  //                     (adjoint.h StageCarry);
  //   the accept fetch  the rule book's tolerance words come through the kernel-argument pointer (solve_search, "does this
  //                     iteration end the search");
  //   the preload       a candidate's block fetches all it reads from LDS in one go (feasible_set.h candidate_block).
  static constexpr bool kFewTame = kFew > 0 && kTame;
  // Newton: control_steps == kSteps, or (kSteps == 0) any control_steps <= kNewtonMaxSteps -- the
  // system's arrays are sized for the bound and every loop over them is guarded by the run-time size
  static constexpr int kNwSteps = !kNewton ? 1 : kSteps ? kSteps : kNewtonMaxSteps;
  static constexpr int kVars = 3 * kNwSteps;  // compile-time bound of the Newton system (= its size when kSteps > 0)
  // Newton: one float32 record per control block (projector + block curvature), written by the
  // tangent-cone pass; it lives in the cs..rt step arrays, which the Newton kernel does not use
  static_assert(2 * 7 >= kNewtonRecord, "Newton records do not fit the step arrays");
  // the four constants the costmap lookup of every stage of every candidate needs (world position = X0 + Rot(psi0) (x, y))
  // stay in VECTOR registers (every lane holds the same value).  The scalar file is over-subscribed -- a hundred
  // scalars are spilled to vector lanes -- and each use of a spilled pair costs two v_readlane and a wait state: twelve
  // lane reads per stage.  (Round 4: the three-address polynomial kernels freed nine vector registers.)
  // (the general kernels have no vector register to spare at four waves per SIMD: scalar there, as before)
  static constexpr bool kVectorPose = kTame;
  static constexpr int kRegSteps = kSteps ? kSteps : 1;
  static constexpr int kPairs = kSteps ? 4 : NEO_MPC_MAX_LBFGS_MEMORY;  // specialisations: lbfgs_memory <= 4
};

// ---------------------------------------------------------------- K1: phases
// K1 runs in phases -- set-up, search, cell scan, K2 -- and the search can be taken up again behind the scan.  Each phase
// starts from a FRESH copy of the launch arguments (re-read from the kernarg segment through a pointer the compiler cannot
// see through) and of the per-instance constants (re-read from the tolerance block of LDS, where the set-up leaves them): the
// vector-register residents of the solver loop are then dead outside it.  Allocated as ONE live range across the scan they
// came out spilled -- and reloaded from scratch inside the loop, +20 % on a C2 launch for code that runs once per solve.
template <class V>
__device__ __forceinline__ void fresh_args(SolveArgs& a) {
  auto kp = (const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr();   // (k_solve's only argument: offset 0)
  asm volatile("" : "+s"(kp));
  a = *(const SolveArgs*)kp;
  if (V::kRouted || V::kStaticOffsets) {
    constexpr LdsLayout kLayout = V::kLayout;
    const int tile_w = a.lds.tile_w, tile_h = a.lds.tile_h, reach = a.lds.reach;
    a.lds = kLayout;
    a.lds.tile_w = tile_w; a.lds.tile_h = tile_h; a.lds.reach = reach;
    if (V::kSteps) a.p.n = V::kSteps;
  }
}
// The parameters the solver loop reads are detached from the wide scalar loads that bring the
// kernel arguments in: a spilled s_load_dwordx16 tuple comes back whole (16 v_readlane) for every
// use of one of its members; as values of their own they are reloaded pair by pair.
__device__ __forceinline__ void own_loop_params(SolveArgs& a) {
  auto own = [](double& v) { asm volatile("" : "+s"(v)); };
  own(a.p.dt); own(a.p.wt_n); own(a.p.wo_n); own(a.p.wc_n); own(a.p.wterm_o); own(a.p.r);
  own(a.p.lo[2]); own(a.p.hi[2]);
  own(a.map.origin_x); own(a.map.origin_y); own(a.map.resolution); own(a.map.inv_resolution);
}
// the per-instance constants as the set-up left them in LDS (request record + tolerance block); wave-uniform: scalar
// registers -- except, kVectorPose, the four the costmap lookup of every stage of every candidate needs (K1Variant says why)
template <bool kVectorPose>
__device__ __forceinline__ void ctx_from_lds(const SolveArgs& a, const double* L, Ctx& c) {
  const double* P = L + a.lds.prob;
  const double* t = L + a.lds.tol;
  c.cx = lane_value(P[P_CARROT_X], 0); c.cy = lane_value(P[P_CARROT_Y], 0);
  c.tyaw = lane_value(t[T_TYAW], 0); c.fyaw = lane_value(t[T_FYAW], 0);
  c.v0 = lane_value(P[P_VEL], 0); c.v1 = lane_value(P[P_VEL + 1], 0); c.v2 = lane_value(P[P_VEL + 2], 0);
  c.c0 = t[T_C0]; c.s0 = t[T_S0]; c.X0 = P[P_CUR_X]; c.Y0 = P[P_CUR_Y];
  if (kVectorPose) asm volatile("" : "+v"(c.c0), "+v"(c.s0), "+v"(c.X0), "+v"(c.Y0));
  else { c.c0 = lane_value(c.c0, 0); c.s0 = lane_value(c.s0, 0); c.X0 = lane_value(c.X0, 0); c.Y0 = lane_value(c.Y0, 0); }
  const int* ti = reinterpret_cast<const int*>(t + T_TILE);
  c.tile_x0 = uniform_int(ti[0]); c.tile_y0 = uniform_int(ti[1]); c.tile_geom = uniform_int(ti[2]);
  c.konst = 0.0; c.true_yaw = 0.0;   // (inside the search f excludes the constant terms; K2 reads both from the block)
}
// (the lane index is not kept in a register across the loop -- the stage-wise kernels at four waves per SIMD parked it in
// scratch and reloaded it at the top of every iteration: it is re-derived from the hardware's lane mask count, seeded
// with an opaque zero so that the compiler cannot hoist it either)
__device__ __forceinline__ int lane_again() {
  int zero;
  asm volatile("v_mov_b32 %0, 0" : "=v"(zero));
  return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, (unsigned)zero));
}

}  // namespace
}  // namespace neo_mpc
