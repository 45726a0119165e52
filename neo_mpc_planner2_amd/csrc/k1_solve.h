// k1_solve.h -- K1 of the batched MPC solver, gfx950 (CDNA4 / MI355X): k_solve, k_solve_routed, the outline of their
// phases and the helper that launches them.  Part of libneo_mpc.so's device code; each of the two units that include it holds
// the variants it launches: neo_mpc_kernels.hip the dense-Newton and L-BFGS ones, neo_mpc_riccati.hip the rest.
//
//   K1 k_solve        one 64-lane wavefront per instance.  Per iteration the wave
//                     evaluates 64 candidate control sequences at once (one rollout per
//                     lane): lanes 0-31 walk the projected proximal-gradient arc at 32
//                     step sizes, lanes 32-63 a projected second-order direction at 32 step
//                     lengths -- dense Newton at control_steps 3 (finite-difference Hessian of the
//                     analytic gradient, one column per lane, solved in registers; the headline
//                     specialisation), the stage-wise (Riccati) Gauss-Newton sweep of riccati.h at
//                     every other control_steps (rollout/adjoint as DPP prefix scans, lane = stage;
//                     damped beyond 8 steps; wall model for costmap steps; in free space the full
//                     step is tried alone before the search), projected L-BFGS on request; the lowest
//                     objective wins (wave arg-min).  Iterates, gradients and the direction's
//                     state live in LDS; the (2R+1)^2 costmap reach tile is staged into LDS
//                     once per solve with coalesced dword loads.  float64 throughout (the arc
//                     search compares objective values, which resolves the minimiser to
//                     sqrt(eps); MI355X has full-rate vector f64); the Newton systems themselves
//                     are float32 (they only yield a direction).
// No MFMA: a 3*control_steps-variable problem has no dense contraction.
//
// Where what is:
//   k1_variant.h   K1Variant<...>: a kernel's template parameters and every constant derived from them, once; fresh_args
//                  and the other helpers by which a phase gets its operands afresh.
//   dense_newton.h the dense direction: its gradient pass (NEO_DENSE_NEWTON_HESSIAN_PASS, expanded in solve_search) and its system.
//   this file      solve_setup, solve_search, solve_finish, the search's LDS pointers (search_lds), what the kernels start
//                  with (NEO_K1_PROLOGUE: solve_lds, solve_instance), the kernels, and the preamble the two dispatch
//                  tables share (K1Launch).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "neo_mpc_device.h"
#include "wave_ops.h"
#include "fast_math.h"
#include "solver_context.h"
#include "solver_rules.h"
#include "costmap.h"
#include "feasible_set.h"
#include "rollout.h"
#include "riccati.h"
#include "adjoint.h"
#include "tangent_cone.h"
#include "dense_newton.h"
#include "lbfgs.h"
#include "cell_scan.h"
#include "k1_variant.h"
#include "k1_timing.h"

namespace neo_mpc {
namespace {

// What the phases hand to one another in registers (everything else goes through LDS).
struct SolveCarry {
  int flags;                 // NEO_MPC_FLAG_RESET (set-up -> K2)
  bool cold;                 // x0 == 0 (wave-uniform: every lane scans the same LDS values)
  bool wall_in_reach;        // a lethal cell in the reach tile (set-up -> the routed kernel's branch)
  double f = INFINITY;       // objective at u; f(x0) comes out of the first candidate pass: lane 0 evaluates x0 itself there
  int it = 0, nfev = 1, status = NEO_MPC_STATUS_MAX_ITER;
};

// ---- phase 0: set-up.  Records, reset, footprint, reach tile; the per-instance constants and the stop tolerances go to
//      the tolerance block of LDS (layout: solver_context.h), where every later phase reads them; x0.
//      Returns false when the instance makes no request this tick (nothing more to do).
template <class V>
__device__ __forceinline__ bool solve_setup(double* L, uint32_t b, int lane, SolveCarry& s) {
  constexpr int kSteps = V::kSteps;
  constexpr bool kTame = V::kTame;
  int flags;
  bool cold = true;
  {
    SolveArgs a;
    fresh_args<V>(a);
    const DevParams& p = a.p;
    const int n = kSteps ? kSteps : p.n, nv = 3 * n;
    load_records(a, L, b, lane);
    // no request for this robot this tick (the plugin threw before its service call, cpp:234-236; K4 status 3): the node's
    // state does not advance: state record and warm start keep their bytes, the outputs say "skipped" (rollout.h)
    if (uniform_int(reinterpret_cast<const int*>(L + a.lds.prob)[PI_SKIP]) == 1) { skip_instance(a, b, lane); return false; }
    select_map(a.map, L + a.lds.prob);
    flags = reset_and_warm(a, L, b, lane) ? NEO_MPC_FLAG_RESET : 0;
    // (the footprint cost -- the request's own, or the raster's -- waits for K2 in the request record's slot in LDS: as a
    // register it was live across the whole kernel and, at four waves per SIMD, spilled to scratch: the only scratch of the
    // headline kernel, 1.5 KB of memory traffic per solve against 885 B of algorithmic bytes)
    const double fcost = footprint_cost(a, L, b, lane);
    if (lane == 0) L[a.lds.prob + P_FOOTPRINT] = fcost;
    Ctx c;
    make_ctx_wave(p, a.map, L + a.lds.prob, fcost, c, lane);
    load_tile(a, c, L, lane);
    s.wall_in_reach = (c.tile_geom & kTileWall) != 0;
    if (s.wall_in_reach) flags |= NEO_MPC_FLAG_WALL_IN_REACH;
    // The stop tolerances are read once per iteration: from LDS, so that they do not sit in (and get
    // spilled from) scalar registers all through the loop.
    // So do two per-instance constants the loop has no use for: the request's true yaw (K2 only) and
    // the part of the objective that does not depend on u -- inside the loop f excludes it.
    if (lane == 0) {
      double* t = L + a.lds.tol;
      t[T_XTOL] = p.xtol; t[T_EARLY] = p.early_tol; t[T_FINAL] = p.final_tol; t[T_FTOL] = p.ftol;
      t[T_STALL] = p.stall_step; t[T_WTOL] = p.wtol; t[T_WTOL_LATE] = p.wtol_late; t[T_KINK] = p.kink_radius;
      t[T_KONST] = c.konst; t[T_TRUE_YAW] = c.true_yaw;
      t[T_HOP_DROP] = p.hop_min_drop; t[T_HOP_RANGE] = p.hop_range;
      t[T_BTOL_MAP] = p.btol_map; t[T_BTOL_FREE] = p.btol_free;
      reinterpret_cast<int*>(t + T_HOP_STAGE)[kHopLanes] = 0;   // no hop candidates yet
      t[T_C0] = c.c0; t[T_S0] = c.s0; t[T_TYAW] = c.tyaw; t[T_FYAW] = c.fyaw;
      int* ti = reinterpret_cast<int*>(t + T_TILE);
      ti[0] = c.tile_x0; ti[1] = c.tile_y0; ti[2] = c.tile_geom;
    }
    double* u = L + a.lds.u;
    // x0 clipped to the feasible set (SciPy clips x0 to the bounds, _slsqp_py.py:268)
    for (int i = lane; i < n; i += kLanes) project_block<kTame>(p, u[3 * i], u[3 * i + 1], u[3 * i + 2]);
    WAVE_SYNC();
    for (int k = 0; k < nv; ++k) cold = cold && (u[k] == 0.0);
    ctx_from_lds<false>(a, L, c);
    // The warm start is the previous solution shifted by a WHOLE control step (py:198-202: block i <- block i + 1, the
    // FILTERED first control last, py:366-367) although only one control interval -- an eighth of a step at 30 Hz and the
    // README's horizon -- has passed: the previous solution itself, i.e. the shift undone with the first block as the solver
    // left it (kept in the state record by K2: S_PREV_U0; the filtered one where a caller's record does not carry it), is
    // usually much closer to this tick's minimiser -- and IS the minimiser for a robot the collision latch has stopped.
    // In free space (no costmap term under either rollout: one basin) the search starts from whichever of the two has the
    // lower objective (lane 0 rolls out the warm start, lane 1 the un-shifted one).  On the costmap it starts where the
    // reference starts, and the un-shifted point, when it has the lower objective, is ONE CANDIDATE of the first iteration
    // (lane kAltLane, competing by objective value like every other lane: it wins where the problem has not changed, and loses
    // to the first step from the reference's start where that leads into another basin -- starting from it outright ended one
    // recorded call of the reference 1.9e-3 above it).  The warm start handed BACK is the reference's shift as ever (K2).
    // Closed loop of 4096 robots (CPU mirror): 6.2 -> 4.45 -> 3.6 iterations per warm tick, per-tick maximum 13 -> 10.
    {
      double* S = L + a.lds.state;
      int* Si = reinterpret_cast<int*>(S);
      const bool has_prev = uniform_int(Si[SI_HAS_PREV]) == 1 && !(flags & NEO_MPC_FLAG_RESET);
      WAVE_SYNC();
      if (lane == 0) {
        double q0 = has_prev ? S[S_PREV_U0] : u[nv - 3], q1 = has_prev ? S[S_PREV_U0 + 1] : u[nv - 2], q2 = has_prev ? S[S_PREV_U0 + 2] : u[nv - 1];
        project_block<kTame>(p, q0, q1, q2);
        S[S_PREV_U0] = q0; S[S_PREV_U0 + 1] = q1; S[S_PREV_U0 + 2] = q2;
        Si[SI_HAS_PREV] = 0;
      }
      WAVE_SYNC();
    }
    if (!cold && n > 1 && !(p.compat & kCompatNoUnshift) && p.max_it < kDumpGradient) {   // (not in the test hooks: they dump AT the given point)
      const double* A0 = L + a.lds.state + S_PREV_U0;
      double ts = 0.0;
      const double fs = rollout_cost<kSteps, kTame, V::kCovered>(
          a, c, L,
          [&](int i, double& b0, double& b1, double& b2) {
            const double* src = lane == 1 ? (i == 0 ? A0 : u + 3 * (i - 1)) : u + 3 * i;
            b0 = src[0]; b1 = src[1]; b2 = src[2];
          },
          NoRecord(), &ts);
      const double f_warm = lane_value(fs, 0), f_alt = lane_value(fs, 1);
      const bool free_both = lane_value(ts, 0) == 0.0 && lane_value(ts, 1) == 0.0;
      if (f_alt < f_warm && free_both) {
        double v0 = 0.0, v1 = 0.0, v2 = 0.0;   // (nv <= 192: up to three elements per lane)
        const int k0 = lane, k1 = lane + kLanes, k2 = lane + 2 * kLanes;
        if (k0 < nv) v0 = k0 >= 3 ? u[k0 - 3] : A0[k0];
        if (k1 < nv) v1 = u[k1 - 3];
        if (k2 < nv) v2 = u[k2 - 3];
        WAVE_SYNC();
        if (k0 < nv) u[k0] = v0;
        if (k1 < nv) u[k1] = v1;
        if (k2 < nv) u[k2] = v2;
      } else if (f_alt < f_warm && lane == 0) {
        reinterpret_cast<int*>(L + a.lds.state)[SI_HAS_PREV] = kAltArmed;
      }
      WAVE_SYNC();
    }
  }
  s.flags = flags; s.cold = cold;
  return true;
}

// ---- the search's arrays in LDS (layout: solver_context.h)
struct SearchLds {
  double *u, *gs, *gt, *gr, *d, *u_prev, *gt_prev, *u_new, *ACS, *ASN;
  int* AMODE;  // [4n]: mode, wfroz, near, near_prev
};
__device__ __forceinline__ SearchLds search_lds(const SolveArgs& a, double* L) {
  SearchLds m;
  m.u = L + a.lds.u;
  m.gs = L + a.lds.gs;
  m.gt = L + a.lds.gt;
  m.gr = L + a.lds.gr;
  m.d = L + a.lds.d;
  m.u_prev = L + a.lds.u_prev;
  m.gt_prev = L + a.lds.gt_prev;
  m.u_new = L + a.lds.u_new;
  m.ACS = L + a.lds.cs;
  m.ASN = L + a.lds.sn;
  m.AMODE = reinterpret_cast<int*>(L + a.lds.mode);
  return m;
}

// ---- phases 1 and 2: the search, the cell scan behind it, and the search once more behind a scan that paid.
// The phases of an iteration are text here, between the NEO_PHASE marks: each was tried as a function of its own, and each
// changed the kernels' code (docs/NOTEBOOK.md A.29 has the counts).  Returns true when a test hook has dumped what it was
// asked for (the kernel ends there).
// (tools/: the lines between the two K1-SEARCH-LOOP marks are what the static tables call "the loop", and they find the
// routed kernel's two searches by the K1-ROUTED-*-SEARCH marks)
template <class V>
__device__ __forceinline__ bool solve_search(double* L, uint32_t b, SolveCarry& sc) {
  // (the variant's constants under the names the text below has always used; what each means: K1Variant.  A bridge while
  // the phases are text of this function: a phase that becomes a function takes V itself, and its names leave this list)
  constexpr int kMinWavesPerSimd = V::kMinWavesPerSimd, kSteps = V::kSteps, kFew = V::kFew, kNwSteps = V::kNwSteps;
  constexpr int kVars = V::kVars, kRegSteps = V::kRegSteps, kPairs = V::kPairs;
  constexpr bool kTame = V::kTame, kRouted = V::kRouted, kCovered = V::kCovered, kNewton = V::kNewton, kRiccati = V::kRiccati;
  constexpr bool kSecond = V::kSecond, kBlockedRule = V::kBlockedRule, kHandOff = V::kHandOff, kFewTame = V::kFewTame;
  constexpr bool kVectorPose = V::kVectorPose;
  double f = sc.f;
  const bool cold = sc.cold;
  // ---- what the search carries from one iteration to the next -- and across the cell scan when it is taken up again
  int npairs = 0, head = 0, nfev = sc.nfev, it = sc.it, status = sc.status;
  neo_search_run run;    // what the stop rules carry (solver_rules.h; three-stage kernels: the gains wait in LDS, T_GAIN1 / T_GAIN2)
  neo_search_run_init(&run);
  double u_term = 0.0;   // dense Newton: sum of the costmap terms under the current iterate's rollout (0: every stage in a free cell)
  double alpha = 1.0;
  bool scanned = false;   // the cell scan has had its turn (cell_scan.h)
  int nscans = 0;         // ... scans of its round so far: a scan that found a cheaper cell is followed by another from the new point
  bool scan_only = false; // this pass of the loop below only scans again
  NEO_SEGMENT_DECL;
  NEO_SEGMENT(0);
  for (;;) {   // (the search; taken up again behind a cell scan that paid)
  // ---- phase 1: the search
  SolveArgs a;
  fresh_args<V>(a);
  own_loop_params(a);
  select_map(a.map, L + a.lds.prob);
  const DevParams& p = a.p;
  const int n = kSteps ? kSteps : p.n, nv = 3 * n, mem = p.mem;
  double cand[3 * kRegSteps], cand_sn[kRegSteps], cand_cs[kRegSteps];
  bool have_trig = false;  // ACS/ASN already hold sin/cos of the rollout at u
  Ctx c;
  ctx_from_lds<kVectorPose>(a, L, c);
  const SearchLds m = search_lds(a, L);
  if (!scanned && nscans == 0) {
    const int lane = lane_again();
    for (int i = lane; i < n; i += kLanes) { m.AMODE[4 * i + 2] = 0; m.AMODE[4 * i + 3] = 0; }
    // (routed stage-wise branch: this direction's prox-only zone around the kink -- the set-up wrote the dense direction's)
    if (kRouted && lane == 0) L[a.lds.tol + T_KINK] = p.kink_radius_stagewise;
    // Long horizons (Riccati direction): the curvature of a block falls with 1/N^2, so the proximal step starts
    // longer; and the Newton step is long along the valleys in which neighbouring blocks trade displacement and
    // leaves the region where the model holds -- Levenberg-Marquardt damping mu (in units of one stage's tracking
    // weights, riccati_prepare), relaxed x1/4 after an iteration won by the (nearly) full Newton step, tightened
    // x4 after one won by a proximal step or a short Newton step.  Nothing of it at control_steps <= 8.
    alpha = kRiccati ? fmax(1.0, n * 0.125) : 1.0;
    // (routed stage-wise branch: what the search carries between iterations waits in the tolerance block of LDS -- kept in
    // registers across the 64-candidate pass, whose candidates sit in registers themselves, it came out spilled to scratch)
    if (kFew && lane == 0) { double* t = L + a.lds.tol; t[T_GAIN1] = INFINITY; t[T_GAIN2] = INFINITY; t[T_ALPHA] = alpha; }
    // (mu lives in the tolerance block of LDS: two scalar registers fewer across the loop)
    if (kRiccati && lane == 0) L[a.lds.tol + T_MU] = n > 8 ? (double)(n - 8) * 0.125 : 0.0;
    // (three tame stages: every lane parks its step multiplier in LDS, once per search -- k1_variant.h kRoutedLaneScales;
    // the candidates phase reads it back)
    if (kFewTame) L[kRoutedLaneScales + lane] = kLaneScales<kSecond>.v[lane];
  }
  // Riccati: a block may be sent straight onto the kink u_i = v_cur only when v_cur is feasible
  bool v_feasible = false;
  if (kRiccati) {
    double b0 = c.v0, b1 = c.v1, b2 = c.v2;
    asm volatile("" : "+v"(b0), "+v"(b1), "+v"(b2));   // (copies of their own: vector copies of v_cur must not outlive this test)
    project_block<kTame>(p, b0, b1, b2);
    v_feasible = b0 == c.v0 && b1 == c.v1 && b2 == c.v2;
  }
  // this lane's step multiplier: the one lane-derived constant worth two registers for the whole loop
  // (half of the table sits in constant memory: re-reading it would put a global load on every
  // iteration's critical path)
  double my_scale;
  {
    int l0 = lane_again();
    my_scale = kRiccati ? 0.0 : lane_scale<kSecond>(l0);
  }
  for (; it < p.max_it && !scan_only; ++it) {   // K1-SEARCH-LOOP-BEGIN
    // The lane index is re-read opaquely every iteration: otherwise the compiler hoists two dozen
    // lane-derived constants (step multipliers, compare masks, LDS addresses) out of the loop and,
    // at 4 waves/SIMD, parks them in scratch -- recomputing them costs a few integer operations.
    int lane = lane_again();
    // stage-wise direction: this iteration's sweep carries the second-order terms of the rollout step
    const bool exact_step = kRiccati && run.nblocked == 0;
    // (same trick for the tolerance block: an opaque LDS offset keeps its loads inside the loop and in
    // the LDS address space -- a volatile pointer would turn them into flat loads with a full wait each)
    int tol_off = a.lds.tol;
    asm volatile("" : "+s"(tol_off));
    const double* TOL = L + tol_off;
    NEO_PHASE_DECL;
    NEO_PHASE(0);
    // ---- adjoint gradient of the tracking + terminal cost
    const int nvr = kSteps ? kVars : nv;  // its size
    bool free_path = false;   // Riccati: every stage of the rollout at u sits in a free cell (raw cost 0)
    int nhops = 0;            // Riccati: hop candidates of this iteration (wave-uniform; the table is in the tolerance block)
    float hc[kVars];     // Newton: column `lane` of the Hessian, then row `lane` (float32, see below)
    float newton_sol = 0.0f;  // Newton: entry `lane` of the direction
    float dm_reg = 0.0f;                // kHandOff: the step test's maximum over this lane's three entries of d (riccati_finish)
    int near_reg = 0;                   // ... and the near word of the lane's stage
    StageCarry carry = {};              // kFewTame: the cone pass' operands, fetched at the adjoint pass' end
    if (kNewton) { NEO_DENSE_NEWTON_HESSIAN_PASS(kSteps, kNwSteps, kTame, kVars, p, c, m.u, m.gs, hc, lane, n); }   // (dense_newton.h)
    else if (!kSteps || kRiccati) adjoint_by_scans<kTame, kRiccati, kFew, kCovered>(a, c, L, exact_step, lane, n, free_path, nhops, kFewTame ? &carry : nullptr);
    else adjoint_short_sweep<kSteps, kTame>(a, c, L, have_trig, lane, n);
    NEO_PHASE(1);
    // ---- total gradient (control norm: minimal-norm subgradient at the kink), tangent-cone reduction at active bounds,
    //      face records of the second-order directions (tangent_cone.h)
    const bool my_corner = tangent_cone_pass<kTame, kNewton, kRiccati>(a, c, L, TOL[T_KINK], lane, n, kFewTame ? &carry : nullptr);
    WAVE_SYNC();
    // (in free space only -- no costmap term under the iterate's rollout: next to a cost step the Newton model is off either
    // way; the dense kernel knows that sum from the previous iteration's winner)
    const bool corner_any = kSecond && !kTame && __ballot(my_corner) != 0ull && (kRiccati ? free_path : (it > 0 && u_term == 0.0));
    NEO_PHASE(2);
    if (p.max_it == kDumpGradient) {
      // test hook (neo_mpc_gradient_batch): hand back the total gradient this kernel variant works with at
      // the projected x0 -- adjoint gradient of the smooth part + gradient of the control norm -- and stop
      for (int k = lane; k < nv; k += kLanes) a.solution[(size_t)b * nv + k] = m.gt[k];
      return true;
    }
    if (kSecond && it == 0 && cold) {
      // a cold start (x0 = 0, the reference's reset state py:359) is far from the minimiser and the
      // Newton step almost never wins there: steepest descent on the face for this one iteration
      if (kRiccati) { for (int k = lane; k < nv; k += kLanes) m.d[k] = -m.gr[k]; }
      else if (lane < nvr) m.d[lane] = -m.gr[lane];
      if (kRiccati) for (int i = lane; i < n; i += kLanes) m.AMODE[4 * i + 3] = 0;
      WAVE_SYNC();
    } else if (kRiccati) {
      const int my_flags = riccati_prepare(a, c, L, n, lane, v_feasible, (float)TOL[T_MU]);
      // (the stages' cases as scalars: the sweep's switch does not wait for the record, its conversion and a lane read)
      int stage_flags[kFew ? kFew : 1] = {};
      if (kFewTame) {
        for (int i = 0; i < kFew; ++i) stage_flags[i] = __builtin_amdgcn_readlane(my_flags, i);
      }
      WAVE_SYNC();
      if (corner_any) riccati_keep_linear_terms(a, L, n, lane, true);   // (the sweep writes its gains over them)
      auto sweep = [&]() {
        SweepHandOff<float> ho = {};
        riccati_sweep<float, (kMinWavesPerSimd < 4), kFew, kHandOff, kFewTame, kFewTame>(a, L, n, lane, &ho, stage_flags);
        riccati_finish<kHandOff>(a, c, L, n, lane, &ho, &dm_reg);
        near_reg = ho.near;
      };
      sweep();
      if (!kTame && corner_any && repin_corner_blocks<true>(a, L, n, lane)) {   // (one-sided slides: once more, those blocks pinned)
        riccati_keep_linear_terms(a, L, n, lane, false);
        sweep();
      }
    } else if (kNewton) {
      newton_sol = dense_newton_direction<kSteps, kNwSteps, kTame>(a, L, hc, corner_any, lane, n, nvr);   // (dense_newton.h)
    }
    NEO_PHASE(3);
    // ---- projected L-BFGS: newest curvature pair, two-loop recursion on the reduced gradient, restriction to the face
    if (!kSecond) lbfgs_direction<kSteps, kPairs>(a, L, it, mem, head, npairs, lane, n);   // (lbfgs.h)
    if (kSecond && it > 0) {
      // the Newton step test (solver_rules.h neo_rules_step_test) on the largest entry of d and on "a block next to the kink"
      float dm = 0.0f;
      int anynear = 0;
      if (kHandOff) {
        // (riccati_finish has applied the rule below to the three entries of the lane's stage; the lanes without a stage hold
        // zero.  dm is the maximum of the magnitudes, or INFINITY as soon as one entry is NaN -- a maximum of non-negative
        // numbers that are not NaN does not depend on the order it is taken in, and INFINITY absorbs everything behind it:
        // three entries per lane, then three lanes, give the bits that one entry per lane over nine lanes gave;
        // tests/test_stagewise_phases.py holds the two orders against each other)
        dm = dm_reg;
        anynear = near_reg == 1;
      } else if (kRiccati) {
        // (a non-finite direction must not read as "no step left": fmaxf drops NaN)
        for (int k = lane; k < nv; k += kLanes) {
          const float v = (float)fabs(m.d[k]);
          dm = (v == v) ? fmaxf(dm, v) : INFINITY;
          anynear |= (m.AMODE[4 * (k / 3) + 2] == 1);
        }
      } else if (lane < nvr) { dm = fabsf(newton_sol); anynear = (m.AMODE[4 * (lane / 3) + 2] == 1); }   // (d[lane], still in a register)
      // (three stages: nine values in lanes 0-8, each finite and non-negative or INFINITY -- one DPP row)
      if constexpr (kHandOff) dm = wave_max_f_few<kFew>(dm);
      else if constexpr (kFew > 0 && 3 * kFew <= 16) dm = wave_max_f_few<3 * kFew>(dm); else dm = wave_max_f(dm);
      const bool near_any = __ballot(anynear != 0) != 0ull;
      const int verdict = neo_rules_step_test((double)dm, near_any, nhops, TOL[T_EARLY], TOL[T_FINAL], kRiccati && !exact_step);
      if (verdict == NEO_STEP_CONVERGED) { status = NEO_MPC_STATUS_CONVERGED; break; }
      if (verdict == NEO_STEP_IS_LAST) run.final_step = true;
    }
    NEO_PHASE(4);
    if (p.max_it > kDumpGradient && it == p.max_it - kDumpGradient - 1) {
      // test hook (neo_mpc_direction_batch): the search direction of lanes 32-63 in this iteration
      for (int k = lane; k < nv; k += kLanes) a.solution[(size_t)b * nv + k] = m.d[k];
      return true;
    }
    // ---- 64 candidates, one rollout per lane; lowest objective wins
    // (run-time-sized Riccati kernel: the multiplier is re-read here -- one constant-memory load per iteration
    // against 2 x control_steps stages of work, and two registers fewer across the sweep)
    // (three tame stages, a wave alone on its SIMD at the launch's end: the constant-memory load was the loop's only
    // vector-memory round trip, fully exposed, behind three lane-divergent arms.  The multiplier comes from LDS instead,
    // where the search's entry parked it -- one read next to T_ALPHA's, through the same opaque offset, one wait for both)
    const double lscale = kFewTame ? TOL[kRoutedLaneScales - V::kLayout.tol + lane] : kRiccati ? lane_scale<kSecond>(lane) : my_scale;
    const double alpha_now = kFew ? TOL[T_ALPHA] : alpha;
    const double pstep = alpha_now * lscale;
    const double step = lane < 32 ? pstep : lscale;
    bool took_trial = false;
    double fb = INFINITY, cterm = 0.0;   // (cterm, dense Newton: the costmap terms of this lane's candidate alone)
    int best = 32;
    // (stage-wise direction, rollout in free space: the full Newton step is tried on its own first, riccati.h)
    if (kRiccati && free_path && it > 0) took_trial = riccati_free_space_trial<kTame, kCovered, kFew, kBlockedRule>(a, c, L, n, lane, alpha_now, f, fb, cterm);
    // (first iteration only: the set-up armed the un-shifted previous solution as lane kAltLane's candidate)
    const double* ALT0 = L + a.lds.state + S_PREV_U0;
    bool alt_armed = false;
    if (it == 0) alt_armed = uniform_int(reinterpret_cast<const int*>(L + a.lds.state)[SI_HAS_PREV]) == kAltArmed;
    if (!took_trial) {
    // hop lanes (Riccati): lane h in 1..nhops tries the current point with the block of hop stage h - 1 changed
    int hop_stage = -1;
    float hop_x = 0.0f, hop_y = 0.0f;
    if (kRiccati && lane >= 1 && lane <= nhops) {
      const double* t = TOL;
      hop_stage = reinterpret_cast<const int*>(t + T_HOP_STAGE)[lane - 1];
      hop_x = reinterpret_cast<const float*>(t + T_HOP_VEC)[2 * (lane - 1)];
      hop_y = reinterpret_cast<const float*>(t + T_HOP_VEC)[2 * (lane - 1) + 1];
    }
    double fc = rollout_cost<kSteps, kTame, kCovered>(
        a, c, L,
        [&](int i, double& b0, double& b1, double& b2) {
          candidate_block<kTame, kRiccati, kFewTame>(a, c, L, lane, step, pstep, i, b0, b1, b2, hop_stage, hop_x, hop_y);
          // (a scalar branch taken in the first iteration only -- the empty asm keeps the compiler from turning it into
          // six selects per block that every iteration pays)
          if (it == 0) {
            asm volatile("");
            if (lane == 0) { b0 = m.u[3 * i]; b1 = m.u[3 * i + 1]; b2 = m.u[3 * i + 2]; }
            // (the un-shifted previous solution, armed by the set-up on the costmap: block 0 from the state slot)
            if (lane == kAltLane && alt_armed) { const double* src = i == 0 ? ALT0 : m.u + 3 * (i - 1); b0 = src[0]; b1 = src[1]; b2 = src[2]; }
          }
          if (kSteps) { cand[3 * i] = b0; cand[3 * i + 1] = b1; cand[3 * i + 2] = b2; }
        },
        [&](int i, double sn, double cs) {
          if (kSteps && !kSecond) { cand_sn[i] = sn; cand_cs[i] = cs; }
        }, kBlockedRule ? &cterm : nullptr);
    NEO_PHASE(5);
    if (!(fc == fc)) fc = INFINITY;
    if (it == 0) { f = lane_value(fc, 0); if (kNewton) u_term = lane_value(cterm, 0); }
    fb = fc;
    best = lane;
    wave_argmin(fb, best);
    }
    ++nfev;
    if (!(fb < f)) { status = NEO_MPC_STATUS_CONVERGED; ++it; break; }
    const bool alt_won = alt_armed && best == kAltLane;
    float stepmax = 0.0f;
    if (kSteps && kSecond && !took_trial) {
      // the winner holds its candidate in registers: it measures the step against u and overwrites u
      // in place -- one LDS round trip, no staging copy, no wave-wide maximum (the Newton paths keep
      // no previous iterate or gradient)
      if (lane == best) {
#pragma unroll
        for (int k = 0; k < 3 * kRegSteps; ++k) {
          stepmax = fmaxf(stepmax, (float)fabs(cand[k] - m.u[k]));
          m.u[k] = cand[k];
        }
      }
      stepmax = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, stepmax), best));
      have_trig = true;
    } else {
      if (kSteps && !kSecond) {
        if (lane == best) {
#pragma unroll
          for (int i = 0; i < kRegSteps; ++i) {
            m.u_new[3 * i] = cand[3 * i]; m.u_new[3 * i + 1] = cand[3 * i + 1]; m.u_new[3 * i + 2] = cand[3 * i + 2];
            m.ASN[i] = cand_sn[i]; m.ACS[i] = cand_cs[i];
          }
        }
      } else if (!kSteps && !took_trial) {
        // rebuild the winning candidate cooperatively: lane i takes control block i
        const double bstep = lane_value(step, best), bpstep = lane_value(pstep, best);
        int bhop = -1;
        float bhx = 0.0f, bhy = 0.0f;
        if (kRiccati && best >= 1 && best <= nhops) {   // (a hop candidate won)
          bhop = reinterpret_cast<const int*>(TOL + T_HOP_STAGE)[best - 1];
          bhx = reinterpret_cast<const float*>(TOL + T_HOP_VEC)[2 * (best - 1)];
          bhy = reinterpret_cast<const float*>(TOL + T_HOP_VEC)[2 * (best - 1) + 1];
        }
        for (int i = lane; i < n; i += kLanes) {
          double b0, b1, b2;
          candidate_block<kTame, kRiccati>(a, c, L, best, bstep, bpstep, i, b0, b1, b2, bhop, bhx, bhy);
          if (alt_won) { const double* src = i == 0 ? ALT0 : m.u + 3 * (i - 1); b0 = src[0]; b1 = src[1]; b2 = src[2]; }
          m.u_new[3 * i] = b0; m.u_new[3 * i + 1] = b1; m.u_new[3 * i + 2] = b2;
        }
      }
      have_trig = true;
      WAVE_SYNC();
      for (int k = lane; k < nv; k += kLanes) {
        const double nu = m.u_new[k], ou = m.u[k];
        stepmax = fmaxf(stepmax, (float)fabs(nu - ou));
        if (!kSecond) { m.u_prev[k] = ou; m.gt_prev[k] = m.gt[k]; }
        m.u[k] = nu;
      }
      stepmax = wave_max_f(stepmax);
    }
    // ---- does this iteration end the search?  (solver_rules.h neo_rules_iteration_ends: one text for every variant and the mirror)
    // (the un-shifted start that won the first iteration says as little about step lengths as a hop)
    const bool hop_won = (kRiccati && best >= 1 && best <= nhops) || alt_won;
    // (no costmap term under the new iterate's rollout; the closing-in rule's free space -- dense direction: the same;
    // stage-wise: under the rollout the iteration started from)
    const bool free_rollout = kBlockedRule ? lane_value(cterm, best) == 0.0 : false;
    const bool free_now = kRiccati ? free_path : (kNewton ? free_rollout : false);
    // (three tame stages: the rule book's seven tolerance words are launch parameters -- the set-up copied them into the
    // tolerance block word for word -- and this phase reads them where they came from: one scalar fetch through the
    // kernel-argument pointer, one wait, and scalar operands, instead of an LDS round trip behind each of the rule book's
    // conditions; nothing of it is held across the loop)
    double tolk[NEO_TOL_COUNT] = {};
    if (kFewTame) {
      auto kp = (const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr();
      asm volatile("" : "+s"(kp));
      const DevParams& q = ((const SolveArgs*)kp)->p;
      tolk[NEO_TOL_XTOL] = q.xtol; tolk[NEO_TOL_FTOL] = q.ftol; tolk[NEO_TOL_STALL] = q.stall_step; tolk[NEO_TOL_WTOL] = q.wtol;
      tolk[NEO_TOL_WTOL_LATE] = q.wtol_late; tolk[NEO_TOL_BTOL_MAP] = q.btol_map; tolk[NEO_TOL_BTOL_FREE] = q.btol_free;
    }
    if (kFew) { run.gain1 = TOL[T_GAIN1]; run.gain2 = TOL[T_GAIN2]; }
    // (the gain is wave-uniform but comes out of the vector ALU.  Dense direction: it goes on as a scalar -- the two gains the
    // rules carry are four vector registers held across the Hessian pass, and the run-time-sized kernel at four waves per SIMD
    // parked two more registers in scratch with the rules called than with their text in place)
    const double gain = kNewton ? lane_value(f - fb, 0) : f - fb;
    const bool ends = neo_rules_iteration_ends(kRiccati, kRouted, kBlockedRule, kFewTame ? tolk : TOL, &run, it, best >= 32, lane_value(step, best), hop_won,
                                               gain, fb, (double)stepmax, free_now, free_rollout);
    double* TOLW = L + tol_off;
    if (kFew) { if (lane == 0) { TOLW[T_GAIN2] = run.gain2; TOLW[T_GAIN1] = run.gain1; } }
    f = fb;
    if (kNewton) u_term = lane_value(cterm, best);
    // (a hop that won says nothing about step lengths: damping and proximal step stay as they are)
    if (kRiccati && !(it == 0 && cold) && !hop_won) {   // (an iteration that had a Newton direction)
      // (step lengths of the Newton lanes as lane masks, feasible_set.h: scalar bit tests)
      constexpr unsigned long long kNearlyFull = newton_lanes_at_least(NEO_RULE_DAMP_RELAX_STEP),
                                   kShort = kNewtonLanes & ~newton_lanes_at_least(NEO_RULE_DAMP_TIGHTEN_STEP);
      const double mu0 = n > 8 ? (double)(n - 8) * 0.125 : 0.0, mu = TOL[T_MU];
      double* mu_slot = L + tol_off + T_MU;
      if ((kNearlyFull >> best) & 1ull) { if (lane == 0) *mu_slot = fmax(NEO_RULE_DAMP_RELAX * mu, mu0 * (1.0 / NEO_RULE_DAMP_RANGE)); }
      else if (best < 32 || ((kShort >> best) & 1ull)) { if (lane == 0) *mu_slot = fmin(NEO_RULE_DAMP_TIGHTEN * mu, NEO_RULE_DAMP_RANGE * mu0); }
    }
    if (best < 32 && !hop_won) {
      const double al = clampd(lane_value(step, best), 1e-6, 1e6);
      if (kFew) { if (lane == 0) TOLW[T_ALPHA] = al; }
      else alpha = al;
    }
    WAVE_SYNC();
    NEO_PHASE(6);
    NEO_PHASE_DUMP();
    if (ends) { status = NEO_MPC_STATUS_CONVERGED; ++it; break; }
  }   // K1-SEARCH-LOOP-END

  // ---- phase 2, second-order directions: a search that has ENDED looks once at the costmap cells around every stage
  //      (cell_scan.h): cheaper cells up to three cells away, which no descent direction sees -- the term has no gradient --
  //      and SLSQP's line search samples by accident.  Skipped when the whole reach tile is free or (dense direction: known
  //      from the winner's rollout) no stage of the iterate has a costmap term under it.  Behind a scan that gained more
  //      than opt_tolerance the search is taken up again: the other blocks have a new neighbour to adjust to.
  // (round 6) A scan that found a cheaper cell is followed by another from where it has put the iterate (one pass of this loop
  // each, NEO_RULE_SCAN_REPEATS at most), until a scan finds nothing: the returned point is a fixed point of the scan -- solved
  // again from its own answer an instance used to get a second look and move.  The round as a whole decides about the resume.
  if (!kSecond || scanned || status != NEO_MPC_STATUS_CONVERGED || p.max_it >= kDumpGradient) break;
  const bool nothing_to_scan = (c.tile_geom & kTileFree) || (kNewton && u_term == 0.0);
  if (nothing_to_scan && nscans == 0) break;
  bool resume = false;
  {
    SolveArgs as;
    fresh_args<V>(as);
    select_map(as.map, L + as.lds.prob);
    Ctx cs;
    ctx_from_lds<false>(as, L, cs);
    int ls = lane_again();
    if (nscans == 0 && ls == 0) L[as.lds.tol + T_FSCAN] = f;
    NEO_SEGMENT_SCAN_BEGIN();
    const bool w = !nothing_to_scan &&
                   cell_scan<kSteps, kTame, kCovered>(as, cs, L, f, kNewton ? &u_term : nullptr, nfev, ls, kSteps ? kSteps : as.p.n);
    NEO_SEGMENT_SCAN_END();
    ++nscans;
    scan_only = w && nscans < NEO_RULE_SCAN_REPEATS;
    if (!scan_only) {
      scanned = true;
      WAVE_SYNC();
      resume = L[as.lds.tol + T_FSCAN] - f > as.p.scan_resume_gain && it < as.p.max_it;
      if (kFew && resume) {
        if (ls == 0) { L[as.lds.tol + T_GAIN1] = INFINITY; L[as.lds.tol + T_GAIN2] = INFINITY; }
        WAVE_SYNC();
      }
    }
  }
  if (scan_only) continue;
  if (!resume) break;
  status = NEO_MPC_STATUS_MAX_ITER;
  neo_search_run_init(&run);
  }
  NEO_SEGMENT(1);
  NEO_SEGMENT_DUMP();
  // (a search taken up again behind a scan that runs into the iteration cap HAD converged, and the scan only improved its
  // point: it is reported converged -- status 1 would hand the warm start back un-shifted, py:399-400, for a better answer)
  if (scanned && status == NEO_MPC_STATUS_MAX_ITER) status = NEO_MPC_STATUS_CONVERGED;
  sc.f = f; sc.it = it; sc.nfev = nfev; sc.status = status;
  return false;
}

// ---- phase 3: K2 (py:365-403) on the search's result
template <class V>
__device__ __forceinline__ void solve_finish(double* L, uint32_t b, int lane, const SolveCarry& sc) {
  const int flags = sc.flags, status = sc.status, it = sc.it, nfev = sc.nfev;
  double f = sc.f;
  SolveArgs a;
  fresh_args<V>(a);
  select_map(a.map, L + a.lds.prob);
  const DevParams& p = a.p;
  const int n = V::kSteps ? V::kSteps : p.n, nv = 3 * n;
  double* u = L + a.lds.u;
  Ctx c;
  ctx_from_lds<false>(a, L, c);
#ifndef NEO_MPC_PHASE_TIMING
  // (test hooks: a search that ended before the dumped iteration keeps the NaN row the host put there)
  if (a.solution && p.max_it < kDumpGradient)
    for (int k = lane; k < nv; k += kLanes) a.solution[(size_t)b * nv + k] = u[k];
#endif
  WAVE_SYNC();
  f += L[a.lds.tol + T_KONST];
  c.true_yaw = L[a.lds.tol + T_TRUE_YAW];
  postprocess(a, c, L, b, lane, u, status == NEO_MPC_STATUS_CONVERGED, L[a.lds.prob + P_FOOTPRINT], flags, f, status, it, nfev);
}

// ---------------------------------------------------------------- K1: the kernels
// What every K1 kernel starts with: its LDS -- the static array of the kStaticTile variants, else the launch's dynamic
// LDS -- and the instance its workgroup solves.
// (the static array belongs to solve_lds<V>, not to a kernel: k_solve<w, 3, 1, t, tile> and k_solve_routed<w, t, tile> build
// the same V and name the same array.  They are in different units today; whether two kernels of ONE unit that share it get
// an allocation each is the compiler's business -- check `make resource-usage` (LDS size) if that ever happens)
template <class V>
__device__ __forceinline__ double* solve_lds() {
  extern __shared__ __align__(16) double Ldyn[];
  __shared__ __align__(16) double Lstat[V::kStaticDoubles];
  return V::kStaticTile ? Lstat : Ldyn;
}
// (balanced dispatch, neo_mpc_balance_dispatch_device: which instance this workgroup solves -- instances are independent,
// every result is bit for bit what it is in launch order; only which of them share a SIMD changes)
__device__ __forceinline__ uint32_t solve_instance(const SolveArgs& args) {
  return args.order ? (uint32_t)__builtin_amdgcn_readfirstlane((int)args.order[blockIdx.x]) : blockIdx.x;
}

// The prologue of both kernels: declares L (the kernel's LDS), lane, and b (the instance this workgroup solves), and ends the
// kernel where there is none -- a workgroup beyond the count, or an order the caller launched this solve ahead of, on
// another stream (never out of range).
// A MACRO: `return` has to be the kernel's own.  As a function that reports "none" (a bool, a sentinel) or that takes the
// kernel's body as a callable and returns early itself, the compiler lays 18 to 36 of the 36 K1 kernels out differently
// (docs/NOTEBOOK.md A.29); as text they are instruction for instruction what they were.
#define NEO_K1_PROLOGUE(V, args)             \
  double* const L = solve_lds<V>();          \
  const int lane = threadIdx.x;              \
  if (blockIdx.x >= (args).count) return;    \
  const uint32_t b = solve_instance(args);   \
  if (b >= (args).count) return

// k_solve<waves per SIMD, control_steps specialisation, direction, tame, static tile>: one direction for every instance.
template <int kMinWavesPerSimd, int kSteps, int kDir = 0, bool kTame = false, int kStaticTile = 0>
__global__ __launch_bounds__(kLanes, kMinWavesPerSimd) void k_solve(const SolveArgs args) {
  using V = K1Variant<kMinWavesPerSimd, kSteps, kDir, kTame, kStaticTile>;
  NEO_K1_PROLOGUE(V, args);
  NEO_WAVE_START;
  SolveCarry sc;
  if (!solve_setup<V>(L, b, lane, sc)) return;
  if (solve_search<V>(L, b, sc)) return;
  solve_finish<V>(L, b, lane, sc);
  NEO_WAVE_END_ARGS(args);
}

// k_solve_routed: control_steps 3, AUTO below the heavy-costmap threshold -- DIRECTION BY NEIGHBOURHOOD (round 6;
// solver_rules.h neo_rules_routes_by_neighbourhood).  The set-up stages the reach tile and knows whether a LETHAL cell is among
// its cells.  No wall in reach (88 % of the BASELINE config-2 instances): the dense projected Newton search (registers,
// finite-difference Hessian) with the cell scan behind it -- round 5's headline kernel.  A wall in reach: the stage-wise
// (Riccati) search, whose wall model slides along walls -- every objective miss the random-parameter fuzz against the reference
// found at control_steps 3 was a dense search hemmed in by lethal cells.  One launch, one wave per instance, one wave-uniform
// branch behind the set-up; the two branches share LDS (the stage-wise carve-up for three stages lies inside the dense one,
// K1Variant) and the register budget (128 at four waves per SIMD, no scratch).
template <int kMinWavesPerSimd, bool kTame = false, int kStaticTile = 0>
__global__ __launch_bounds__(kLanes, kMinWavesPerSimd) void k_solve_routed(const SolveArgs args) {
  using Dense = K1Variant<kMinWavesPerSimd, kRoutedSteps, 1, kTame, kStaticTile>;
  using Stagewise = K1Variant<kMinWavesPerSimd, kRoutedSteps, 2, kTame, kStaticTile, true>;
  NEO_K1_PROLOGUE(Dense, args);
  NEO_WAVE_START;
  SolveCarry sc;
  if (!solve_setup<Dense>(L, b, lane, sc)) return;
  // (the test hooks dump what the instance's own direction works with)
  if (__builtin_amdgcn_readfirstlane((int)sc.wall_in_reach)) {
    // (the stage-wise searches are the long ones -- 7.3 iterations against 5.1, up to 19 against 11, 1.5 x the instructions per
    // iteration -- and a launch of 4096 ends with the longest of them: they issue ahead of the dense waves they share a SIMD
    // with, which finish early either way.  Same box, three runs each: 23.0 -> 24.5 M solves/s; 262 144 instances: no change)
    __builtin_amdgcn_s_setprio(3);
    if (solve_search<Stagewise>(L, b, sc)) return;   // K1-ROUTED-STAGEWISE-SEARCH
  } else {
    if (solve_search<Dense>(L, b, sc)) return;   // K1-ROUTED-DENSE-SEARCH
  }
  solve_finish<Dense>(L, b, lane, sc);
  NEO_WAVE_END_ARGS(args);
}

// ---------------------------------------------------------------- K1: launching
// Register budget of K1: with the per-iteration opaque lane index (see the top of the solver loop) the Newton kernel needs
// 124 VGPRs and the generic kernel 118, both spill-free at 4 waves/SIMD; the control_steps == 3 L-BFGS kernel needs 130
// (3 waves/SIMD).  __launch_bounds__ pins the occupancy each was measured at, so that a later edit cannot silently drop a
// wave per SIMD (it would spill instead, which `make resource-usage` shows).  NEO_MPC_SOLVE_WAVES=2|3|4 in the environment
// of neo_mpc_create overrides (LaunchTuning), for A/B runs.
int solve_variant(const LaunchTuning& t, int fallback) { return t.solve_waves ? t.solve_waves : fallback; }

// What the two dispatch tables (launch_solve, launch_solve_riccati) know before they pick a row, and the launch itself.
using SolveKernel = void (*)(const SolveArgs);
struct K1Launch {
  const SolveArgs& a;
  void *stream, *ev_start, *ev_stop;
  bool disc;         // the tame instantiations apply (K1Variant kTame)
  size_t lds;        // the launch's dynamic LDS
  // (the static-tile kernels count on the tile being there: no tile at all -- a reach of 60 cells and more -- is not "small")
  bool small_tile;
  K1Launch(const SolveArgs& a_, const LaunchTuning& tuning, void* stream_, void* ev_start_, void* ev_stop_)
      : a(a_), stream(stream_), ev_start(ev_start_), ev_stop(ev_stop_),
        disc(a_.p.tame != 0 && !tuning.no_tame), lds(a_.lds.total_bytes),
        small_tile(a_.lds.tile_w * a_.lds.tile_h > 0 && a_.lds.tile_w * a_.lds.tile_h <= 1024 && !tuning.dynamic_lds) {}
  // One launch of a K1 kernel, one workgroup per instance; `lds_bytes`: its dynamic LDS (0 for the static-tile variants).
  // with events: hipExtLaunchKernel stamps them from the dispatch packet itself (no barrier packets in
  // front of and behind the kernel, which is what separate hipEventRecord calls put on the queue)
  void operator()(SolveKernel kernel, size_t lds_bytes) const {
    const dim3 grid(a.count), block(kLanes);
    hipEvent_t e0 = (hipEvent_t)ev_start, e1 = (hipEvent_t)ev_stop;
    if (e0 || e1) hipExtLaunchKernelGGL(kernel, grid, block, lds_bytes, (hipStream_t)stream, e0, e1, 0, a);
    else hipLaunchKernelGGL(kernel, grid, block, lds_bytes, (hipStream_t)stream, a);
  }
};
// the variant of `kernel<waves per SIMD, ...>` built for w = 4, 3 or (anything else) 2 waves per SIMD
#define NEO_K1_BY_WAVES(w, kernel, ...) \
  ((w) == 4 ? (SolveKernel)kernel<4, __VA_ARGS__> : (w) == 3 ? (SolveKernel)kernel<3, __VA_ARGS__> : (SolveKernel)kernel<2, __VA_ARGS__>)

}  // namespace
}  // namespace neo_mpc
