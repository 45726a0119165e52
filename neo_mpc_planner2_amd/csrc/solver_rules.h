/* solver_rules.h -- the rule book of the search: every constant and derived tolerance, ONCE, and the
 * decisions that use them, ONCE -- does the Newton step test end the search or announce the last step, does the iteration
 * that has taken its winner end it (the end of this file).
 *
 * Plain C: included by the host side of the library (neo_mpc_capi.cpp: derive()), by the device code (k1_solve.h, costmap.h;
 * the decisions are __host__ __device__ there) and by the CPU mirror of the search that the test infrastructure keeps
 * (mpc_oracle.c, part 2 -- the mirror follows the build's algorithm by construction and takes its rule book from here; the
 * restatement of the REFERENCE in the same file shares nothing with the product).  A threshold or a rule changed here changes
 * on the GPU and in the mirror at once. */
#ifndef NEO_MPC_SOLVER_RULES_H_
#define NEO_MPC_SOLVER_RULES_H_

#include <math.h>
#include <stdbool.h>

#include "../../include/neo_mpc.h"

/* ---- stop rules */
#define NEO_RULE_STALL_ITERATIONS 5     /* consecutive iterations gaining < ftol (relative) or moving < stall_step that end the search */
#define NEO_RULE_BLOCKED_RUN 3          /* dense direction: this many iterations in a row not won by a decent Newton step ... */
#define NEO_RULE_BLOCKED_STEP 0.25      /* ... (a proximal lane, or a Newton step cut below this) arm the blocked-run rule */
#define NEO_RULE_BLOCKED_TOL_MAP 0.1    /* ... which fires when they gained less than this x opt_tolerance together (costmap term under the rollout) */
#define NEO_RULE_BLOCKED_TOL_FREE 0.03  /* ... (no costmap term under the rollout) */
#define NEO_RULE_LATE_ITERATION 20      /* from here on the three-iteration window is the control_steps-3 one */
#define NEO_RULE_CORNER_ROOM 1e-9        /* second-order directions: a sliding block this close (m/s) to ANOTHER constraint sits in a corner of the feasible set (repin_corner_blocks) */
#define NEO_RULE_CLOSING_RUN 2           /* dense / L-BFGS: blocked iterations in a row before the closing-in rule may end the search */
#define NEO_RULE_WINDOW_STEP 0.5        /* stage-wise direction: an iteration won by a Newton step of at least this length is not "blocked" */
#define NEO_RULE_FINAL_FRAC_GN 0.3      /* a Gauss-Newton (not exact) full step has to be this much shorter than opt_tolerance to be the last */
#define NEO_RULE_TRIAL_RATIO 0.75       /* stage-wise direction, free space: the full step is taken alone when it achieves this share of the predicted decrease */
#define NEO_RULE_KINK_RADIUS 3e-3       /* blocks closer to the control norm's kink are left to the proximal step (dense / L-BFGS directions) */
#define NEO_RULE_KINK_RADIUS_STAGEWISE 1e-4   /* ... (the stage-wise direction predicts landings on the kink inside its sweep) */
/* ---- the piecewise-constant costmap term: wall model and hop candidates (costmap.h) */
#define NEO_RULE_STICKY 100.0           /* penalty on motion across a rising cost step, in units of the tracking curvature */
#define NEO_RULE_STICKY_DIST 0.02       /* ... for stages closer than this to the cell edge (cells) */
#define NEO_RULE_WALL 1e4               /* ... behind a lethal cell */
#define NEO_RULE_WALL_DIST 0.1          /* wall zone and stand-off (cells) */
#define NEO_RULE_HOP_DIST 0.25          /* a cheaper cell is worth a hop candidate when its edge is closer than this (cells) ... */
#define NEO_RULE_HOP_MAX_DV 0.05        /* ... and the hop changes a velocity by less than this (m/s) */
#define NEO_RULE_HOP_MARGIN 0.01        /* a hop lands this far inside the cheaper cell (cells) */
#define NEO_RULE_HOP_MIN_DROP 0.1       /* ... worth it when the term drops by more than this x opt_tolerance */
#define NEO_RULE_HOP_LANES 4
/* ---- cell scan (cell_scan.h): what a search that has ended does about cheaper cells further away than a hop */
#define NEO_RULE_SCAN_CELLS 3           /* the scan looks at the (2 x this + 1)^2 - 1 cells around every stage ... */
#define NEO_RULE_SCAN_RESUME_GAIN 1.0   /* ... and the search is taken up again behind a scan that gained more than this x opt_tolerance */
#define NEO_RULE_SCAN_REPEATS 1         /* scans in a row behind a search: a scan that found a cheaper cell could be followed by another from the new point -- measured (mirror, config 2): the answers that are fixed points of the whole solve to 1e-3 go 95.8 % (1) -> 97.3 % (2) -> 97.7 % (8), each to a LOWER objective; on the GPU every scan of a launch's last waves lengthens the launch: the dense kernel 0.093 -> 0.109 ms (2) -> 0.139 ms (8).  One it stays */

/* search direction of lanes 32-63 */
#define NEO_DIRECTION_LBFGS 0
#define NEO_DIRECTION_DENSE 1
#define NEO_DIRECTION_STAGEWISE 2

typedef struct neo_rules {
  int direction;        /* NEO_DIRECTION_* */
  int max_iterations, lbfgs_memory;
  double xtol;          /* step tolerance */
  double final_tol;     /* Newton directions: a full step below this is the last one */
  double ftol;          /* an iteration gaining less than this (relative to the u-dependent objective) counts as stalled */
  double stall_step;    /* ... or moving less than this */
  double wtol, wtol_late;   /* three iterations together gaining less than this (relative) end the search; 0: off */
  double btol_map, btol_free;   /* blocked-run rule (absolute); 0: off */
  double kink_radius;
  double hop_min_drop;  /* absolute */
  double scan_resume_gain;   /* absolute */
  double flat;          /* (3 / control_steps)^2 beyond 3 control steps with a Newton direction, else 1 */
} neo_rules;

/* AUTO = dense Newton at control_steps 3 unless the costmap weight is heavy (the wall model lives in the stage-wise
 * direction), stage-wise otherwise; NEWTON = dense (control_steps <= 8).  A pinned LBFGS / NEWTON at a heavy costmap weight
 * (refused by neo_mpc_create; reachable through neo_mpc_set_params on a live handle) runs the stage-wise direction. */
static inline int neo_rules_direction(const neo_mpc_params* p) {
  const int heavy_costmap = p->w_costmap > 0.25 * p->w_trans;
  return heavy_costmap && p->method != NEO_MPC_METHOD_AUTO ? NEO_DIRECTION_STAGEWISE
         : p->method == NEO_MPC_METHOD_LBFGS ? NEO_DIRECTION_LBFGS
         : p->method == NEO_MPC_METHOD_NEWTON ? NEO_DIRECTION_DENSE
         : p->method == NEO_MPC_METHOD_RICCATI ? NEO_DIRECTION_STAGEWISE
         : (p->control_steps == 3 && !heavy_costmap ? NEO_DIRECTION_DENSE : NEO_DIRECTION_STAGEWISE);
}

/* hop range in cells for a map of this resolution (dt = prediction_horizon / control_steps) */
static inline double neo_rules_hop_range(double dt, double resolution) {
  return fmin(NEO_RULE_HOP_DIST, NEO_RULE_HOP_MAX_DV * dt / resolution);
}

/* Cells a feasible rollout can get away from the robot's own cell, + 1: the radius of the LDS reach tile (neo_mpc_capi.cpp) and
 * of the cell scan -- the scan looks at no cell further than this from the robot's cell (Chebyshev), so that every kernel
 * variant, tile or no tile, and the CPU mirror consider the same cells. */
static inline int neo_rules_reach_cells(const neo_mpc_params* p, double resolution) {
  const double bx = fmax(fabs(p->min_vel_x), fabs(p->max_vel_x)), by = fmax(fabs(p->min_vel_y), fabs(p->max_vel_y));
  const double vmax = fmin(p->max_vel_trans, hypot(bx, by));
  const double cells = ceil(vmax * p->prediction_horizon / resolution);
  return cells < 1e6 ? (int)cells + 1 : 1000001;
}

/* Width in bytes of the reach tile's rows for a reach of R cells (a power of two that covers 2 R + 1 cells from a column
 * aligned to 4), 0: no tile (neo_mpc_capi.cpp derive(); the CPU mirror's copy of the neighbourhood test below). */
#define NEO_RULE_MAX_TILE_REACH 60
#define NEO_RULE_MAX_TILE_WIDTH 128
static inline int neo_rules_tile_width(int reach) {
  if (reach > NEO_RULE_MAX_TILE_REACH) return 0;
  int w = 4;
  while (w < 2 * reach + 4) w <<= 1;
  return w <= NEO_RULE_MAX_TILE_WIDTH ? w : 0;
}

/* Direction by neighbourhood (round 6).  AUTO at control_steps 3 below the heavy-costmap threshold used to mean the dense
 * direction for every instance.  It has no wall model, and every objective miss the random-parameter fuzz against the
 * reference found at control_steps 3 since round 4 (five in 7200 costmap cases: the builder's 30027, the round-5 review's
 * 61020, 61027, 62024 x 2) was a dense search hemmed in by LETHAL cells -- a wall no candidate crosses: the objective jumps by
 * 1000 / control_steps behind it, every longer step is rejected, the blocked-run rule ends the search with smooth cost left on
 * the table -- while the stage-wise direction, whose wall model slides along such walls, solved all five.  Each instance now
 * takes the direction its neighbourhood asks for: WALL IN REACH (a lethal cell, raw 254, or the outside of the map, among the
 * cells of the reach tile -- rows [my0 - R, my0 + R], columns from (mx0 - R) & ~3, neo_rules_tile_width(R) of them, (mx0, my0)
 * the robot's cell, R = neo_rules_reach_cells) -> stage-wise; no wall in reach -> dense, with the cell scan behind it for the
 * ordinary cost steps as before.  12 % of the BASELINE config-2 instances have a wall in reach.  One launch, one kernel: the
 * wave branches once, behind the set-up that stages the tile (k_solve_routed).  Measured on the CPU mirror against the
 * reference: 305 random parameter sets, 3660 costmap cases, no objective miss (routing on ANY non-free cell -- half of the
 * config-2 instances -- gives the same count). */
static inline int neo_rules_routes_by_neighbourhood(const neo_mpc_params* p) {
  return p->method == NEO_MPC_METHOD_AUTO && p->control_steps == 3 && !(p->w_costmap > 0.25 * p->w_trans);
}

/* All thresholds derive from opt_tolerance (the reference's SLSQP ftol, py:364) unless the caller set one explicitly.
 * neo_rules_derive_as: for a given direction (an instance routed to the stage-wise direction takes that direction's rules). */
static inline void neo_rules_derive_as(const neo_mpc_params* p, int direction, neo_rules* r) {
  const int n = p->control_steps;
  r->direction = direction;
  const int newton = r->direction != NEO_DIRECTION_LBFGS;
  r->max_iterations = p->max_iterations > 0 ? p->max_iterations : 100;
  r->lbfgs_memory = p->lbfgs_memory > 0 ? p->lbfgs_memory : 4;
  r->xtol = p->step_tolerance > 0.0 ? p->step_tolerance : 1e-3 * p->opt_tolerance;
  r->final_tol = p->step_tolerance > 0.0 ? p->step_tolerance : p->opt_tolerance;
  r->stall_step = p->stall_step > 0.0 ? p->stall_step : 0.3 * p->opt_tolerance;
  r->kink_radius = p->kink_radius > 0.0 ? p->kink_radius
                   : r->direction == NEO_DIRECTION_STAGEWISE ? NEO_RULE_KINK_RADIUS_STAGEWISE : NEO_RULE_KINK_RADIUS;
  r->hop_min_drop = NEO_RULE_HOP_MIN_DROP * p->opt_tolerance;
  r->scan_resume_gain = NEO_RULE_SCAN_RESUME_GAIN * p->opt_tolerance;
  /* Beyond 3 control steps the objective is flatter per block (the weights are divided by N, and two neighbouring blocks
   * of a long horizon can trade displacement at almost no cost): the gain thresholds of the Newton directions shrink with
   * (3/N)^2, the three-iteration window with (3/N)^3 */
  r->flat = (newton && n > 3) ? (3.0 / n) * (3.0 / n) : 1.0;
  r->ftol = p->cost_tolerance > 0.0 ? p->cost_tolerance : (newton ? 3e-4 * r->flat : 3e-6) * p->opt_tolerance;
  r->wtol = p->window_tolerance > 0.0 ? p->window_tolerance
            : (p->window_tolerance == 0.0 && newton) ? 3e-3 * p->opt_tolerance * r->flat * fmin(1.0, 3.0 / n) : 0.0;
  r->wtol_late = p->window_tolerance > 0.0 ? p->window_tolerance
                 : (p->window_tolerance == 0.0 && newton) ? 3e-3 * p->opt_tolerance : 0.0;
  /* blocked-run rule: dense direction only, part of the window rule (off with it); absolute (a search on its way out of a
   * lethal cell has a huge f), scaled with the horizon like the stall threshold */
  const int blocked = r->direction == NEO_DIRECTION_DENSE && r->wtol > 0.0;
  r->btol_map = blocked ? NEO_RULE_BLOCKED_TOL_MAP * r->flat * p->opt_tolerance : 0.0;
  r->btol_free = blocked ? NEO_RULE_BLOCKED_TOL_FREE * r->flat * p->opt_tolerance : 0.0;
}
static inline void neo_rules_derive(const neo_mpc_params* p, neo_rules* r) { neo_rules_derive_as(p, neo_rules_direction(p), r); }
/* The rules of an instance the routed control_steps-3 kernel sends to the stage-wise direction: that direction's prox-only zone
 * around the kink (it predicts landings inside its sweep), and the control_steps-3 STOP rules of the dense direction -- the
 * window rule on every run of three iterations, the blocked-run rule with its thresholds, closing-in behind two blocked
 * iterations.  What ends a search depends on the horizon, not on how the direction was computed; the stage-wise exceptions
 * (window and closing-in only behind three blocked iterations, no blocked-run rule) exist for long horizons, whose
 * Gauss-Newton steps converge linearly and whose long shots need blocked iterations to leave lethal cells.  Measured on the
 * mirror: the same objective misses against the reference (none in 3660 costmap cases, every fixture gate unchanged), closed
 * loop of 4096 robots: per-tick maximum 15 -> 13 iterations in the median, 21 -> 15 at worst. */
static inline void neo_rules_derive_routed(const neo_mpc_params* p, neo_rules* r) {
  neo_rules dense;
  neo_rules_derive_as(p, NEO_DIRECTION_DENSE, &dense);
  neo_rules_derive_as(p, NEO_DIRECTION_STAGEWISE, r);
  r->btol_map = dense.btol_map;
  r->btol_free = dense.btol_free;
}

/* ---------------------------------------------------------------- the decisions of the search, in plain C: compiled into
 * the device code (k1_solve.h solve_search, every K1 variant) and into the CPU mirror (mpc_oracle.c orc_pg_solve) from this
 * one text.  How each side measures what goes in -- the maximum of |d|, the step taken, the costmap terms under a rollout --
 * is its own business; what follows from the measurements is decided here. */
#if defined(__HIPCC__)
#define NEO_RULES_FN __host__ __device__ static inline
#else
#define NEO_RULES_FN static inline
#endif

/* ---- damping of the stage-wise direction beyond 8 control steps (Levenberg-Marquardt mu, start value mu0) */
#define NEO_RULE_DAMP_RELAX_STEP 0.8    /* an iteration won by a Newton step of at least this length relaxes the damping ... */
#define NEO_RULE_DAMP_RELAX 0.25        /* ... by this factor */
#define NEO_RULE_DAMP_TIGHTEN_STEP 0.3  /* one won by a proximal lane or by a Newton step shorter than this tightens it ... */
#define NEO_RULE_DAMP_TIGHTEN 4.0       /* ... by this factor */
#define NEO_RULE_DAMP_RANGE 16.0        /* mu stays within [mu0 / this, mu0 x this] */

/* The stop tolerances as a search reads them: a block of doubles -- the head of K1's tolerance block in LDS (solver_context.h;
 * read where a rule needs one: as arguments they were all loaded up front and cost the kernels registers), an array in the mirror. */
enum { NEO_TOL_XTOL, NEO_TOL_EARLY, NEO_TOL_FINAL, NEO_TOL_FTOL, NEO_TOL_STALL, NEO_TOL_WTOL, NEO_TOL_WTOL_LATE,
       NEO_TOL_BTOL_MAP, NEO_TOL_BTOL_FREE, NEO_TOL_COUNT };
static inline void neo_rules_stop_tolerances(const neo_rules* r, double* tol) {
  tol[NEO_TOL_XTOL] = r->xtol; tol[NEO_TOL_EARLY] = r->xtol; tol[NEO_TOL_FINAL] = r->final_tol; tol[NEO_TOL_FTOL] = r->ftol;
  tol[NEO_TOL_STALL] = r->stall_step; tol[NEO_TOL_WTOL] = r->wtol; tol[NEO_TOL_WTOL_LATE] = r->wtol_late;
  tol[NEO_TOL_BTOL_MAP] = r->btol_map; tol[NEO_TOL_BTOL_FREE] = r->btol_free;
}

/* What a search carries from one iteration to the next about how it is doing. */
typedef struct neo_search_run {
  int stall;            /* consecutive iterations gaining < ftol (relative) or moving < stall_step */
  int blocked_run;      /* consecutive iterations not won by a Newton step of at least NEO_RULE_BLOCKED_STEP */
  int nblocked;         /* consecutive iterations not won by a Newton step of at least NEO_RULE_WINDOW_STEP (or won by a hop) */
  double gain1, gain2;  /* objective decrease of the previous two iterations */
  bool final_step;      /* the step test has announced this iteration as the last */
} neo_search_run;
/* at the start of a search, and again behind a cell scan that paid (the search is taken up from a new point) */
NEO_RULES_FN void neo_search_run_init(neo_search_run* s) {
  s->stall = 0; s->blocked_run = 0; s->nblocked = 1; s->final_step = false;
  s->gain1 = INFINITY; s->gain2 = INFINITY;
}

/* The Newton step test in front of the candidate pass (second-order directions, not in the first iteration).  dm: the
 * largest entry of the full step d; near_any: a block hovers next to the control norm's kink -- the prox step moves it, which d
 * does not describe; nhops: hop candidates of this iteration; gauss_newton: d carries no second-order terms of the rollout. */
enum { NEO_STEP_GOES_ON = 0, NEO_STEP_IS_LAST = 1, NEO_STEP_CONVERGED = 2 };
NEO_RULES_FN int neo_rules_step_test(double dm, int near_any, int nhops, double early_tol, double final_tol, int gauss_newton) {
  /* the full Newton step is already below the step tolerance: u is the answer
   * (with a cheaper cell a hop away the search runs once more: its hop lanes decide) */
  if (dm < early_tol && !near_any && nhops == 0) return NEO_STEP_CONVERGED;
  /* a full Newton step below opt_tolerance (SLSQP's own step test) is the last one: searched and taken like any other, but
   * nothing re-checks the point it lands on (the error left is of the order of the step squared)
   * (a Gauss-Newton step converges linearly: it has to be shorter to be the last) */
  if (dm < (gauss_newton ? NEO_RULE_FINAL_FRAC_GN : 1.0) * final_tol && !near_any) return NEO_STEP_IS_LAST;
  return NEO_STEP_GOES_ON;
}

/* Does the iteration that has just taken its winner end the search?  Updates *s.
 * The kind of search -- stagewise: the stage-wise direction; routed: ... with the control_steps-3 stop rules of the dense
 * direction (neo_rules_derive_routed); blocked_rule: the blocked-run rule is on (dense direction, routed searches).
 * tol: the stop tolerances (NEO_TOL_*).  The iteration -- newton_won: a lane of the second-order direction (32-63) won, with the
 * step length won_step; hop_won: a hop candidate or the un-shifted start won; gain: f - fb; fb: the objective of the new iterate
 * WITHOUT its constant terms; stepmax: the largest change of a control; free_now: the closing-in rule's free space (dense
 * direction: no costmap term under the NEW iterate's rollout; stage-wise: under the rollout the iteration started from);
 * free_rollout: no costmap term under the new iterate's rollout (read by the blocked-run rule only). */
NEO_RULES_FN int neo_rules_iteration_ends(int stagewise, int routed, int blocked_rule, const double* tol, neo_search_run* s, int it,
                                          int newton_won, double won_step, int hop_won, double gain, double fb, double stepmax,
                                          int free_now, int free_rollout) {
  /* (gain thresholds are relative to the u-dependent part of the objective: the constant terms -- the terminal distance term,
   * py:266 -- can be 20 x the rest) */
  const double fscale = fmax(1.0, fabs(fb));
  /* iterations that gain next to nothing or barely move (creeping along a costmap cell edge, the slow tail next to the
   * control norm's kink) end the search once NEO_RULE_STALL_ITERATIONS of them are in a row */
  s->stall = (gain <= tol[NEO_TOL_FTOL] * fscale || stepmax <= tol[NEO_TOL_STALL]) ? s->stall + 1 : 0;
  /* stage-wise direction: the window and closing-in rules only judge runs of BLOCKED iterations (none of the three won
   * by a Newton step of at least half its length); iterations won by the Newton step end through the step test
   * (the un-shifted start that won the first iteration says as little about step lengths as a hop) */
  s->nblocked = (!newton_won || won_step < NEO_RULE_WINDOW_STEP || hop_won) ? s->nblocked + 1 : 0;
  const int window_on = !stagewise || routed || s->nblocked >= 3;
  /* three iterations that together gained less than wtol: creeping along a costmap cell edge
   * (from NEO_RULE_LATE_ITERATION on the window is the control_steps-3 one again: a long-horizon search that has run twice
   * its usual length is creeping, gaining 1e-8 of f per iteration up to the iteration cap -- a handful per 65 536 solves, but
   * a launch lasts as long as its slowest wave) */
  const double wtol0 = tol[NEO_TOL_WTOL];   /* (the closing-in rule below is on whenever the window rule is) */
  const double wtol = it >= NEO_RULE_LATE_ITERATION ? tol[NEO_TOL_WTOL_LATE] : wtol0;
  const double g1 = s->gain1, g2 = s->gain2;
  int creeping = wtol > 0.0 && gain + g1 + g2 <= wtol * fscale && window_on;
  /* ... and so does a step below stall_step whose gain halved twice in a row: the search is closing in on a costmap cell
   * edge (or the kink) geometrically; what is left to gain is less than the last gain.  -3 % iterations at control_steps 3 and
   * 32, no command moves by 1e-3.  In free space three gains it takes (round 5: the INFINITY the two older ones start at used
   * to pass for a gain, and a warm search that began next to the kink ended after its second iteration, 2.4e-3 from the
   * reference's converged first control on one G13 tick), and the geometric series the gains start has to be worth less than
   * the stall threshold, gain r / (1 - r) <= ftol f~ with r = gain / gain1: the rule ended warm searches whose gains fell by
   * a sixth per iteration with 3e-6 left to gain, which is 2.5e-3 in the first control along a direction of curvature 1.
   * (dense and L-BFGS directions, routed searches: only behind NEO_RULE_CLOSING_RUN blocked iterations -- the gains of a Newton
   * search that converges quadratically halve twice in a row as well, and one blocked iteration after them, a bound about to
   * become active, is no sign of creeping: random parameter sets, 1 solve in 3000 stopped 5e-3 short)
   * (free_now: where the first control is gated, not only the objective) */
  creeping = creeping || (wtol0 > 0.0 && stepmax <= tol[NEO_TOL_STALL] && gain <= 0.5 * g1 && g1 <= 0.5 * g2 &&
                          (!free_now || (g2 < INFINITY && gain * gain <= tol[NEO_TOL_FTOL] * fscale * (g1 - gain))) &&
                          ((stagewise && !routed) ? window_on : s->nblocked >= NEO_RULE_CLOSING_RUN));
  /* Blocked-run rule.  NEO_RULE_BLOCKED_RUN iterations in a row not won by a decent Newton step that together gain less
   * than 0.1 x opt_tolerance (0.03 x with no costmap term under the new iterate's rollout): something the quadratic model
   * does not see is in the way -- a costmap cell edge, or blocks hovering next to the control norm's kink -- and the search
   * advances 1e-6 of f per iteration (SLSQP stops on ONE iteration gaining less than opt_tolerance).  In a closed 30 Hz loop of
   * 4096 robots such searches set the duration of every launch: per-tick maximum 25 -> 13 iterations in the median, 100 -> 16
   * at worst; cold solves and the zero-map drift check are untouched (4096 cold C2 solves: no objective more than 9e-6 higher;
   * 8192 zero-map problems against solves run to the end: unchanged, max 5.8e-4).  Absolute, not scaled by |f|: f is
   * dominated by the lethal term while a search is on its way out of a lethal cell.  A stage-wise search that is not routed does
   * not take it: its wall model and hop candidates deal with cell edges, and its long shots need their blocked iterations to
   * get out of lethal cells. */
  int blocked_stop = 0;
  if (blocked_rule) {
    s->blocked_run = (!newton_won || won_step < NEO_RULE_BLOCKED_STEP) ? s->blocked_run + 1 : 0;
    if (s->blocked_run >= NEO_RULE_BLOCKED_RUN)   /* (a tolerance of 0: the rule is off -- a gain is never <= 0 here) */
      blocked_stop = gain + g1 + g2 <= (free_rollout ? tol[NEO_TOL_BTOL_FREE] : tol[NEO_TOL_BTOL_MAP]);
  }
  s->gain2 = g1; s->gain1 = gain;
  /* the last-step rule rests on the Newton model having held: an iteration announced as the last but WON by a proximal
   * step, a hop or a short Newton step (a bound about to become active, the kink) is not the last */
  if (s->nblocked != 0) s->final_step = false;
  return stepmax < tol[NEO_TOL_XTOL] || s->stall >= NEO_RULE_STALL_ITERATIONS || creeping || s->final_step || blocked_stop;
}

#endif /* NEO_MPC_SOLVER_RULES_H_ */
