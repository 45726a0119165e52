/*
 * neo_mpc.h -- C-ABI of the MI355X-native batched MPC solver (libneo_mpc.so).
 *
 * Drop-in boundary for the optimisation inner loop of neobotix/neo_mpc_planner2.
 * The entry points below are what `NeoMpcPlanner::computeVelocityCommands`
 * (src/NeoMpcPlanner.cpp:240-252) binds INSTEAD of the blocking ROS2 service call
 * to the Python node: one `neo_mpc_problem` carries exactly the fields of the
 * `neo_srvs2/srv/Optimizer` request built at cpp:240-246, one `neo_mpc_command`
 * the `output_vel` returned at cpp:250-252, `neo_mpc_params` the ROS parameters the
 * node declares at neo_mpc_planner2/mpc_optimization_server.py:49-75, and
 * `neo_mpc_state` the state the node keeps between calls (py:115-152).
 *
 * Conventions: plain C, no exceptions; every call returns NEO_MPC_OK (0) or a
 * negative NEO_MPC_ERR_* code and `neo_mpc_last_error()` describes the failure;
 * the library never retains caller pointers after a call returns; a handle is NOT
 * thread-safe (the plugin already serialises under `mutex_`, cpp:207), distinct
 * handles are independent.  There is no CPU fallback: `neo_mpc_create` fails when
 * no gfx950 device is visible.
 */
#ifndef NEO_MPC_H_
#define NEO_MPC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NEO_MPC_ABI_VERSION 2
/* ABI 2 (round 4): neo_mpc_behaviour_version(); NEO_MPC_COMPAT_REFERENCE_START; unknown compat bits and the forced
 * directions without a wall model at a heavy costmap weight are refused; neo_mpc_problem.skip (was reserved[0]) and
 * NEO_MPC_FLAG_SKIPPED; neo_mpc_carrot.status 3.  No record changed its size or the offset of a field that existed.
 * Round 5 added entry points only (neo_mpc_effective_method, neo_mpc_balance_dispatch_device) and gave the last 28 bytes
 * of neo_mpc_state, reserved until then, a meaning (has_prev_u0, prev_u0): still ABI 2.
 * The footprint gate (neo_mpc_footprint_batch, neo_mpc_footprint_gate, neo_mpc_footprint_gate_device) added a record and two
 * entry points; no existing record, entry point or result changed: still ABI 2, behaviour 6.
 * The rolling windows (neo_mpc_window_batch, neo_mpc_set_world_map[_device], neo_mpc_roll_costmap_pool[_device],
 * neo_mpc_get_costmap_pool) added a record and five entry points in the same way: still ABI 2, behaviour 6.
 * The fleet stamp (neo_mpc_stamp_batch, neo_mpc_stamp_fleet[_device], neo_mpc_inflation_costs) added a record and three
 * entry points in the same way: still ABI 2, behaviour 6.
 * The grid planner (neo_mpc_replan_batch, neo_mpc_replan, neo_mpc_replan_plans[_device]) added two records and two entry
 * points in the same way: still ABI 2, behaviour 6.
 * The world inflation (neo_mpc_inflate_world_map[_device], neo_mpc_get_world_map) added three entry points and no record:
 * still ABI 2, behaviour 6.
 * The scan obstacle layer (neo_mpc_scan_batch, neo_mpc_update_scan_layer[_device], neo_mpc_get_scan_layer,
 * neo_mpc_reset_scan_layer, NEO_MPC_MAX_SCAN_POINTS) added a record, four entry points and a constant in the same way: still
 * ABI 2, behaviour 6.
 * The laser projection (neo_mpc_scanner, neo_mpc_laser_batch, neo_mpc_laser_beam_table, neo_mpc_project_laser[_device],
 * neo_mpc_update_scan_layer_from_ranges[_device], NEO_MPC_MAX_SCAN_SOURCES, NEO_MPC_LASER_INF_IS_VALID) added two records,
 * five entry points and two constants in the same way: still ABI 2, behaviour 6.
 * The speckle filter of the world scan layer (neo_mpc_set_world_scan_denoise, neo_mpc_get_world_scan_denoised,
 * NEO_MPC_MAX_DENOISE_GROUP) added two entry points and a constant and no record: still ABI 2, behaviour 6.
 * The decay of the world scan layer's old marks (neo_mpc_set_world_scan_decay, neo_mpc_get_world_scan_ages, NEO_MPC_NO_AGE)
 * added two entry points and a constant and no record: still ABI 2, behaviour 6.
 * The plan check (neo_mpc_plan_check_batch, neo_mpc_plan_check, neo_mpc_check_plans[_device]) added two records and two
 * entry points in the same way: still ABI 2, behaviour 6.
 * The read-back of the dispatch order (neo_mpc_get_dispatch_order, a test hook) added an entry point only: still ABI 2,
 * behaviour 6.
 *
 * Behaviour history (iterates and iteration counts differ between versions, results stay inside the parity protocol of
 * DESIGN.md section 1; neo_mpc_behaviour_version() returns the number of the build that answers):
 *   1  AUTO = dense Newton up to 8 control steps, L-BFGS beyond.
 *   2  AUTO = dense Newton at control_steps 3, the stage-wise (Riccati) direction everywhere else -- and at 3 when
 *      w_costmap > w_trans / 4; stop thresholds beyond 3 control steps scaled with (3 / control_steps)^2.
 *   3  hop candidates in the stage-wise direction; blocked-run stop rule in the dense direction; searches on free space
 *      start from the better of the warm start and the warm start un-shifted; page-locked host batches are worked on in
 *      place (neo_mpc_solve_batch); neo_mpc_pin_host_memory, neo_mpc_set_host_path; neo_mpc_solve_batch_begin / _wait.
 *   4  the stage-wise direction carries the second-order terms of the rollout step (exact Hessian) behind an iteration
 *      won by a Newton step; its window rules judge runs of blocked iterations only; gain thresholds relative to the
 *      u-dependent part of the objective; blocks next to the control norm's kink take their proximal step on their face
 *      and sit every other Newton candidate out; a block sliding along a box bound stops at the disc corner; the dense
 *      direction tries a hop to a cheaper costmap cell where its search is about to end; state records are written back
 *      field by field (old_goal only when it changed).  Blocks in a corner of the feasible set that a Newton step sends
 *      outward are pinned and the direction is computed once more; the closing-in stop rule of the dense / L-BFGS
 *      directions waits for two blocked iterations; a step below opt_tolerance ends the search only if it won its iteration.
 *   5  (round 5) cell scan in place of the dense direction's exit hop, in both second-order directions: a search that has
 *      ended looks at the costmap cells around every stage (up to 3 cells away, inside the reach of a feasible rollout),
 *      evaluates the cheapest ones as candidates and is taken up again once when that gained more than opt_tolerance.
 *      The warm start is un-shifted with the previous solve's own first block (neo_mpc_state.prev_u0, was reserved); on a
 *      costmap the un-shifted point is a candidate of the first iteration instead of a starting point.  Closing-in stop
 *      rule, in free space: three real gains and a geometric estimate of what is left below the stall threshold.  A
 *      pinned LBFGS / NEWTON direction that a neo_mpc_set_params call takes across w_costmap = w_trans / 4 runs the
 *      stage-wise direction from there on (neo_mpc_effective_method) instead of failing the reconfigure; neo_mpc_create
 *      still refuses the combination.  neo_mpc_problem.skip: host batches with values other than 0 / 1 are refused.
 *   6  (round 6) AUTO at control_steps 3 (below w_costmap = w_trans / 4): DIRECTION BY NEIGHBOURHOOD.  An instance with a
 *      lethal cell (raw 254, or the outside of the map) among the cells of its reach tile -- NEO_MPC_FLAG_WALL_IN_REACH says
 *      so in its command -- is solved by the stage-wise direction (wall model, hop candidates; with the control_steps-3
 *      stop rules), every other instance by the dense direction as before; one launch, one kernel (k_solve_routed).  The
 *      dense direction has no wall model: every objective miss of random-parameter runs against the reference at
 *      control_steps 3 was a dense search hemmed in by lethal cells.  method = NEO_MPC_METHOD_NEWTON is the dense direction
 *      for every instance (version 5's AUTO at control_steps 3).
 * method = NEO_MPC_METHOD_NEWTON / _LBFGS / _RICCATI pins a direction. */
#define NEO_MPC_BEHAVIOUR_VERSION 6

/* return codes */
#define NEO_MPC_OK 0
#define NEO_MPC_ERR_INVALID_ARGUMENT (-1)
#define NEO_MPC_ERR_NO_DEVICE (-2)
#define NEO_MPC_ERR_DEVICE (-3)      /* a HIP runtime call failed */
#define NEO_MPC_ERR_NO_COSTMAP (-4)  /* solve before set_costmap */
#define NEO_MPC_ERR_UNSUPPORTED (-5)

/* per-instance solver status (neo_mpc_command.status); 0 <=> SciPy's `x.success` (py:397) */
#define NEO_MPC_STATUS_CONVERGED 0
#define NEO_MPC_STATUS_MAX_ITER 1

/* neo_mpc_command.flags */
#define NEO_MPC_FLAG_RESET 1   /* new goal: warm start / last_control / waiting_time reset (py:358-361) */
#define NEO_MPC_FLAG_STOPPED 2 /* zero twist because of the collision latch (py:374-377) */
#define NEO_MPC_FLAG_SKIPPED 4 /* neo_mpc_problem.skip was set: no request was made for this robot this tick (cpp:234-236).
                                  Its state record and warm start have not been touched; the command is zero twist with this
                                  flag alone, its rows of solution / predicted_path / velocities are zero */
#define NEO_MPC_FLAG_WALL_IN_REACH 8 /* a lethal cell (raw 254) -- or the outside of the map -- lies within the cells a feasible
                                  rollout of this robot can reach (the solver's reach tile; always set when the reach is too
                                  long for a tile).  Under NEO_MPC_METHOD_AUTO at control_steps 3 such an instance was solved
                                  by the stage-wise direction, every other one by the dense direction */

/* neo_mpc_params.compat_flags */
#define NEO_MPC_COMPAT_ODOM_YAW_GOAL_W 1 /* py:213: odom_yaw takes quaternion w from the goal pose */
#define NEO_MPC_COMPAT_REFERENCE_START 2 /* every search starts at the reference's starting point: the warm start as
                                            py:397-400 / 198-202 left it (projected onto the feasible set, like SciPy clips
                                            x0).  Without it (default) a search on free space starts from the better of that
                                            and the same sequence with the whole-step shift undone -- fewer iterations per
                                            warm tick, same objective */
#define NEO_MPC_COMPAT_ALL (NEO_MPC_COMPAT_ODOM_YAW_GOAL_W | NEO_MPC_COMPAT_REFERENCE_START) /* any other bit: INVALID_ARGUMENT */

/* neo_mpc_params.method */
#define NEO_MPC_METHOD_AUTO 0   /* control_steps == 3: by neighbourhood -- dense Newton (the register-resident 9 x 9
                                   system) for an instance with no lethal cell in reach, stage-wise (Riccati) Newton
                                   for one next to a wall (NEO_MPC_FLAG_WALL_IN_REACH), in one launch; stage-wise
                                   Newton at every other control_steps -- and for every instance at 3 when
                                   w_costmap > w_trans / 4 (cost steps become walls: the wall model is part
                                   of the stage-wise direction) */
#define NEO_MPC_METHOD_LBFGS 1  /* projected L-BFGS, any control_steps */
#define NEO_MPC_METHOD_NEWTON 2 /* projected Newton (finite-difference Hessian of the analytic
                                   gradient, one column per lane); control_steps <= 8 */
/* (LBFGS and NEWTON have no wall model for costmap steps: with w_costmap > w_trans / 4 -- where AUTO hands every
 * control_steps to the stage-wise direction -- they end above the reference's SLSQP on a few percent of the costmap cases
 * (G8 "turn", G9), so neo_mpc_create refuses that combination with NEO_MPC_ERR_UNSUPPORTED; a LIVE handle reconfigured
 * across the threshold (neo_mpc_set_params = cb_params, which cannot fail in the reference) keeps working: it runs the
 * stage-wise direction while the weights stay there -- neo_mpc_get_params still returns the pinned method,
 * neo_mpc_effective_method what runs) */
#define NEO_MPC_METHOD_RICCATI 3 /* projected Gauss-Newton, solved stage by stage (Riccati recursion over the
                                   rollout chain, 3x3 blocks, float32): any control_steps, O(control_steps)
                                   per iteration; beyond 8 control steps with adaptive Levenberg-Marquardt
                                   damping; in free space (no costmap term under the rollout) the full
                                   step is tried on its own before the 64-candidate search */
#define NEO_MPC_NEWTON_MAX_CONTROL_STEPS 8

#define NEO_MPC_MAX_CONTROL_STEPS 64
#define NEO_MPC_MAX_FOOTPRINT_POINTS 16
#define NEO_MPC_MAX_LBFGS_MEMORY 8

/* ROS parameters of the reference node, same names (py:49-75; README.md:53-84), then
 * this build's solver options. */
typedef struct neo_mpc_params {
  double acc_x_limit, acc_y_limit, acc_theta_limit;          /* post-clamp py:385-391 */
  double min_vel_x, min_vel_y, min_vel_trans, min_vel_theta; /* box bounds py:127-133 (min_vel_trans unused) */
  double max_vel_x, max_vel_y, max_vel_trans, max_vel_theta; /* max_vel_trans: disc constraint py:157-158 */
  double w_trans, w_orient, w_control, w_terminal;           /* py:252-253, 268 */
  double w_costmap, w_footprint;                             /* py:260, 263 */
  double waiting_time;                                       /* py:70 (initial value only, see py:361, 380) */
  double low_pass_gain;                                      /* py:367 */
  double opt_tolerance;                                      /* py:364 (SLSQP ftol) */
  double prediction_horizon;                                 /* py:137 */
  int32_t control_steps;                                     /* py:75 */
  /* --- build-specific --- */
  int32_t max_iterations; /* <=0: 100, SciPy SLSQP's maxiter */
  int32_t lbfgs_memory;   /* <=0: 4 */
  int32_t compat_flags;   /* NEO_MPC_COMPAT_*; neo_mpc_default_params sets NEO_MPC_COMPAT_ODOM_YAW_GOAL_W (the reference's
                             objective); bits outside NEO_MPC_COMPAT_ALL are refused */
  double step_tolerance;  /* stop when max|du| < this; <=0: 1e-3 * opt_tolerance, and (Newton) a full step
                             shorter than opt_tolerance -- SLSQP's step test -- is taken as the last one */
  double cost_tolerance;  /* an iteration is "stalled" when it lowers the objective by less than
                             cost_tolerance * max(1, |f|) (<=0: 3e-6 * opt_tolerance with L-BFGS, 3e-4 *
                             opt_tolerance with Newton) or moves less
                             than stall_step; 5 stalled iterations in a row end the search */
  double kink_radius;     /* blocks with |u_i - v_cur| below this are moved by the proximal step of
                             the control norm and kept out of the L-BFGS model; <=0: 3e-3 */
  double stall_step;      /* <=0: 0.3 * opt_tolerance */
  int32_t method;         /* NEO_MPC_METHOD_*: search direction of lanes 32-63 */
  int32_t reserved_i;
  double window_tolerance; /* the search also ends when three iterations in a row lower the objective by
                              less than window_tolerance * max(1, |f|) together (SLSQP ends on ONE
                              iteration gaining less than opt_tolerance); 0: 3e-3 * opt_tolerance with
                              Newton, off with L-BFGS (whose normal progress is that slow); <0: off */
} neo_mpc_params;

/* One Optimizer.srv request (cpp:240-246).  256 bytes. */
typedef struct neo_mpc_problem {
  double cur_xy[2];        /* current_pose.pose.position.{x,y}, costmap global frame (cpp:244) */
  double cur_q[4];         /* current_pose.pose.orientation x,y,z,w */
  double carrot_xy[2];     /* carrot_pose.pose.position.{x,y}, base frame (cpp:242) */
  double carrot_q[4];      /* carrot_pose.pose.orientation x,y,z,w */
  double goal_xyz[3];      /* goal_pose.position (cpp:243) */
  double goal_q[4];        /* goal_pose.orientation x,y,z,w */
  double cur_vel[3];       /* current_vel linear.x, linear.y, angular.z (cpp:241) */
  double control_interval; /* 1/controller_frequency (cpp:246) */
  double delta_t;          /* wall-clock seconds since the previous call (py:369-371) */
  double footprint_cost;   /* normalised getFootprintCost(published footprint) (py:262, 343); used
                              when the batch carries no polygons */
  int32_t map_index;       /* which costmap of a pool this instance lives in (neo_mpc_set_costmap_pool);
                              ignored with a single costmap */
  int32_t switch_opt;      /* request.switch_opt = closer_to_goal (cpp:245); the reference stores it (py:354)
                              and never reads it -- carried so that the record is the request field for field */
  int32_t skip;            /* 1: this robot makes NO request this tick -- the plugin threw before its service call
                              (footprint cost 255, cpp:234-236; neo_mpc_select_carrots sets it with every non-zero carrot
                              status): the solver leaves the robot's state and warm start alone (NEO_MPC_FLAG_SKIPPED).
                              Must be 0 or 1: the host entry points refuse anything else (NEO_MPC_ERR_INVALID_ARGUMENT;
                              the field was reserved[0] in ABI 1), the device entry points act on 1 alone */
  int32_t reserved_i;      /* reserved fields MUST be zero */
  double reserved[5];      /* (never read by the device: a request is 216 bytes on the wire) */
} neo_mpc_problem;

/* State the reference node keeps between requests (py:115-152).  128 bytes.  The warm
 * start (`initial_guess`, py:136) is a separate double[3*control_steps] row per instance. */
typedef struct neo_mpc_state {
  double last_control[3];      /* py:117 */
  double old_goal[7];          /* py:146, 402: position xyz + orientation xyzw */
  double waiting_time;         /* py:103, 361, 378-382 */
  int32_t has_old_goal;        /* 0 before the first call: py:146 compares PoseStamped with Pose */
  int32_t collision;           /* py:148 latch */
  int32_t collision_footprint; /* py:149 */
  int32_t has_prev_u0;         /* (was reserved_i) 1: prev_u0 holds ... */
  double prev_u0[3];           /* (was reserved[3]) ... the previous solve's first control block as the solver left it, before
                                  the low-pass of py:366-367 -- the node has no such attribute: it is the build's own hint
                                  (behaviour version 5), written by every solve / postprocess call and read by the next
                                  solve, which un-shifts the warm start with it.  It never changes
                                  what a result means: the point only competes by objective value; zeros (a fresh or an
                                  ABI-1 caller's record) and garbage are harmless */
} neo_mpc_state;

/* Optimizer.srv response (`output_vel.twist`, py:375-377, 389-391) + diagnostics.  48 bytes. */
typedef struct neo_mpc_command {
  double vel[3];       /* linear.x, linear.y, angular.z */
  double cost;         /* objective at the raw solver output (SciPy `x.fun`) */
  int32_t status;      /* NEO_MPC_STATUS_* */
  int32_t iterations;  /* `x.nit` */
  int32_t evaluations; /* objective evaluations per lane */
  int32_t flags;       /* NEO_MPC_FLAG_* */
} neo_mpc_command;

/* One batch of independent instances.  All pointers are host pointers for
 * neo_mpc_solve_batch / neo_mpc_postprocess_batch and device pointers for the
 * *_device variants.  Optional members may be NULL. */
typedef struct neo_mpc_batch {
  size_t count;
  const neo_mpc_problem* problems; /* [count] */
  neo_mpc_state* states;           /* [count] in/out */
  double* warm_start;              /* [count][3*control_steps] in/out (py:136, 397-400) */
  neo_mpc_command* commands;       /* [count] out */
  double* solution;                /* optional [count][3*control_steps]: raw solver output `x.x`
                                      (out for solve, IN for postprocess) */
  double* predicted_path;          /* optional out [count][control_steps][3]: X, Y, yaw of the
                                      `local_plan` rollout (py:293-306) */
  const double* footprints;        /* optional [count][footprint_points][2]: published footprint
                                      polygon, global frame (py:140-144) */
  uint32_t footprint_points;       /* 0: use problems[i].footprint_cost */
  uint32_t reserved;
  double* velocities;              /* optional out [count][3]: packed copy of commands[i].vel (the
                                      buffer a multi-GPU caller hands to the all-gather) */
} neo_mpc_batch;

/* ---- next row of the path: the carrot (look-ahead) selection that feeds the solver ---------- */

/* `<plugin>.lookahead_dist_*` (cpp:311-322) and the plan cut-off of cpp:78-80. */
typedef struct neo_mpc_lookahead_params {
  double lookahead_dist_min, lookahead_dist_max, lookahead_dist_close_to_goal;
  double max_transform_dist; /* max(size_x, size_y) * resolution / 2 (cpp:79-80) */
} neo_mpc_lookahead_params;

/* Result of transformGlobalPlan + getLookAheadDistance + getLookAheadPoint + the slow_down_
 * update (cpp:66-135, 157-189, 221-232) for one robot.  80 bytes. */
typedef struct neo_mpc_carrot {
  double xy[2];           /* carrot_pose.pose.position, base frame (cpp:214) */
  double q[4];            /* carrot_pose.pose.orientation x,y,z,w, base frame */
  double lookahead_dist;  /* cpp:211 */
  uint32_t begin, end;    /* plan poses [begin, end) were kept (cpp:83-104); the caller erases
                             [0, begin) like cpp:126 */
  int32_t closer_to_goal; /* cpp:95-100 (-> request.switch_opt, cpp:245) */
  int32_t slow_down;      /* slow_down_ after cpp:221-232 */
  int32_t status;         /* 0 ok; 1 plan with zero length (cpp:69-71); 2 nothing left (cpp:130-132); 3 the robot's
                             footprint cost is 255 (cpp:234-236: the plugin throws, no optimizer request is made --
                             carrot and look-ahead distance are filled in as for status 0, slow_down is updated like
                             cpp:221-232 did before the throw, problems[i].skip is set) */
  int32_t reserved;
} neo_mpc_carrot;

/* Ragged batch of global plans.  Poses are planar (x, y, yaw) in the plan frame; `robot_poses`
 * is the robot pose already expressed in that frame (transformPose, cpp:74-77). */
typedef struct neo_mpc_plan_batch {
  size_t count;
  const double* plan_poses;      /* [plan_offsets[count]][3] */
  const uint32_t* plan_offsets;  /* [count + 1] */
  const double* robot_poses;     /* [count][3] */
  const double* footprint_costs; /* [count] footprintCostAtPose on nav2's 0..255 scale (cpp:218) */
  int32_t* slow_down;            /* [count] in/out: slow_down_ (h:162, initially 1) */
  neo_mpc_carrot* carrots;       /* [count] out */
  neo_mpc_problem* problems;     /* optional [count]: carrot_xy / carrot_q are written into the
                                    requests the solver will consume (cpp:242) */
} neo_mpc_plan_batch;

/* ---- the step in front of the carrot: the footprint gate (cpp:218-219) ------------------------- */

/* `collision_checker_->footprintCostAtPose(x, y, yaw, footprint)` (cpp:218-219) for `count` robots on the costmap(s) the
 * handle holds -- nav2's FootprintCollisionChecker<Costmap2D*> (Humble) with nav2_util::LineIterator and
 * Costmap2D::worldToMap, evaluated on the raw cell values:
 *   oriented polygon  P_j = (x + p_j.x cos(yaw) - p_j.y sin(yaw), y + p_j.x sin(yaw) + p_j.y cos(yaw)), float64;
 *   cell of a vertex  off the map when X < origin_x, Y < origin_y or a coordinate is not finite; else
 *                     mx = trunc((X - origin_x) / resolution), my likewise, off the map unless mx < size_x and my < size_y
 *                     (the map's true size -- not the lethal border the device copy carries);
 *   cells of an edge  LineIterator from (x0, y0) to (x1, y1), end points included: with dx = |x1 - x0|, dy = |y1 - y0|,
 *                     sx, sy = +1 / -1 (+1 when equal) and dx >= dy, cell k = 0 .. dx is
 *                     (x0 + sx k, y0 + sy ((dx / 2 + k dy) / dx)) in integer arithmetic (dx = 0: the one cell); dx < dy: the
 *                     same with the axes swapped;
 *   cost of an edge   254 when any of its cells is 254, else the largest raw value among them (which may be 255);
 *   cost of the outline (order-dependent, like nav2's fold)  254 when P_0 is off the map; then with c = 0, for
 *                     j = 0 .. n - 2: 254 when P_(j+1) is off the map; c = max(c, edge(j, j + 1)); 254 when c == 254;
 *                     at the end max(c, edge(n - 1, 0)).  255 comes out when an unknown cell was met before a lethal one
 *                     decided the fold: the plugin throws on 255 (cpp:234-236) and not on 254.
 * This is NOT the py:343 outline cost that neo_mpc_batch.footprints feeds (a different line walk on normalised costs).
 * Pointers are host pointers for neo_mpc_footprint_gate and device pointers for neo_mpc_footprint_gate_device.  64 bytes. */
typedef struct neo_mpc_footprint_batch {
  size_t count;
  const double* footprint;       /* [footprint_points][2] base frame, shared by every robot -- or, with
                                    per_robot_footprints, [count][footprint_points][2] */
  uint32_t footprint_points;     /* 3 .. NEO_MPC_MAX_FOOTPRINT_POINTS */
  uint32_t per_robot_footprints; /* 0: one polygon for all; 1: one per robot; anything else is refused */
  const double* poses;           /* optional [count][3]: x, y, yaw in the costmap's global frame.  NULL: problems[i].cur_xy and
                                    the yaw of problems[i].cur_q (py:176-178) */
  const int32_t* map_indices;    /* optional [count]: which map of a pool.  NULL: problems[i].map_index, or 0 without
                                    `problems`.  Ignored with a single costmap, like neo_mpc_problem.map_index */
  neo_mpc_problem* problems;     /* optional [count] (required when `poses` is NULL): footprint_cost is written as
                                    cost >= 254 ? 1.0 : 0.0; no other byte of the records is touched (`skip` stays
                                    neo_mpc_select_carrots' to set) */
  double* footprint_costs;       /* [count] out: nav2's 0 .. 255 scale -- what neo_mpc_plan_batch.footprint_costs takes */
  double* footprints_out;        /* optional [count][footprint_points][2] out: the oriented polygons, global frame -- what
                                    neo_mpc_batch.footprints takes */
} neo_mpc_footprint_batch;

/* ---- the step in front of the gate: a fleet's rolling windows, cut from one world map (K7) ------------ */

/* nav2 gives each robot a rolling local costmap, and those windows are not independent data: each is the static layer's map
 * re-sampled around its robot (LayeredCostmap::updateMap -> Costmap2D::updateOrigin -> the rolling-window branch of
 * StaticLayer::updateCosts).  A fleet server holds ONE world map; the library keeps a device copy of it
 * (neo_mpc_set_world_map) and cuts `count` windows of one geometry from it where the maps live
 * (neo_mpc_roll_costmap_pool): roll -> gate -> carrots -> solve.  nav2 cannot be built next to this library, so the text
 * below is the contract (tests/rolling_window_reference.py is its executable form).
 *
 * All arithmetic is float64; each + - * / below is ONE correctly rounded operation, evaluated in the order written
 * (nothing is fused into a multiply-add, no division becomes a multiplication by a reciprocal).
 *
 * Moving window k to pose (x, y) -- its origin (ox, oy) is state, in and out (`origins`):
 *   Sx = (size_x - 1 + 0.5) * res                 getSizeInMetersX
 *   nx = x - Sx / 2                               updateMap's new origin
 *   q  = (nx - ox) / res
 *   c  = trunc(q), toward zero                    updateOrigin's static_cast<int>; c = 0 where q is not finite or
 *                                                 |q| >= 2^31 (nav2's conversion is undefined there; the device variant
 *                                                 never looks at a value on the host)
 *   ox <- ox + c * res                            the origin stays on its own lattice: a sub-cell move does not roll
 *   likewise for y with size_y.
 * Filling cell (i, j) of window k from the world map (WSX x WSY cells, resolution wres, origin (wox, woy), same frame as the
 * windows; wres need not equal res):
 *   wx = ox + (i + 0.5) * res, wy = oy + (j + 0.5) * res      mapToWorld
 *   the cell is OUTSIDE when wx < wox or wy < woy              worldToMap's refusal -- not a truncation into cell 0
 *   else qx = (wx - wox) / wres, qy = (wy - woy) / wres, and the cell is outside unless qx < WSX and qy < WSY (compared in
 *   float64, before any conversion); inside, its value is world[trunc(qy)][trunc(qx)]
 *   an outside cell gets `outside_value` (nav2's default_value: 255 with track_unknown_space, else 0).
 * Out of scope: a tf transform between the world map's frame and the windows' (they are one frame); `use_maximum`; further
 * layers (the world map IS the master grid the caller wants sampled, inflation included: a caller that holds a raw occupancy
 * grid gets nav2's inflation from neo_mpc_inflate_world_map below, between neo_mpc_set_world_map and the rolls).  The other robots of the fleet
 * are stamped into the windows by the step behind the roll: neo_mpc_stamp_batch below (K8); what the sensors see, by
 * neo_mpc_scan_batch (K10).
 * Pointers are host pointers for neo_mpc_roll_costmap_pool and device pointers for neo_mpc_roll_costmap_pool_device.
 * 56 bytes. */
typedef struct neo_mpc_window_batch {
  size_t count;                    /* windows = maps of the pool: 1 .. NEO_MPC_MAX_POOL_MAPS (0: nothing happens) */
  uint32_t size_x, size_y;         /* cells of one window */
  double resolution;               /* of the windows */
  const double* poses;             /* optional [count][3]: x, y, yaw -- neo_mpc_footprint_batch.poses' layout, so one array
                                      serves the roll and the gate; the yaw is not read */
  const neo_mpc_problem* problems; /* optional [count], used when `poses` is NULL: window k is centred on problems[k].cur_xy.
                                      Both NULL: the windows stay where `origins` puts them and are filled again (the world
                                      map changed) */
  double* origins;                 /* [count][2] in/out */
  uint32_t outside_value;          /* 0 .. 255 */
  uint32_t reserved;               /* MUST be zero */
} neo_mpc_window_batch;

/* ---- the step behind the roll: the fleet's robots stamped into each other's windows (K8) -------------- */

#define NEO_MPC_MAX_INFLATION_CELLS 64 /* largest R = ceil(inflation_radius / resolution): 1.6 m at 2.5 cm */

/* Inside nav2 a robot sees the others through the obstacle layer and the inflation layer of its own local costmap.  A server
 * that cuts every window from one world map has no such layer, but it holds every pose: neo_mpc_stamp_fleet writes the
 * other robots' outlines into each window as lethal cells with nav2's inflation ring around them, between the roll and the
 * gate: roll -> stamp -> gate -> carrots -> solve.  Windows and robots are one to one, as in the roll: window k of the
 * handle's costmap pool -- the one a roll or neo_mpc_set_costmap_pool left there; its origins, size and resolution `res`
 * are the handle's -- belongs to robot k, and `count` must equal the pool's map count.
 *
 * nav2 cannot be built next to this library, so the text below is the contract (tests/fleet_stamp_reference.py is its
 * executable form).  Of its two halves the COST rule is nav2's InflationLayer::computeCost and its combination rule by
 * transcription; the STAMP rule is this library's own -- it is not nav2's Costmap2D::setConvexPolygonCost, which refuses a
 * polygon with a vertex off the map.  Neither is pinned against nav2 itself: nav2's layers are not available to the tests.
 * Every float64 + - * / below is ONE correctly rounded operation in the order written (nothing fused); nothing else in the
 * contract is floating point.
 *
 * Polygon of robot j: P_j[0 .. n-1] in the windows' global frame, n = footprint_points, convex with an area, either
 * winding.  Either `polygons` [count][n][2], used as they are (the array neo_mpc_footprint_gate writes as footprints_out
 * and neo_mpc_batch.footprints takes), or a base-frame `footprint` (shared, or one per robot) placed at `poses` / `problems`
 * by the device routine of the footprint gate: for the same inputs the gate's footprints_out is bit for bit what is stamped.
 *
 * Stamped cells of robot j on window k's lattice, which continues beyond the window's edges (a robot just outside still
 * inflates into the window): cell (i, l), any integers, has the centre cx = ox_k + (i + 0.5) res, cy = oy_k + (l + 0.5) res
 * and is stamped when that centre is inside or on the polygon: with c_e = (b.x - a.x) (cy - a.y) - (b.y - a.y) (cx - a.x)
 * for the edge e from a = P[e] to b = P[(e + 1) % n], when every c_e >= 0 or every c_e <= 0.  A polygon with a vertex that
 * is not finite stamps nothing.  A polygon whose bounding box lies more than R cells from the window is out of its reach
 * (decided in float64, before any conversion to an integer).
 *
 * Distance: for the window's cell (i, l), n_j = min (i - i')^2 + (l - l')^2 over the stamped cells (i', l') of robot j, an
 * integer, and N = min of n_j over j != k: robot k is never stamped into its own window.
 *
 * Cost, tabulated by squared cell distance: R = ceil(inflation_radius / res); T[0] = 254; for 1 <= n <= R^2 with
 * d = sqrt(n): T[n] = 253 when d res <= inscribed_radius, else (uint8)(252 exp(-cost_scaling_factor (d res -
 * inscribed_radius))).  N > R^2 leaves the cell as it is (nav2's cell_inflation_radius_ cut-off).  T is built on the host
 * with libm (neo_mpc_inflation_costs); the kernel never evaluates exp.
 *
 * Combination (nav2's inflation with inflate_unknown false), c = T[N], old = the cell's value: old == 255 becomes c when
 * c >= 253 and stays 255 otherwise; any other old becomes max(old, c).  The rule is monotone in c and T does not increase,
 * so the result does not depend on the order of the robots.
 *
 * Not touched: the lethal border and the pitch padding of the device maps (they stay 254); `origins`.  Stamps are not
 * undone: the next roll cuts the windows afresh, and on an ingested pool they stay until the pool is set again.
 * Pointers are host pointers for neo_mpc_stamp_fleet and device pointers for neo_mpc_stamp_fleet_device.  80 bytes. */
typedef struct neo_mpc_stamp_batch {
  size_t count;                    /* robots = windows: the pool's map count (0: nothing happens) */
  const double* polygons;          /* optional [count][footprint_points][2], global frame; when given, footprint, poses and
                                      problems are not read */
  const double* footprint;         /* used when `polygons` is NULL: [footprint_points][2] base frame, shared by every robot
                                      -- or, with per_robot_footprints, [count][footprint_points][2] */
  uint32_t footprint_points;       /* 3 .. NEO_MPC_MAX_FOOTPRINT_POINTS */
  uint32_t per_robot_footprints;   /* 0: one footprint for all; 1: one per robot; anything else is refused */
  const double* poses;             /* with `footprint`: optional [count][3] x, y, yaw (the roll's and the gate's array) */
  const neo_mpc_problem* problems; /* with `footprint`, used when `poses` is NULL: cur_xy and the yaw of cur_q */
  double inscribed_radius;         /* m; >= 0, finite */
  double inflation_radius;         /* m; >= 0, finite; R = ceil(inflation_radius / res) <= NEO_MPC_MAX_INFLATION_CELLS */
  double cost_scaling_factor;      /* 1/m; >= 0, finite */
  uint64_t reserved;               /* MUST be zero */
} neo_mpc_stamp_batch;

/* ---- the step between the roll and the stamp: an obstacle layer fed from sensor points (K10) ---------- */

#define NEO_MPC_MAX_SCAN_POINTS 8192u
#define NEO_MPC_SCAN_CLEAR 1u   /* raytrace the layer free from the sensor origin to every point */
#define NEO_MPC_SCAN_MARK  2u   /* mark the points' cells lethal in the layer */

/* What is neither on the world map nor a member of the fleet -- a pallet left in an aisle, a person, another vendor's robot --
 * reaches a window through nav2's obstacle layer.  neo_mpc_update_scan_layer keeps one such layer per window in the handle:
 * it rolls with its window, is cleared along this tick's sensor rays and marked at their end points (nav2 Humble's
 * ObstacleLayer::raytraceFreespace, Costmap2D::raytraceLine, bresenham2D and the marking loop of
 * ObstacleLayer::updateBounds), is combined into the window with updateWithMax and inflated around its own lethal cells
 * with the cost table and combination rule of neo_mpc_stamp_batch.  The tick is roll -> scan (points or ranges) -> stamp ->
 * gate -> carrots -> solve.  The scan step comes BEFORE the stamp: a ray that turns an unknown cell free would otherwise erase a stamp ring that
 * left it at 255.
 *
 * Input: points, not ranges.  nav2's obstacle layer consumes Observations: a sensor origin and a cloud of hit points already
 * in the costmap's global frame; the projection of a LaserScan and the tf transform happen in front of it (laser_geometry,
 * ObservationBuffer).  The record takes the same thing, one observation per robot and tick; LaserScan ranges and several
 * scanners per robot go through neo_mpc_laser_batch (K11, below), which projects them and runs this update over all of
 * them.  Out of scope: a z coordinate (min / max_obstacle_height); observation_persistence (the shared layer's decay, K14, is
 * another thing: step 2b below); footprint_clearing_enabled -- obstacle_min_range is the stand-in for a scanner that sees its
 * own robot.
 *
 * Like neo_mpc_stamp_batch's, the contract is one by transcription: nav2 cannot be built next to this library, so the text
 * below is the contract (tests/scan_layer_reference.py is its executable form).  Neither is pinned against nav2 itself: nav2's
 * layers are not available to the tests.  Everything below is float64 + - * /, one sqrt of an exact integer, comparisons and
 * integer arithmetic; every floating-point operation is ONE correctly rounded operation in the order written (nothing fused,
 * no reciprocal).
 *
 * Window k of the handle's pool has sx x sy cells, resolution res and origin (ox, oy), as the last roll or
 * neo_mpc_set_costmap_pool left them.  `count` must equal the pool's map count.  The layer of window k is a grid of the same
 * size with values in {255, 0, 254} plus an origin (lx, ly).  It is kept by the handle.
 *
 * Reset.  The layer is unknown_value everywhere with (lx, ly) = (ox, oy): on the first update; after
 * neo_mpc_reset_scan_layer; whenever sx, sy, res, the map count or unknown_value differ from the previous update's.  A pool
 * replaced with the same geometry keeps its layers.
 *
 * 1. Roll the layer.  This library's own rule: the layer follows its window instead of recomputing nav2's updateOrigin, so the
 * two cannot drift apart.  qx = (ox - lx) / res, and cx = qx rounded to the nearest integer, ties to even.  If qx is not
 * finite or |qx| >= sx, the whole layer becomes unknown_value.  cy is computed likewise.  New cell (i, l) = old cell
 * (i + cx, l + cy) where that lies inside the grid, else unknown_value.  Then (lx, ly) <- (ox, oy).
 *
 * worldToMap(wx, wy).  It fails when a coordinate is not finite, or wx < ox, or wy < oy.  Else mx = trunc((wx - ox) / res)
 * and my likewise.  It fails unless mx < sx and my < sy, compared in float64 before conversion.
 *
 * cellDistance(d) = (unsigned) max(0.0, ceil(d / res)), compared and clamped in float64 (above at 2^31 - 1, which no grid
 * reaches).
 *
 * 2. Clear (with NEO_MPC_SCAN_CLEAR).  The sensor origin is (sx0, sy0).  If worldToMap of it fails, nothing of this robot is
 * cleared.  Otherwise its cell is (x0, y0).  ex = ox + sx res and ey = oy + sy res.  M = cellDistance(raytrace_max_range) and
 * m = cellDistance(raytrace_min_range).  For every point (wx, wy), skipped when a coordinate is not finite:
 *   1. a = wx - sx0 and b = wy - sy0, once.
 *   2. Four clips in order:
 *        if wx < ox: t = (ox - sx0) / a; wx = ox; wy = sy0 + b t
 *        if wy < oy: t = (oy - sy0) / b; wx = sx0 + a t; wy = oy
 *        if wx > ex: t = (ex - sx0) / a; wx = ex - 0.001; wy = sy0 + b t
 *        if wy > ey: t = (ey - sy0) / b; wx = sx0 + a t; wy = ey - 0.001
 *   3. (x1, y1) = worldToMap of the result.  The point is skipped when it fails.
 *   4. The line walk (raytraceLine): Dx = x1 - x0, Dy = y1 - y0, and dist = sqrt((double)(Dx^2 + Dy^2)) -- the argument of
 *      the square root is the exact integer; nav2 calls hypot here.  If dist < m, nothing is cleared.  If dist > 0:
 *      u0 = (unsigned)(x0 + Dx / dist m) and v0 likewise; else (u0, v0) = (x0, y0).  dx = x1 - u0 and dy = y1 - v0; the
 *      signs are +1 when the difference is > 0, else -1.  scale = dist == 0 ? 1.0 : min(1.0, M / dist).  Major axis:
 *      A = max(|dx|, |dy|) and B is the other; x is the major axis on a tie.  n = min(M, (unsigned)(scale A)).  Start at
 *      (u0, v0) with e = A / 2 (integer division) and repeat n times: clear the cell; step one cell along the major axis;
 *      e += B; if (unsigned)e >= A, step one cell along the minor axis and e -= A.  Then clear the cell reached.
 *      "Clear" means layer cell <- 0.  Every cell the walk touches lies inside the grid.
 *
 * 3. Mark (with NEO_MPC_SCAN_MARK).  It runs after every clear of this update.  For every point, with the original
 * coordinates and skipped when not finite: s = (wx - sx0) (wx - sx0) + (wy - sy0) (wy - sy0).  The point is skipped when
 * s >= obstacle_max_range obstacle_max_range, or s < obstacle_min_range obstacle_min_range, or worldToMap fails.  Else layer
 * cell <- 254.  A sensor origin off the map still marks.
 *
 * 4. Combine into the window (updateWithMax).  For every cell, v = layer value and old = window value.  v == 255 leaves the
 * cell alone.  Else the cell becomes v when old == 255 or old < v.  Consequences: a cleared cell turns an unknown window
 * cell free; with unknown_value 0 every unknown window cell becomes free, as nav2 does without track_unknown_space.
 *
 * 5. Inflate.  Seeds are the layer's cells equal to 254, inside the window only.  R, the table T and the combination are word
 * for word those of neo_mpc_stamp_batch; T comes from neo_mpc_inflation_costs at res.  They are applied to the window values
 * step 4 left.  Stated difference from nav2: the inflation of the world's own walls came with the roll (K9); a cell that
 * step 4 turned from unknown to free does not get that inflation back; nav2 inflates after all layers have merged, so it
 * would give it back.
 *
 * Not touched: the lethal border and pitch padding of the device maps, and the pool's `origins`.  The window part is not
 * undone: the next roll cuts the windows afresh, and the layer persists.
 *
 * Idempotence.  An update repeated with the same batch, with no roll in between, changes neither layer nor pool.
 *
 * flags == 0 is a real use: scans arrive at 10 Hz and ticks run at 30 Hz; a roll cuts the windows afresh, so the layer has to
 * be put into them again on the ticks between scans.
 * Pointers are host pointers for neo_mpc_update_scan_layer and device pointers for neo_mpc_update_scan_layer_device.
 * 104 bytes. */
typedef struct neo_mpc_scan_batch {
  size_t count;                   /* robots = windows: the pool's map count (0: nothing happens) */
  const double* points;           /* [count][max_points][2] hit points, global frame; may be NULL when flags == 0 */
  const uint32_t* point_counts;   /* optional [count]: robot k has point_counts[k] <= max_points points; NULL: max_points each */
  const double* sensor_origins;   /* [count][2] Observation.origin_, global frame; may be NULL when flags == 0 */
  uint32_t max_points;            /* 0 .. NEO_MPC_MAX_SCAN_POINTS */
  uint32_t flags;                 /* NEO_MPC_SCAN_*; 0: no new observation -- the layer is rolled and applied again */
  double obstacle_max_range, obstacle_min_range;   /* m, finite, >= 0 */
  double raytrace_max_range, raytrace_min_range;   /* m, finite, >= 0 */
  double inscribed_radius, inflation_radius, cost_scaling_factor;   /* as neo_mpc_stamp_batch */
  uint32_t unknown_value;         /* the layer's default: 255 (nav2's track_unknown_space) or 0; anything else is refused */
  uint32_t reserved;              /* MUST be zero */
} neo_mpc_scan_batch;

/* ---- the scan step fed from LaserScan ranges, several scanners per robot (K11) ------------------------- */

#define NEO_MPC_MAX_SCAN_SOURCES 4u
#define NEO_MPC_MAX_DENOISE_GROUP 16u /* largest minimal_group_size of neo_mpc_set_world_scan_denoise */
#define NEO_MPC_NO_AGE 0xFFFFFFFFu   /* neo_mpc_get_world_scan_ages: the cell holds no mark */
#define NEO_MPC_LASER_INF_IS_VALID 1u   /* neo_mpc_scanner.flags: a range of +inf is a beam that met nothing (nav2's inf_is_valid) */

/* A fleet server receives sensor_msgs/LaserScan messages, not points: float32 ranges, an angle geometry shared by every
 * scan of a scanner model, one robot pose per scan, and usually two scanners a robot, front and rear.  K11 projects the
 * ranges of every scanner of every robot into global-frame points and sensor origins on the device, and
 * neo_mpc_update_scan_layer_from_ranges runs the update of neo_mpc_scan_batch over all of them: every clear of every
 * scanner first, every mark of every scanner afterwards, as nav2's ObstacleLayer::updateBounds raytraces all clearing
 * observations before it marks any.  Two successive neo_mpc_update_scan_layer calls cannot give that order: the second
 * scanner's rays would erase the cells the first one marked in the same tick.
 *
 * The model is laser_geometry::LaserProjection::projectLaser -- a table of cos / sin per scan geometry, a range valid when
 * range_min <= r < range_max -- and, for +inf, ObstacleLayer::laserScanValidInfCallback.  Like neo_mpc_scan_batch's, the
 * contract is one by transcription: laser_geometry and nav2 cannot be built next to this library, so the text below is the
 * contract (tests/laser_scan_reference.py is its executable form) and neither is pinned against them.  Stated differences
 * from nav2: float64 throughout (nav2's cloud and tf transform are float32); one planar pose per scan -- no per-beam time
 * interpolation as in transformLaserScanToPointCloud, no z coordinate; range_max - 1e-4 is formed in float64.  Every float64
 * + - * / is ONE correctly rounded operation in the order written (nothing fused).
 *
 * A scanner: configuration, shared by the whole fleet.  64 bytes. */
typedef struct neo_mpc_scanner {
  double mount_x, mount_y, mount_yaw;   /* the scanner's pose in the robot's base frame */
  double angle_min, angle_increment;    /* LaserScan's, widened from float32 by the caller */
  double range_min, range_max;          /* LaserScan's: finite, 0 <= range_min <= range_max */
  uint32_t flags;                       /* NEO_MPC_LASER_INF_IS_VALID or 0; other bits are refused */
  uint32_t reserved;                    /* MUST be zero */
} neo_mpc_scanner;

/* Projection of beam i of source (scanner) s of robot k, with the robot at (x_k, y_k, yaw_k):
 *   1. r = (double)ranges[k][s][i].  If r == +inf and the scanner has NEO_MPC_LASER_INF_IS_VALID, r = range_max - 1e-4.
 *   2. The beam is valid iff r >= range_min && r < range_max.  NaN, -inf, and +inf without the flag fail this test.
 *   3. An invalid beam writes the point (NaN, NaN), which steps 2 and 3 of neo_mpc_scan_batch skip.  Nothing is compacted.
 *   4. The beam table, built on the host with libm (neo_mpc_laser_beam_table; the device never evaluates a beam's cos or sin):
 *        a = mount_yaw + (angle_min + (double)i * angle_increment);   Tb[s][i] = (c, sn) = (cos(a), sin(a))
 *   5. Base frame: bx = mount_x + r * c and by = mount_y + r * sn.
 *   6. Global frame, with (S, C) = (sin(yaw_k), cos(yaw_k)) evaluated on the device (the one step that is not pinned to the
 *      bit: the device's sincos is within 1 ulp, exact at yaw 0):
 *        gx = (x_k + bx * C) - by * S;   gy = (y_k + bx * S) + by * C
 *   7. The sensor origin of (k, s) is the same two formulas at (bx, by) = (mount_x, mount_y).
 *
 * The layer update over `sources` scanners: reset, roll (step 1), combine (4) and inflate (5) are neo_mpc_scan_batch's,
 * unchanged.  Step 2 (clear) runs for every source with that source's own origin; a source whose origin fails worldToMap
 * clears nothing.  Step 3 (mark) runs for every source, after every clear of every source; the squared distance of its
 * range test is taken to the point's own source's origin.
 *
 * Pointers: `scanners` is ALWAYS a host pointer and is consumed before the call returns.  The others are host pointers for
 * neo_mpc_project_laser / neo_mpc_update_scan_layer_from_ranges and device pointers for the _device variants; a device
 * `points_out` must be 16-byte aligned.  128 bytes. */
typedef struct neo_mpc_laser_batch {
  size_t count;                      /* robots; for the update: = windows, the pool's map count (0: nothing happens) */
  const float* ranges;               /* [count][sources][beams] LaserScan.ranges as on the wire */
  const double* poses;               /* [count][3] robot x, y, yaw, global frame: the roll's and the gate's array */
  const neo_mpc_scanner* scanners;   /* [sources], host memory */
  uint32_t sources;                  /* 1 .. NEO_MPC_MAX_SCAN_SOURCES */
  uint32_t beams;                    /* >= 1; sources * beams <= NEO_MPC_MAX_SCAN_POINTS */
  double* points_out;                /* [count][sources][beams][2]; the update: optional, NULL = a buffer of the handle's */
  double* origins_out;               /* [count][sources][2]; the update: optional, NULL = a buffer of the handle's */
  uint32_t scan_flags;               /* NEO_MPC_SCAN_*, not 0: a tick without a new scan is neo_mpc_scan_batch's flags == 0 */
  uint32_t unknown_value;            /* as neo_mpc_scan_batch */
  double obstacle_max_range, obstacle_min_range;   /* as neo_mpc_scan_batch */
  double raytrace_max_range, raytrace_min_range;
  double inscribed_radius, inflation_radius, cost_scaling_factor;
  uint64_t reserved;                 /* MUST be zero */
} neo_mpc_laser_batch;

/* ---- one obstacle layer for the whole fleet, on the world map (K12) ------------------------------------ */

/* neo_mpc_update_scan_layer gives every window a layer of its own: what robot A sees never reaches robot B's window, the
 * same pallet is inflated again in every window that overlaps it, and the layers cost two more pools of memory.  A fleet
 * server holds every robot's scans and poses, so it can keep ONE layer on the world map's lattice, feed it from all robots,
 * merge and inflate it into a copy of the world map once per update and let the roll cut the windows from that copy:
 *   world scan (points or ranges) -> roll -> stamp -> gate -> carrots -> solve.
 * The path is additive: the per-window layers (K10, K11) stay as they are and may be used in the same tick, behind the roll.
 *
 * State, kept by the handle next to its world map, on the world map's geometry -- WSX x WSY cells of wres at (wox, woy):
 *   `layer`  values in {255, 0, 254}, persistent; the lattice is fixed, so nothing rolls.  It is unknown_value everywhere on
 *            the first update, after neo_mpc_reset_world_scan_layer, and whenever the world map's size, resolution or origin
 *            or unknown_value differ from the previous update's.  neo_mpc_set_world_map with unchanged geometry keeps it.
 *   `live`   the world map with the layer merged in and inflated.  neo_mpc_roll_costmap_pool[_device] cuts its windows from
 *            `live` while it is VALID and from the world map otherwise.  `live` becomes valid at the end of every update and
 *            invalid with every neo_mpc_set_world_map[_device], neo_mpc_inflate_world_map[_device] and
 *            neo_mpc_reset_world_scan_layer; the next update composes it afresh from the map as it then is, and an update
 *            with flags == 0 is enough for that.  A handle on which no update was ever called behaves bit for bit as before.
 *            neo_mpc_get_world_map keeps returning the static map.
 *
 * An update, over `count` robots (free of the pool's map count; no pool is needed), each step one or more launches on the
 * caller's stream, the launch boundary being the order; no atomics:
 *   1. Clear (with NEO_MPC_SCAN_CLEAR).  Every ray of every source of every robot by step 2 of neo_mpc_scan_batch's contract,
 *      word for word, with the world's geometry in place of the window's: (ox, oy, res, sx, sy) = (wox, woy, wres, WSX, WSY)
 *      in worldToMap, the four clips and cellDistance.  Layer cell <- 0, in place.
 *   2. Mark (with NEO_MPC_SCAN_MARK).  After every clear of every robot, step 3 of that contract on the world's geometry:
 *      layer cell <- 254.  Robot A's mark therefore survives robot B's ray of the same update -- nav2's order for several
 *      observation sources in one costmap.
 *   3. Fleet footprint clearing (with a neo_mpc_fleet_clear record).  The layer is shared, so A's scanner marks B's hull, and
 *      without this step B's own footprint gate would read 254 and abort (cpp:234-236).  After the marks every robot's
 *      outline is set free in the layer -- the fleet form of nav2's footprint_clearing_enabled; the other robots still reach
 *      the windows through neo_mpc_stamp_fleet.  Polygons as in neo_mpc_stamp_batch: `polygons`, or `footprint` placed at
 *      `poses` / `problems` by the device routine of the footprint gate -- for the same inputs the gate's footprints_out is
 *      bit for bit what is cleared.  The rule, float64, ONE correctly rounded operation at a time in the order written
 *      (nothing fused): the world cell (i, l), 0 <= i < WSX, 0 <= l < WSY, has the centre cx = wox + (i + 0.5) wres,
 *      cy = woy + (l + 0.5) wres; for the edge from a = P[e] to b = P[(e + 1) % n]: ex = b.x - a.x, ey = b.y - a.y,
 *      c_e = ex (cy - a.y) - ey (cx - a.x) (neo_mpc_stamp_batch's edge function), L_e = sqrt(ex ex + ey ey).  The cell becomes
 *      0 when every c_e >= -(padding L_e) or every c_e <= padding L_e.  With padding == 0 this is the stamp rule exactly.  A
 *      polygon with a vertex that is not finite clears nothing; cells outside the world do not exist.  For a convex polygon
 *      with an area the cleared cells lie within padding / sin(theta / 2) of its bounding box, theta its sharpest interior
 *      angle: that box is what the device walks.
 *      `padding` is in metres.  It exists because a hit on a hull lies ON the polygon's boundary: the centre of its cell may lie
 *      just outside the polygon while the gate's edge walk crosses that very cell.  Callers want padding >= one cell
 *      diagonal (sqrt(2) wres) plus the scanner's noise.
 *   4. Compose.  live = the world map combined with the layer by step 4 of neo_mpc_scan_batch's contract (updateWithMax: 255
 *      in the layer leaves the cell alone), then inflated around the layer's cells equal to 254 by its step 5, with
 *      R = ceil(inflation_radius / wres) <= NEO_MPC_MAX_INFLATION_CELLS and T from neo_mpc_inflation_costs at wres.  The
 *      stated difference from nav2 carries over: a cell the layer turns from unknown to free does not get the world's own
 *      inflation back.
 * flags == 0 runs steps 3 (if given) and 4 only.  An update repeated with the same inputs changes neither layer nor live --
 * with one exception: with decay on (step 2b), a repeated update with NEO_MPC_SCAN_MARK advances the clock and may expire
 * marks; a repeated flags == 0 update still changes nothing.
 * Out of scope: recomposing only the tiles a scan touched; a z coordinate.
 *
 * Step 2b, Decay (K14; optional, off by default: neo_mpc_set_world_scan_decay).  The lattice is fixed, so a mark stays until a
 * later ray happens to pass through it: a person or a pallet jack marked where no robot looks again, or beyond every
 * raytrace_max_range, is a lethal seed for as long as the handle lives.  With decay on, a mark that no scan has made again for
 * a while goes away -- what nav2 users get from the spatio-temporal voxel layer.  It is NOT nav2's observation_persistence,
 * which keeps observations in a buffer and applies them again.  The library's own rule, by contract and transcription, as
 * step 3 is; integers only.  It runs behind every mark and in front of the footprint clearing.
 *   The unit.  The library has no clock and the records no spare field: age is counted in SCAN UPDATES.  A scan update is an
 *   update, from points or from ranges, with NEO_MPC_SCAN_MARK in its flags and count > 0; flags == 0 and CLEAR-only updates
 *   are none.  A server whose scanners run at 10 Hz and that wants five seconds sets 50.
 *   The state, kept only while decay is on: `stamp`, a uint32_t per world cell, read only under a cell that is 254, and
 *   `clock`, one uint32_t in device memory, the number of scan updates so far -- advanced by device code on the caller's
 *   stream, so that a captured update that is replayed advances it.  Every difference is an unsigned 32-bit subtraction:
 *   wrap-around is harmless.
 *   With A = max_age: a scan update first advances `clock` by one.  Its step 2 writes stamp[cell] = clock wherever it writes
 *   254.  Then, in EVERY update while decay is on -- a flags == 0 update too, so that a lowered max_age acts at once --, a cell
 *   with layer == 254 and clock - stamp >= A becomes unknown_value, in the layer itself: the layer has forgotten the cell, in
 *   `live` the world map shows through and the ring is gone.
 *   So a mark made by scan update n is in the layer after scan updates n .. n + A - 1 and gone after scan update n + A; a
 *   mark that is made again is young again.  A mark that is in the layer when decay comes on -- made with decay off, or
 *   before an off -> on -> off -> on sequence -- counts as made by the last scan update before that: the first update with
 *   decay on fills `stamp` with the clock as it stands.  A layer reset needs nothing: no cell is 254.
 *   Steps 3, 3b and 4 read the layer as decay left it: the survivor of a pair whose partner expired is a lone mark to step 3b.
 * With decay off an update is bit for bit, launch for launch and buffer for buffer what it is without this step.
 *
 * Step 3b, Denoise (K13; optional, off by default: neo_mpc_set_world_scan_denoise).  With one layer for the fleet every
 * robot's false returns land on the same lattice, and each is a 254 seed that step 4 inflates into `live` until some ray
 * happens to clear it.  Modelled on nav2_costmap_2d::DenoiseLayer, which sits behind the obstacle layer and in front of
 * inflation -- the contract by transcription, not pinned against it; integers only.  It runs after every clear, mark and
 * footprint clearing of the update.  With G = minimal_group_size:
 *   The world cell (i, l), 0 <= i < WSX, 0 <= l < WSY, is OCCUPIED when layer[l][i] == 254 or world[l][i] == 254 -- `layer`
 *   as step 3 left it, `world` the static world map the handle holds, the array step 4 reads.  Cells outside the world do not
 *   exist.  Two occupied cells are neighbours when they differ by one in exactly one coordinate (connectivity 4), or by at
 *   most one in each coordinate and are not the same cell (connectivity 8).  A group is a connected component of occupied
 *   cells.
 *   D = layer, except that a cell with layer == 254, world != 254 and a group of fewer than G cells has D = 0: the return
 *   was real enough to count as an observation of that cell, so it is free, as nav2 sets it.
 *   Step 4 then reads D wherever it reads the layer, in updateWithMax and as the inflation seeds.
 *   `layer` itself is NOT changed: a lone mark stays in the layer, and when a later scan marks the cell next to it, both
 *   appear.
 * So a mark that touches a wall of the world map belongs to the wall's group and is kept, and two groups of fewer than G
 * cells each are both dropped however close they lie, unless they are connected.  Stated differences from nav2: the static
 * map is never altered (nav2 filters the master grid and would drop specks of the static map too), and `live` does not get
 * the world's own inflation back under a dropped mark, as in step 4.  With the filter off an update is bit for bit, launch
 * for launch and buffer for buffer what it is without this step.  The device decides a cell's group size without labelling:
 * the occupied cells within G - 1 neighbour steps of it number at least G exactly when its group does, and they lie within
 * G - 1 cells of it.
 *
 * The clear record.  Pointers are host pointers for the synchronous calls and device pointers for the _device variants.
 * 64 bytes. */
typedef struct neo_mpc_fleet_clear {
  size_t count;                    /* robots: must equal the scan or laser batch's count */
  const double* polygons;          /* optional [count][footprint_points][2], global frame; when given, footprint, poses and
                                      problems are not read */
  const double* footprint;         /* used when `polygons` is NULL: [footprint_points][2] base frame, or with
                                      per_robot_footprints [count][footprint_points][2] */
  uint32_t footprint_points;       /* 3 .. NEO_MPC_MAX_FOOTPRINT_POINTS */
  uint32_t per_robot_footprints;   /* 0: one footprint for all; 1: one per robot; anything else is refused */
  const double* poses;             /* with `footprint`: optional [count][3] x, y, yaw */
  const neo_mpc_problem* problems; /* with `footprint`, used when `poses` is NULL: cur_xy and the yaw of cur_q */
  double padding;                  /* m; >= 0, finite */
  uint64_t reserved;               /* MUST be zero */
} neo_mpc_fleet_clear;

/* ---- the fleet's global plans against the live world map: which of them it blocks (K15) ----------------- */

/* The world map -- static map, inflation (K9), the fleet's shared obstacle layer (K12 to K14) -- is the one live picture the
 * fleet server holds, and the global plans are the one input of a tick that never met it: neo_mpc_select_carrots streams them
 * and picks a look-ahead pose without knowing whether the plan behind that pose still exists.  nav2 answers this robot by
 * robot with the planner server's `is_path_valid` service, which the behaviour tree polls to trigger a replan; a server that
 * holds every plan and the live map answers it for the whole fleet in one launch (neo_mpc_check_plans[_device]).  nav2
 * cannot be built next to this library, so the text below is the contract (tests/plan_check_reference.py is its executable
 * form).  Every output is an integer.
 *
 * Which map.  The world map the next roll would read: the composition of the last world-scan update while one is current
 * (see neo_mpc_update_world_scan_layer: `live`), else the handle's copy of the world map; WSX x WSY cells, resolution wres,
 * origin (wox, woy).  Plan poses are in that map's frame.  The rolling windows and what is stamped into them are not looked
 * at: the other robots of the fleet are no obstacles to a plan.
 *
 * For robot i, with np = plan_offsets[i + 1] - plan_offsets[i] poses (x, y, yaw):
 *   np == 0           status 2 (nav2 calls an empty path invalid), begin = end = first_blocked = 0, value = 0.
 *   begin             with `robot_poses`: the plan's closest pose, by neo_mpc_select_carrots' rule to the letter (cpp:83-88:
 *                     the first minimum of the float64 hypot, nav2's min_by -- pose 0 where the first distance is NaN or no
 *                     distance is below infinity); without: 0.
 *   end               max_poses == 0: np; else min(np, begin + max_poses).
 *   value of pose k, point mode (no footprint)  neo_mpc_footprint_batch's vertex rule against the map's true size: off the
 *                     map when X < wox, Y < woy or a coordinate is not finite; else mx = trunc((X - wox) / wres), my
 *                     likewise, off the map unless mx < WSX and my < WSY; off the map the value is `outside_value`, else
 *                     the raw cell world[my][mx].  (nav2's service ignores worldToMap's refusal and reads a cell from
 *                     indices it left unset -- a stale cell; this contract deliberately does not: the caller says what the
 *                     outside of the map is worth.)
 *   value of pose k, footprint mode  neo_mpc_footprint_batch's outline cost -- oriented polygon, LineIterator's cells,
 *                     nav2's order-dependent fold, 254 for any vertex off the map -- of `footprint` at (x, y, yaw) of the
 *                     pose, on the world map.  `outside_value` is not read.
 *   a value v blocks  when v == 255 ? unknown_blocks : v >= max_cost.  max_cost 253 is nav2's rule (inscribed or lethal).
 *   first_blocked     the smallest k in [begin, end) whose value blocks, `end` when none does; status 1 when one does,
 *                     else 0.
 *   value             blocked: the value of pose first_blocked.  Not blocked: the largest value below 255 met over
 *                     [begin, end), 0 when there is none -- how tight a still-valid plan has become.
 * The call writes `results` and nothing else: neo_mpc_problem.skip stays neo_mpc_select_carrots' to set, and what to do about
 * a blocked plan is the caller's decision -- neo_mpc_replan_plans[_device] below takes these records as its mask.
 * Out of scope: replanning (the grid planner below is a call of its own); the rolling windows; one footprint per robot; the arc length to the blocked pose (the caller has
 * the index); neo_mpc_select_carrots or this call inside a closed fleet loop that has no plans.
 * Pointers are host pointers for neo_mpc_check_plans and device pointers for neo_mpc_check_plans_device.  72 bytes. */
typedef struct neo_mpc_plan_check {   /* 24 bytes */
  uint32_t begin, end;      /* poses [begin, end) were checked */
  uint32_t first_blocked;   /* end: none */
  int32_t status;           /* 0 valid; 1 blocked; 2 plan with zero length */
  uint32_t value;           /* 0 .. 255, see above */
  uint32_t reserved;        /* written as 0 */
} neo_mpc_plan_check;

typedef struct neo_mpc_plan_check_batch {
  size_t count;
  const double* plan_poses;      /* [plan_offsets[count]][3]: neo_mpc_plan_batch's ragged layout, so one array serves the */
  const uint32_t* plan_offsets;  /* [count + 1]                carrots and the check; poses in the world map's frame */
  const double* robot_poses;     /* optional [count][3]; NULL: every check starts at pose 0 */
  const double* footprint;       /* optional [footprint_points][2] base frame, shared by the fleet; NULL: point mode */
  uint32_t footprint_points;     /* 0 with a NULL footprint, else 3 .. NEO_MPC_MAX_FOOTPRINT_POINTS */
  uint32_t max_cost;             /* 1 .. 254 */
  uint32_t unknown_blocks;       /* 0 or 1: whether the value 255 blocks */
  uint32_t outside_value;        /* 0 .. 255 */
  uint32_t max_poses;            /* 0: to the plan's end */
  uint32_t reserved;             /* MUST be zero */
  neo_mpc_plan_check* results;   /* [count] out */
} neo_mpc_plan_check_batch;

/* ---- detours for the fleet's blocked plans, searched on the live world map: a grid planner (K16) --------- */

/* The consumer of the plan check's answer: for every robot whose plan the live map blocks, a path from where it stands to a
 * goal the caller chose, searched on the same map, for the whole fleet in one launch (neo_mpc_replan_plans[_device]).
 * nav2's planners (NavFn, Smac) cannot be built next to this library and hold float potentials; this is the library's own
 * rule, in integers alone, and the text below is the contract (tests/grid_planner_reference.py is its executable form).
 * The result is unique by construction -- a shortest-path cost and a walk with a fixed tie rule --, every loop of the kernel
 * is bounded by the window, and a robot's search waits for no other robot's.
 *
 * Which map.  The plan check's exactly: the composition of the last world-scan update while one is current (`live`), else
 * the handle's copy of the world map; WSX x WSY cells, resolution wres, origin (wox, woy).  The rolling windows and the
 * other robots are not looked at.
 *
 * For robot i, starts[i] = (x, y) and goals[i] = (x, y), float64, in that map's frame:
 *   cells             the plan check's point-mode rule gives the start cell s = (sx, sy) and the goal cell g = (gx, gy): off
 *                     the map when X < wox, Y < woy or a coordinate is not finite; else mx = trunc((X - wox) / wres), my
 *                     likewise, off the map unless mx < WSX and my < WSY.
 *   search window     W x W cells, W = `window`: x0 = clamp((sx + gx) / 2 - W / 2, 0, max(WSX - W, 0)) in integer
 *                     division, y0 likewise from sy, gy and WSY; its cells are [x0, x0 + W) x [y0, y0 + W) intersected with
 *                     the map.  Everything outside the window is not traversable.
 *   traversable       a cell with the raw value v: v == 255 ? unknown_cost > 0 : v < max_cost.  Its cost m is unknown_cost
 *                     for 255, else v.  The start cell's own value is never looked at where moves leave it: the robot
 *                     stands there (so s == g is a path of one cell whatever the cell holds).  As a cell another move
 *                     enters or passes, the start cell counts by its value like any other.
 *   moves             8-connected, direction k = 0 .. 7 for E, NE, N, NW, W, SW, S, SE (N: towards larger my).  A move
 *                     a -> b needs b traversable; a diagonal move also needs both cells it passes between -- (bx, ay) and
 *                     (ax, by) -- traversable: no corner is cut.
 *   step(a -> b)      (k odd ? 14 : 10) * (neutral_cost + m(b)), uint32.  The worst path of a window stays below 1.2e8:
 *                     nothing wraps.
 *   potential         G(g) = 0, G(a) = min over the allowed moves a -> b of step(a -> b) + G(b): the cost of the cheapest
 *                     path from a to the goal inside the window.
 *   path              from s, at every cell the allowed move that minimises step + G, the lowest k on a tie, until g.  G
 *                     falls strictly along it: at most W * W cells.
 *   status            the first that applies:
 *                       4  not asked: `checks` was given and checks[i].status != 1
 *                       3  s or g is off the map, or outside the window
 *                       2  the goal cell is not traversable (and is not the start cell)
 *                       1  no path inside the window
 *                       5  a path was found and is longer than max_path_cells
 *                       0  a path was found
 *   length, cost      the path's cells, both ends included, and G(s); both 0 unless status is 0 or 5.
 *   window_x0, _y0    x0, y0; 0 for status 4, and for status 3 where s or g is off the map.
 * Paths have the fixed stride max_path_cells a robot:
 *   path_cells[i][j]  = (mx, my), int32, for j < min(length, max_path_cells).
 *   path_poses[i][j]  = (x, y, yaw), float64, optional: x = wox + (mx + 0.5) * wres as one rounded multiply and one rounded
 *                     add (no fused multiply-add), y likewise; yaw is entry k of the table below for the move that leaves
 *                     cell j (whether or not cell j + 1 is written), the last pose of a path repeats the yaw of the pose
 *                     before it, a path of one cell has yaw 0.  The table, k = 0 .. 7 (k * pi / 4, from k = 5 on
 *                     (k - 8) * pi / 4, as float64):
 *                       0.0, 0.7853981633974483, 1.5707963267948966, 2.356194490192345, 3.141592653589793,
 *                       -2.356194490192345, -1.5707963267948966, -0.7853981633974483
 * Entries beyond a path, and every entry of a robot with another status than 0 or 5, are not written (the host variant
 * leaves the caller's values there).
 * Out of scope: splicing the result into the ragged plan_poses / plan_offsets arrays (the stride is fixed, the caller
 * compacts); a footprint-aware search (inflate with neo_mpc_inflate_world_map and choose max_cost); windows beyond 128
 * cells; smoothing; other robots as obstacles; choosing the goal from the old plan; the call inside a closed fleet loop that
 * has no plans.
 * Pointers are host pointers for neo_mpc_replan_plans and device pointers for neo_mpc_replan_plans_device.  80 bytes. */
typedef struct neo_mpc_replan {   /* 24 bytes */
  int32_t status;                 /* 0 .. 5, see above */
  uint32_t length;                /* cells of the path, both ends included */
  uint32_t cost;                  /* G(s) */
  int32_t window_x0, window_y0;   /* the search window's first cell */
  uint32_t reserved;              /* written as 0 */
} neo_mpc_replan;

typedef struct neo_mpc_replan_batch {
  size_t count;
  const double* starts;              /* [count][2] */
  const double* goals;               /* [count][2] */
  const neo_mpc_plan_check* checks;  /* optional [count]: the plan check's records as a mask; NULL: every robot is asked */
  uint32_t window;                   /* W: 4 .. 128 */
  uint32_t max_cost;                 /* 1 .. 254 */
  uint32_t unknown_cost;             /* 0 .. 252; 0: the value 255 is a wall */
  uint32_t neutral_cost;             /* 1 .. 255 */
  uint32_t max_path_cells;           /* >= 1: the stride of path_cells and path_poses */
  uint32_t reserved;                 /* MUST be zero */
  int32_t* path_cells;               /* [count][max_path_cells][2] out */
  double* path_poses;                /* optional [count][max_path_cells][3] out */
  neo_mpc_replan* results;           /* [count] out */
} neo_mpc_replan_batch;

typedef struct neo_mpc_handle neo_mpc_handle;

/* library / ABI */
int neo_mpc_abi_version(void);
int neo_mpc_behaviour_version(void);   /* NEO_MPC_BEHAVIOUR_VERSION of the library that answers */
const char* neo_mpc_last_error(void);
int neo_mpc_last_error_code(void);     /* the NEO_MPC_ERR_* of the calling thread's last failure (neo_mpc_create returns
                                          NULL and no code) */

/* Fills the defaults the reference node declares (py:49-75) and this build's solver options. */
int neo_mpc_default_params(neo_mpc_params* params);

/* Replaces `MpcOptimizationServer.__init__` (py:45-152) + the service client creation at
 * cpp:308.  `device` is the HIP device ordinal.  NULL on failure.
 * The A/B switches of the measurement tools are environment variables READ HERE, ONCE (never on the solve path; a tool
 * that flips one re-creates its handle): NEO_MPC_SOLVE_WAVES=2|3|4, NEO_MPC_NO_TAME_SPECIALISATION, NEO_MPC_DYNAMIC_LDS (kernel
 * variant), NEO_MPC_NO_CHUNKS (large staged host batches in one piece), NEO_MPC_HOST_PATH=staged|zerocopy|zerocopy_out (what
 * NEO_MPC_HOST_PATH_AUTO means).  None changes a result beyond rounding. */
neo_mpc_handle* neo_mpc_create(const neo_mpc_params* params, int device);
void neo_mpc_destroy(neo_mpc_handle* handle);

/* Dynamic reconfigure (`cb_params`, py:405-439).  Unlike the reference every field takes effect. */
int neo_mpc_set_params(neo_mpc_handle* handle, const neo_mpc_params* params);
int neo_mpc_get_params(const neo_mpc_handle* handle, neo_mpc_params* params);
/* (Cloning a live handle -- another GPU of a fleet server: neo_mpc_get_params returns what the caller SET, which may be a
 * pinned LBFGS / NEWTON that a later reconfigure took across w_costmap = w_trans / 4 -- a combination neo_mpc_create refuses.
 * Create the sibling with `method` = neo_mpc_effective_method(handle): that is the direction the live handle runs.) */
/* The direction the handle's solves run: NEO_MPC_METHOD_LBFGS / _NEWTON / _RICCATI (never AUTO) -- what AUTO resolved to,
 * or the stage-wise direction in place of a pinned LBFGS / NEWTON above w_costmap = w_trans / 4 (see NEO_MPC_METHOD_*);
 * < 0 on a null handle.  AUTO at control_steps 3 below that threshold decides per instance (behaviour 6): NEWTON is the
 * answer -- the direction of the instances with no wall in reach; those with NEO_MPC_FLAG_WALL_IN_REACH in their command ran
 * the stage-wise one. */
int neo_mpc_effective_method(const neo_mpc_handle* handle);

/* Replaces the node's `Costmap2d(self)` subscription (py:118): raw nav2 costs, row-major
 * cells[my*size_x + mx] (e.g. `costmap_->getCharMap()` in the plugin).  The data is copied before the
 * call returns; the device-side ingest is left in flight, ordered in front of every later call on
 * this handle (the *_device entry points wait for it on the caller's stream).
 * Stream ordering, all set_costmap* variants: the ingest records an event on the stream it ran on and every
 * solve / postprocess / objective entry point makes its own stream wait for it; every solve records an event
 * on its stream and the next ingest waits for it before it rewrites the device map -- a solve never sees a
 * half-written map whatever streams the caller mixes.  (The caller's own buffers -- `d_cells`, `d_origins`,
 * the batch arrays -- stay the caller's to order.)  The two small tables every wave reads as it starts -- the pool's origins
 * (neo_mpc_set_costmap_pool) and the per-step costmap terms (neo_mpc_set_params) -- are rewritten only after every launch
 * that may still read them has ended (a host-side wait): both calls are safe between neo_mpc_solve_batch_begin and _wait. */
int neo_mpc_set_costmap(neo_mpc_handle* handle, const uint8_t* cells, uint32_t size_x,
                        uint32_t size_y, double resolution, double origin_x, double origin_y);
/* Same, `d_cells` already in device memory; ingested on `stream` (hipStream_t, may be NULL). */
int neo_mpc_set_costmap_device(neo_mpc_handle* handle, const uint8_t* d_cells, uint32_t size_x,
                               uint32_t size_y, double resolution, double origin_x,
                               double origin_y, void* stream);

/* Fleet variant of neo_mpc_set_costmap: `count` costmaps of one size and resolution -- nav2's rolling
 * local costmaps, one per robot or per group of robots -- stored back to back (map k at
 * cells + k*size_x*size_y), origins[2k], origins[2k+1] = origin of map k.  Every instance reads the map
 * its `neo_mpc_problem.map_index` names.  Replaces whatever costmap(s) the handle held. */
#define NEO_MPC_MAX_POOL_MAPS 65535u /* one ingest launch: the map index is the grid's y coordinate */
int neo_mpc_set_costmap_pool(neo_mpc_handle* handle, const uint8_t* cells, uint32_t count, uint32_t size_x,
                             uint32_t size_y, double resolution, const double* origins);
/* Same with `d_cells` and `d_origins` in device memory; the ingest runs on `stream`.  `d_origins` is read
 * by every later solve: it must stay valid (and may be rewritten by the caller between ticks). */
int neo_mpc_set_costmap_pool_device(neo_mpc_handle* handle, const uint8_t* d_cells, uint32_t count,
                                    uint32_t size_x, uint32_t size_y, double resolution,
                                    const double* d_origins, void* stream);

/* Replaces `client->async_send_request(request); result.get()` (cpp:248-250), i.e. the whole of
 * `MpcOptimizationServer.optimizer` (py:349-403), for `count` independent instances.  Synchronous.
 * Pageable host arrays are staged through device memory (copies queued around the kernel, one wait; batches of
 * 65 536 instances or more in four pieces on two streams, so that copies and kernels overlap).  When EVERY
 * array of the batch is page-locked (hipHostMalloc, hipHostRegister, neo_mpc_pin_host_memory below, torch
 * pin_memory) nothing is copied: the kernel reads the records from the caller's arrays and writes the results into
 * them over PCIe while other instances compute -- one launch and one wait per call. */
int neo_mpc_solve_batch(neo_mpc_handle* handle, const neo_mpc_batch* batch);
/* The same call in its two halves -- `client->async_send_request(request)` and `result.get()` (cpp:248-250) -- for
 * callers that keep more than one batch moving (a server of several fleets; double-buffered ticks): `begin` enqueues
 * the batch on a stream of its own and returns a ticket, `wait` blocks until that batch's results are in its arrays.
 * Every array of the batch must be page-locked (it is worked on in place, see above; NEO_MPC_ERR_UNSUPPORTED
 * otherwise) and must not be touched between the two calls.  Up to NEO_MPC_MAX_BATCHES_IN_FLIGHT tickets at a time;
 * ticket 0 (an empty batch) needs no wait.  neo_mpc_set_costmap between begin and wait is ordered behind the batches in
 * flight.  Not thread-safe per handle, like every other call. */
#define NEO_MPC_MAX_BATCHES_IN_FLIGHT 4
int neo_mpc_solve_batch_begin(neo_mpc_handle* handle, const neo_mpc_batch* batch, uint32_t* ticket);
int neo_mpc_solve_batch_wait(neo_mpc_handle* handle, uint32_t ticket);
/* Page-locks `bytes` of host memory at `ptr` for the device (hipHostRegister) / releases it: lets a caller built
 * without HIP headers -- the nav2 plugin is plain g++ -- keep its request arena where neo_mpc_solve_batch can work on
 * it in place.  The caller unpins before it frees the memory. */
int neo_mpc_pin_host_memory(void* ptr, size_t bytes);
int neo_mpc_unpin_host_memory(void* ptr);
/* How neo_mpc_solve_batch moves a batch whose arrays are all page-locked (pageable arrays are always staged). */
#define NEO_MPC_HOST_PATH_AUTO 0          /* = ZEROCOPY (NEO_MPC_HOST_PATH=staged|zerocopy|zerocopy_out in the environment
                                             of neo_mpc_create overrides what AUTO means, for A/B runs) */
#define NEO_MPC_HOST_PATH_STAGED 1        /* copies into device staging and back (DMA), as for pageable arrays */
#define NEO_MPC_HOST_PATH_ZEROCOPY 2      /* the kernel reads and writes the caller's arrays in place */
#define NEO_MPC_HOST_PATH_ZEROCOPY_OUT 3  /* inputs copied up by DMA, results written in place by the kernel */
int neo_mpc_set_host_path(neo_mpc_handle* handle, int mode);
/* Same with every pointer in device memory; enqueued on `stream`, returns without waiting. */
int neo_mpc_solve_batch_device(neo_mpc_handle* handle, const neo_mpc_batch* batch, void* stream);

/* Balanced dispatch for a fleet's NEXT tick (round 5; optional, changes no result).  A launch of up to 4096 instances is one
 * residency round on an MI355X -- workgroups w, w + 1024, w + 2048, w + 3072 share a SIMD -- and ends with the SIMD whose
 * four searches need the most iterations.  Robots keep their habits from tick to tick, so the iteration counts of the
 * previous tick (`d_previous_commands[i].iterations`, device memory, `count` records) predict the next tick's load: the
 * library sorts the instances by them (by their exponential average over successive calls of the same count, decay 1/2),
 * deals them over the SIMDs longest first, and the following
 * neo_mpc_solve_batch_device[_timed] calls OF THE SAME COUNT on this handle solve instance order[w] in workgroup w (every
 * array of the batch stays in the caller's order; every instance's result is bit for bit what it is without).  The order
 * is built by a small kernel on `stream` -- enqueue the next solve behind it, i.e. on the same stream or behind an event.
 * Refresh it every few ticks; counts that are not a multiple of 1024, or beyond 4096, get launch order.
 * d_previous_commands == NULL: back to launch order. */
int neo_mpc_balance_dispatch_device(neo_mpc_handle* handle, const neo_mpc_command* d_previous_commands, size_t count,
                                    void* stream);
/* Test hook: what the last neo_mpc_balance_dispatch_device left in the handle.  Host pointers; either array may be NULL.
 * `*count_out`: the count the handle is armed for, 0 when it is disarmed (never armed, disarmed with NULL, or a failed
 * call) -- then nothing else is written.  `order_out` receives `count` entries: workgroup w of the next solve of that
 * count solves instance order_out[w].  `load_out` receives `count` entries, the exponential averages the order is sorted
 * by, ONLY for a count the library sorts (a multiple of 1024 up to 4096): for a count that gets launch order the averages
 * are never computed and `load_out` is left untouched.  Off the hot path: waits for the whole device (the order is built
 * on the caller's stream), then copies. */
int neo_mpc_get_dispatch_order(neo_mpc_handle* handle, uint32_t* order_out, float* load_out, size_t* count_out);
/* Same; `start_event` / `stop_event` (hipEvent_t, either may be NULL) are stamped with the start and the
 * end of the solve kernel by the dispatch itself (hipExtLaunchKernel): a measurement harness gets K1's
 * duration without putting event-record packets between consecutive launches. */
int neo_mpc_solve_batch_device_timed(neo_mpc_handle* handle, const neo_mpc_batch* batch, void* stream,
                                     void* start_event, void* stop_event);

/* Only the part of `optimizer` after the solve (py:365-403): low-pass, collision check, stop
 * latch, acceleration clamp, warm-start shift, with `batch->solution` supplying `x.x` and
 * `success[i]` supplying `x.success` (NULL: all true).  Host pointers. */
int neo_mpc_postprocess_batch(neo_mpc_handle* handle, const neo_mpc_batch* batch,
                              const int32_t* success);

/* Test hook: the total gradient the solve kernel works with at u[count][3*control_steps] (projected onto the
 * feasible set first, like x0): analytic adjoint gradient of the tracking + terminal cost plus the gradient of
 * the control norm, taken from inside the kernel variant the current parameters select.  What SciPy obtains
 * by forward differences of `objective` (py:204-269; _slsqp_py.py:381).  Host pointers. */
int neo_mpc_gradient_batch(neo_mpc_handle* handle, const neo_mpc_problem* problems, const double* u,
                           double* grad_out, size_t count);

/* Test hook: the search direction of lanes 32-63 (Newton / L-BFGS) in solver iteration `iteration` (0-based) of a
 * solve started from u (instances that stop earlier leave their row untouched).  Host pointers. */
int neo_mpc_direction_batch(neo_mpc_handle* handle, const neo_mpc_problem* problems, const double* u,
                            double* dir_out, size_t count, int iteration);

/* `MpcOptimizationServer.objective` (py:204-269) evaluated on the device for
 * u[count][3*control_steps] (not projected); `footprint_cost` from problems[i].  Host pointers. */
int neo_mpc_objective_batch(neo_mpc_handle* handle, const neo_mpc_problem* problems,
                            const double* u, double* cost_out, size_t count);

/* Carrot selection for `count` robots (host pointers / device pointers + stream): replaces
 * transformGlobalPlan's pruning, getLookAheadDistance, getLookAheadPoint and the slow_down_ state
 * machine (cpp:83-104, 157-189, 221-232) with the plan->base transform taken as the planar rigid
 * transform given by the robot pose. */
int neo_mpc_select_carrots(neo_mpc_handle* handle, const neo_mpc_lookahead_params* params,
                           const neo_mpc_plan_batch* batch);
int neo_mpc_select_carrots_device(neo_mpc_handle* handle, const neo_mpc_lookahead_params* params,
                                  const neo_mpc_plan_batch* batch, void* stream);

/* The footprint gate for `count` robots (neo_mpc_footprint_batch above).  Host pointers, synchronous: the results are in the
 * caller's arrays when it returns.  NEO_MPC_ERR_NO_COSTMAP before a costmap is set; NEO_MPC_ERR_INVALID_ARGUMENT for
 * footprint_points outside 3 .. 16, a null `footprint` / `footprint_costs`, `poses` and `problems` both null, a pose, quaternion
 * or polygon coordinate that is not finite, and -- with a costmap pool -- a map index (map_indices[i], else
 * problems[i].map_index) outside [0, pool size).  count == 0 is NEO_MPC_OK and launches nothing. */
int neo_mpc_footprint_gate(neo_mpc_handle* handle, const neo_mpc_footprint_batch* batch);
/* Same with every pointer in device memory; enqueued on `stream` (hipStream_t, may be NULL), returns without waiting.  The
 * values are not looked at on the host: a coordinate that is not finite puts its vertex off the map (cost 254), and a map
 * index outside the pool is clamped into it -- below 0 reads map 0, beyond the last map the last one -- exactly as the solve
 * kernel treats neo_mpc_problem.map_index.  Both variants wait for a costmap ingest in flight on their stream and count as a
 * user of the device map for the next ingest, like a solve (see neo_mpc_set_costmap). */
int neo_mpc_footprint_gate_device(neo_mpc_handle* handle, const neo_mpc_footprint_batch* batch, void* stream);

/* The world map the rolling windows are cut from (neo_mpc_window_batch above): raw nav2 costs, row-major
 * cells[my*size_x + mx], geometry checked like neo_mpc_set_costmap's.  The handle keeps its OWN device copy: `cells` is
 * consumed before the call returns and no caller pointer is retained.  It does not touch the handle's costmap(s). */
int neo_mpc_set_world_map(neo_mpc_handle* handle, const uint8_t* cells, uint32_t size_x, uint32_t size_y,
                          double resolution, double origin_x, double origin_y);
/* Same, `d_cells` in device memory: a device-to-device copy enqueued on `stream` (hipStream_t, may be NULL) -- `d_cells`
 * is the caller's again once that copy has run.  Both variants wait for the last roll before they overwrite the copy; the
 * copy has an event of its own and a roll on another stream waits for it. */
int neo_mpc_set_world_map_device(neo_mpc_handle* handle, const uint8_t* d_cells, uint32_t size_x, uint32_t size_y,
                                 double resolution, double origin_x, double origin_y, void* stream);

/* nav2's inflation layer on the world map (K9): set -> inflate -> roll.  A fleet server usually holds an occupancy grid of
 * 0 / 254 / 255; the solver's costmap term, the gate's `footprint_cost > 200` (cpp:225-228) and `w_costmap` want the slopes
 * nav2's InflationLayer puts around the walls.  These calls rewrite the handle's OWN copy of the world map in place -- the
 * caller's buffer was released by neo_mpc_set_world_map[_device] and is not involved -- and every later roll cuts its windows
 * from the inflated map; when the world changes: set the raw map again, inflate again.  An inflation is not undone.
 *
 * Like neo_mpc_stamp_batch's, the contract is one by transcription (tests/world_inflation_reference.py is its executable
 * form): the cost rule and the combination rule are the stamp's, word for word, which are nav2's with inflate_unknown
 * false.  nav2's own InflationLayer is a queue-ordered wavefront; its result is this one up to the order in which it reaches
 * the cells within a distance bin.  Neither is pinned against nav2 itself: nav2's layers are not available to the tests.
 * Apart from the table T, which neo_mpc_inflation_costs builds on the host, the contract is integers only.
 *
 * Reach and table: the world map is WSX x WSY cells at resolution wres; R = ceil(inflation_radius / wres); T[0 .. R^2] is
 * exactly what neo_mpc_inflation_costs(wres, inscribed_radius, inflation_radius, cost_scaling_factor, ...) returns.
 * R > NEO_MPC_MAX_INFLATION_CELLS is refused with NEO_MPC_ERR_UNSUPPORTED.
 *
 * Seeds: the cells of the world map whose value is 254 (LETHAL_OBSTACLE) when the call starts.  Nothing else is a seed: not
 * 253, not 255 (nav2's inflate_around_unknown is out of scope), and nothing beyond the map's edges.
 *
 * Distance: for cell (i, l), N = min (i - i')^2 + (l - l')^2 over the seeds (i', l'), an integer.  N > R^2 leaves the cell
 * as it is; so does a map without seeds.
 *
 * Cost and combination: c = T[N], old = the cell's value: old == 255 becomes c when c >= 253 and stays 255 otherwise; any
 * other old becomes max(old, c).
 *
 * Two consequences: the set of cells equal to 254 is the same before and after (T[n] <= 253 for n >= 1, and 254 stays 254);
 * and the operation is idempotent -- inflating an inflated map with the same parameters changes nothing.
 *
 * neo_mpc_inflate_world_map is synchronous.  NEO_MPC_ERR_INVALID_ARGUMENT for a null handle and for a radius or scaling
 * factor that is negative or not finite; NEO_MPC_ERR_NO_COSTMAP before neo_mpc_set_world_map; NEO_MPC_ERR_UNSUPPORTED for
 * R > NEO_MPC_MAX_INFLATION_CELLS.  A refused call leaves the map as it was. */
int neo_mpc_inflate_world_map(neo_mpc_handle* handle, double inscribed_radius, double inflation_radius,
                              double cost_scaling_factor);
/* Same, enqueued on `stream` (hipStream_t, may be NULL), returns without waiting.  Ordered exactly like
 * neo_mpc_set_world_map_device's copy, which writes the same buffer: it waits on its stream for the last roll, which reads
 * the copy, and for the previous copy or inflation when that ran on another stream; a roll on another stream waits for it.
 * The cost table is kept in the handle, apart from the stamp's (windows and world may differ in resolution): when (wres,
 * inscribed_radius, inflation_radius, cost_scaling_factor) differ from the previous call's it is rebuilt and uploaded
 * synchronously; otherwise the call allocates nothing, copies nothing and does not synchronise, so set_world_map_device ->
 * inflate_world_map_device -> roll -> stamp -> gate -> carrots -> solve can be captured on one stream in one HIP graph. */
int neo_mpc_inflate_world_map_device(neo_mpc_handle* handle, double inscribed_radius, double inflation_radius,
                                     double cost_scaling_factor, void* stream);
/* Reads the handle's copy of the world map back, as the last neo_mpc_set_world_map or inflation left it: the cells,
 * cells_out[size_y][size_x], and the geometry; any out pointer may be NULL (sizes first, then the cells).  Host pointers,
 * synchronous; waits for the copy or inflation in flight -- one that was ENQUEUED by a call.  Work replayed from a HIP graph
 * is not waited for: the handle's event was recorded while the graph was captured, and waiting for such an event does not
 * wait for a replay (the same holds for neo_mpc_get_costmap_pool, and for the wait in front of a rebuilt cost table), so behind
 * a replay synchronise the replay's stream first.  For display and logging: until a roll, the copy exists in device memory
 * only.  NEO_MPC_ERR_NO_COSTMAP before neo_mpc_set_world_map. */
int neo_mpc_get_world_map(neo_mpc_handle* handle, uint8_t* cells_out, uint32_t* size_x, uint32_t* size_y, double* resolution,
                          double* origin_x, double* origin_y);

/* Moves the windows to their robots and fills them from the world map (K7; the contract: neo_mpc_window_batch).  Afterwards
 * the handle's costmap IS this pool -- `count` maps of size_x x size_y cells, stored as neo_mpc_set_costmap_pool stores
 * them; it replaces whatever the handle held -- and every instance reads the window its neo_mpc_problem.map_index names.
 * Host pointers, synchronous: `origins` has been written back when it returns.  NEO_MPC_ERR_NO_COSTMAP before
 * neo_mpc_set_world_map; NEO_MPC_ERR_INVALID_ARGUMENT for a null `origins`, count > NEO_MPC_MAX_POOL_MAPS, a zero size, a
 * resolution that is not positive and finite, outside_value > 255, a non-zero `reserved`, and a pose or origin that is not
 * finite; a refused call leaves the handle's costmap as it was.  count == 0 is NEO_MPC_OK and launches nothing. */
int neo_mpc_roll_costmap_pool(neo_mpc_handle* handle, const neo_mpc_window_batch* windows);
/* Same with every pointer in device memory; enqueued on `stream`, returns without waiting; no value behind a pointer is
 * looked at on the host.  `origins` is retained: it is read by every later solve and gate, exactly like `d_origins` of
 * neo_mpc_set_costmap_pool_device, and must stay valid.  A roll with the geometry, count and `origins` pointer of the
 * previous one allocates nothing and does not synchronise, so roll -> gate -> carrots -> solve can be captured in a HIP
 * graph on one stream and replayed with new poses.  Ordering, both variants: a roll waits on its stream for the previous
 * ingest or roll, for every launch still reading the device map and for the world map's copy, and the solves and gates
 * behind it wait for it -- like neo_mpc_set_costmap. */
int neo_mpc_roll_costmap_pool_device(neo_mpc_handle* handle, const neo_mpc_window_batch* windows, void* stream);

/* Reads the handle's costmap(s) back: the raw cells of maps [first, first + count) of the pool -- or of the single map, a
 * pool of one -- without border and pitch, cells_out[count][size_y][size_x], and their origins, origins_out[count][2]
 * (either may be NULL).  Host pointers, synchronous; waits for the ingest or roll in flight.  For callers whose windows
 * exist in device memory only (logging, display).  NEO_MPC_ERR_NO_COSTMAP without a costmap, NEO_MPC_ERR_INVALID_ARGUMENT
 * for a range outside the pool. */
int neo_mpc_get_costmap_pool(neo_mpc_handle* handle, uint32_t first, uint32_t count, uint8_t* cells_out,
                             double* origins_out);

/* The cost table T of neo_mpc_stamp_batch for windows of resolution `resolution`: pure host arithmetic (libm), no handle, no
 * device.  *cells_out = R (may be NULL); with `table_out` not NULL, T[0 .. R^2] is written and `capacity` must be at
 * least R^2 + 1 bytes.  NEO_MPC_ERR_INVALID_ARGUMENT for a resolution that is not positive and finite, a radius or scaling
 * factor that is negative or not finite, or a capacity that is too small; NEO_MPC_ERR_UNSUPPORTED when
 * R > NEO_MPC_MAX_INFLATION_CELLS. */
int neo_mpc_inflation_costs(double resolution, double inscribed_radius, double inflation_radius, double cost_scaling_factor,
                            uint8_t* table_out, size_t capacity, uint32_t* cells_out);

/* Stamps the fleet's robots into each other's windows (K8; the contract: neo_mpc_stamp_batch).  Host pointers, synchronous.
 * Refusals, all of which leave the pool as it was: NEO_MPC_ERR_INVALID_ARGUMENT for a null argument, a non-zero `reserved`,
 * footprint_points outside 3 .. NEO_MPC_MAX_FOOTPRINT_POINTS, per_robot_footprints other than 0 or 1, a radius or scaling
 * factor that is negative or not finite, neither `polygons` nor a `footprint` with `poses` or `problems`, a pose or vertex
 * that is not finite, and a `count` that is not the pool's map count; NEO_MPC_ERR_NO_COSTMAP when the handle holds no
 * costmap; NEO_MPC_ERR_UNSUPPORTED when it holds a single costmap instead of a pool, and when
 * R > NEO_MPC_MAX_INFLATION_CELLS.  count == 0 is NEO_MPC_OK and does nothing. */
int neo_mpc_stamp_fleet(neo_mpc_handle* handle, const neo_mpc_stamp_batch* batch);
/* Same with every pointer in device memory; enqueued on `stream`, returns without waiting; no value behind a pointer is
 * looked at on the host.  The cost table is kept in the handle: when (resolution, inscribed_radius, inflation_radius,
 * cost_scaling_factor) differ from the previous call's it is rebuilt and uploaded synchronously; otherwise a call with the
 * count and footprint_points of an earlier one allocates nothing and copies nothing, so roll -> stamp -> gate -> carrots ->
 * solve can be captured in a HIP graph on one stream.  Ordering, both variants: a stamp rewrites the device maps in place,
 * so like a roll it waits on its stream for the previous ingest, roll or stamp and for every launch still reading the maps,
 * and the gates and solves behind it wait for it. */
int neo_mpc_stamp_fleet_device(neo_mpc_handle* handle, const neo_mpc_stamp_batch* batch, void* stream);

/* Updates the windows' obstacle layers from one observation per robot and puts them into the windows (K10; the contract:
 * neo_mpc_scan_batch).  Host pointers, synchronous.  Refusals, all of which leave pool and layers as they were:
 * NEO_MPC_ERR_INVALID_ARGUMENT for a null handle or batch, a non-zero `reserved`, flag bits beyond the two, an unknown_value
 * other than 0 or 255, max_points > NEO_MPC_MAX_SCAN_POINTS, a null `points` or `sensor_origins` with non-zero flags, a
 * range, radius or scaling factor that is negative or not finite, a `count` that is not the pool's map count, and -- in this
 * variant only -- a point_counts[k] > max_points or a sensor origin that is not finite; NEO_MPC_ERR_NO_COSTMAP without a
 * costmap; NEO_MPC_ERR_UNSUPPORTED for a single costmap instead of a pool, and for R > NEO_MPC_MAX_INFLATION_CELLS.
 * count == 0 is NEO_MPC_OK and does nothing. */
int neo_mpc_update_scan_layer(neo_mpc_handle* handle, const neo_mpc_scan_batch* batch);
/* Same with every pointer in device memory; enqueued on `stream`, returns without waiting; no value behind a pointer is
 * looked at on the host: a point_counts[k] beyond max_points is clamped to it, and a sensor origin that is not finite fails
 * worldToMap.  Ordering, both variants: an update is a write of the device maps exactly like a stamp -- it waits on its
 * stream for the previous ingest, roll, stamp or update and for every launch still reading the maps, and the gates and solves
 * behind it wait for it; the layer buffers are touched only inside such writes, so the same chain orders them.
 * Memory: the layers cost the handle up to two more pools' worth of device memory (the layers, and those of the update in
 * flight).  They are allocated on the first update and reallocated only on a reset by geometry.  The cost table is kept in
 * the handle, apart from the stamp's and the world's, and rebuilt and uploaded synchronously when (res, inscribed_radius,
 * inflation_radius, cost_scaling_factor) differ from the previous update's.  A device update with the geometry, count and
 * inflation parameters of the previous one allocates nothing, copies nothing and does not synchronise, so roll -> scan ->
 * stamp -> gate -> carrots -> solve can be captured on one stream in one HIP graph and replayed with new points. */
int neo_mpc_update_scan_layer_device(neo_mpc_handle* handle, const neo_mpc_scan_batch* batch, void* stream);
/* Reads layers [first, first + count) back as the last update left them: cells_out[count][size_y][size_x] and their origins,
 * origins_out[count][2] (either may be NULL).  Host pointers, synchronous; waits for the write of the device maps in flight
 * -- one that was ENQUEUED by a call: behind a graph replay synchronise the replay's stream first (neo_mpc_get_world_map says
 * why).  NEO_MPC_ERR_NO_COSTMAP when there is no layer -- before the first update and behind neo_mpc_reset_scan_layer;
 * NEO_MPC_ERR_INVALID_ARGUMENT for a null handle and a range outside the layers. */
int neo_mpc_get_scan_layer(neo_mpc_handle* handle, uint32_t first, uint32_t count, uint8_t* cells_out, double* origins_out);
/* The next update starts from a layer of unknown_value.  Touches no device memory.  NEO_MPC_ERR_INVALID_ARGUMENT for a null
 * handle. */
int neo_mpc_reset_scan_layer(neo_mpc_handle* handle);

/* The beam table of one scanner (K11; the contract: neo_mpc_laser_batch, step 4): table_out[beams][2] = (cos, sin) of every
 * beam's angle in the base frame.  Pure host code: no handle, no device.  NEO_MPC_ERR_INVALID_ARGUMENT for a null argument,
 * beams outside 1 .. NEO_MPC_MAX_SCAN_POINTS and a scanner the projection refuses (below). */
int neo_mpc_laser_beam_table(const neo_mpc_scanner* scanner, uint32_t beams, double* table_out);
/* Projects LaserScan ranges into global-frame points and sensor origins (K11), and nothing else: for display, logging and
 * tests.  `points_out` and `origins_out` are required; scan_flags, unknown_value and the range and inflation fields are
 * ignored; no costmap is needed, layers and pool are not touched and `count` is free.  Host pointers, synchronous.
 * Refusals, which leave the out buffers alone: NEO_MPC_ERR_INVALID_ARGUMENT for a null handle, batch or array, a non-zero
 * `reserved` of the batch or of a scanner, `sources` outside 1 .. NEO_MPC_MAX_SCAN_SOURCES, beams == 0 or
 * sources * beams > NEO_MPC_MAX_SCAN_POINTS, unknown scanner flag bits, a mount, angle or range of a scanner that is not
 * finite, range_min < 0, range_max < range_min, and -- in the host variants only -- a pose that is not finite.
 * count == 0 is NEO_MPC_OK and does nothing. */
int neo_mpc_project_laser(neo_mpc_handle* handle, const neo_mpc_laser_batch* batch);
/* Same with `ranges`, `poses` and the two out arrays in device memory (`scanners` stays a host pointer); enqueued on
 * `stream`, returns without waiting; no value behind the device pointers is looked at: a pose that is not finite yields
 * points that are not finite, which the layer update skips.  A `points_out` that is not 16-byte aligned is refused.  The
 * beam tables are kept in the handle, keyed by the scanners' bytes and `beams`: when they differ from the previous call's
 * the tables are rebuilt and uploaded synchronously; otherwise the call allocates nothing, copies nothing and does not
 * synchronise. */
int neo_mpc_project_laser_device(neo_mpc_handle* handle, const neo_mpc_laser_batch* batch, void* stream);
/* Projects the ranges (K11) and updates the windows' obstacle layers from all sources (the contract: neo_mpc_laser_batch).
 * Host pointers, synchronous; `points_out` / `origins_out`, when given, receive what was projected.  Refusals, all of which
 * leave pool, layers and out buffers as they were: those of neo_mpc_project_laser; scan_flags == 0 or with bits beyond the
 * two; and every refusal of neo_mpc_update_scan_layer that concerns unknown_value, the ranges, the inflation parameters,
 * `count` and the pool, with the same codes.  count == 0 is NEO_MPC_OK and does nothing. */
int neo_mpc_update_scan_layer_from_ranges(neo_mpc_handle* handle, const neo_mpc_laser_batch* batch);
/* Same with device pointers, enqueued on `stream`.  Ordering: the projection and the update are one write of the device
 * maps, fenced exactly like neo_mpc_update_scan_layer_device.  Memory: without `points_out` / `origins_out` the handle
 * keeps count * sources * beams * 16 bytes of points and count * sources * 16 bytes of origins, allocated on the first use
 * and on a change of (count, sources, beams).  A call with the scanners, count, sources, beams, geometry and inflation
 * parameters of the previous one allocates nothing, copies nothing and does not synchronise, so roll -> scan from ranges ->
 * stamp -> gate -> carrots -> solve can be captured on one stream in one HIP graph and replayed with new ranges and poses. */
int neo_mpc_update_scan_layer_from_ranges_device(neo_mpc_handle* handle, const neo_mpc_laser_batch* batch, void* stream);

/* Updates the fleet's shared obstacle layer on the world map from one observation per robot and composes `live` (K12; the
 * contract: neo_mpc_fleet_clear above).  `batch` is neo_mpc_scan_batch's record with `count` = the number of robots, 1 ..
 * NEO_MPC_MAX_POOL_MAPS (0 does nothing); `clear` may be NULL.  Host pointers, synchronous.  Refusals, all of which leave
 * layer, live and their validity as they were: those of neo_mpc_update_scan_layer that concern `reserved`, the flags,
 * unknown_value, max_points, null arrays with non-zero flags, the ranges and radii, point_counts and sensor origins, with the
 * same codes and texts; NEO_MPC_ERR_NO_COSTMAP before neo_mpc_set_world_map; NEO_MPC_ERR_UNSUPPORTED for
 * R > NEO_MPC_MAX_INFLATION_CELLS at the world's resolution; NEO_MPC_ERR_INVALID_ARGUMENT for count > NEO_MPC_MAX_POOL_MAPS
 * and, of the clear record, the refusals of neo_mpc_stamp_fleet (reserved, footprint_points, per_robot_footprints, neither
 * polygons nor a footprint with poses or problems, a pose or vertex that is not finite), a `padding` that is negative or not
 * finite, and a `count` other than the batch's. */
int neo_mpc_update_world_scan_layer(neo_mpc_handle* handle, const neo_mpc_scan_batch* batch, const neo_mpc_fleet_clear* clear);
/* Same with every pointer of both records in device memory; enqueued on `stream`, returns without waiting; no value behind a
 * pointer is looked at on the host.  Ordering: an update reads the world map and rewrites what the roll reads, so it is fenced
 * exactly like neo_mpc_inflate_world_map_device -- it waits on its stream for the last roll and the previous copy, inflation
 * or update, and a roll on another stream waits for it.  Memory: two more world maps' worth (with decay on, four more bytes a
 * cell), allocated on the first update and on a larger world.  The cost table is kept in the handle, apart from K8's, K9's and K10's, and rebuilt synchronously
 * when (wres, inscribed_radius, inflation_radius, cost_scaling_factor) differ from the previous update's.  A device update
 * with the shapes and inflation parameters of the previous one allocates nothing, copies nothing and does not synchronise, so
 * world scan -> roll -> stamp -> gate -> carrots -> solve can be captured on one stream in one HIP graph and replayed with
 * new points and poses.  The roll's source -- `live` or the world map -- is a pointer fixed when the roll is CAPTURED: capture
 * the roll behind an update, and capture again after a call that invalidates `live`. */
int neo_mpc_update_world_scan_layer_device(neo_mpc_handle* handle, const neo_mpc_scan_batch* batch, const neo_mpc_fleet_clear* clear,
                                           void* stream);
/* K11's projection, unchanged, in front of steps 1 to 4 over all sources (the contract: neo_mpc_laser_batch, with the
 * world's layer in place of the windows').  Refusals: those of neo_mpc_update_scan_layer_from_ranges with the pool's replaced
 * by the world's as above, and those of the clear record. */
int neo_mpc_update_world_scan_layer_from_ranges(neo_mpc_handle* handle, const neo_mpc_laser_batch* batch,
                                                const neo_mpc_fleet_clear* clear);
/* Same with device pointers (`scanners` stays a host pointer), enqueued on `stream`: the projection and the update are one
 * rewrite of what the roll reads, fenced like neo_mpc_update_world_scan_layer_device; a call with the scanners, shapes and
 * inflation parameters of the previous one allocates nothing, copies nothing and does not synchronise. */
int neo_mpc_update_world_scan_layer_from_ranges_device(neo_mpc_handle* handle, const neo_mpc_laser_batch* batch,
                                                       const neo_mpc_fleet_clear* clear, void* stream);
/* Reads the layer and `live` back as the last update left them, layer_out[WSY][WSX] and live_out[WSY][WSX] on the geometry of
 * the world map of that update (either may be NULL); `live` is returned whether or not it is still valid.  Host pointers,
 * synchronous; waits for the update in flight -- one that was ENQUEUED by a call (neo_mpc_get_world_map says why).
 * NEO_MPC_ERR_NO_COSTMAP before the first update, behind neo_mpc_reset_world_scan_layer and behind a neo_mpc_set_world_map of
 * another size (the next update resets the layer in that case anyway). */
int neo_mpc_get_world_scan_layer(neo_mpc_handle* handle, uint8_t* layer_out, uint8_t* live_out);
/* The next update starts from a layer of unknown_value, and until then the roll reads the world map.  Touches no device
 * memory.  NEO_MPC_ERR_INVALID_ARGUMENT for a null handle. */
int neo_mpc_reset_world_scan_layer(neo_mpc_handle* handle);
/* The speckle filter of the shared layer (step 3b of the contract above; K13).  minimal_group_size 0 or 1: off; 2 ..
 * NEO_MPC_MAX_DENOISE_GROUP: on.  connectivity: 4 or 8, checked when off as well.  Anything else, and a null handle, is
 * NEO_MPC_ERR_INVALID_ARGUMENT and leaves the previous setting in force.  The call needs no world map, launches nothing and
 * touches neither layer nor live nor their validity: the setting takes effect with the next update, and an update with
 * flags == 0 is enough to recompose.  It is handle configuration: it survives neo_mpc_reset_world_scan_layer and
 * neo_mpc_set_world_map, and a handle on which it was never called behaves as before.  Memory: one more world map's worth
 * while the filter is on, allocated by the first update behind switching it on and by an update on a larger world -- that
 * update may synchronise; a later one with the same geometry and setting allocates nothing, so the tick stays capturable
 * after one eager call.  A captured HIP graph holds the setting it was captured with. */
int neo_mpc_set_world_scan_denoise(neo_mpc_handle* handle, uint32_t minimal_group_size, uint32_t connectivity);
/* Reads back D of the last update, cells_out[WSY][WSX]: the layer as step 4 read it -- the layer's own bytes when the filter
 * was off at that update.  Host pointer, synchronous; waits for the update in flight as neo_mpc_get_world_scan_layer does,
 * and returns NEO_MPC_ERR_NO_COSTMAP where it does.  A null cells_out only asks whether there is one. */
int neo_mpc_get_world_scan_denoised(neo_mpc_handle* handle, uint8_t* cells_out);
/* The decay of the shared layer's old marks (step 2b of the contract above; K14).  max_age 0: off; every other value: on, a
 * mark expires max_age scan updates after the last one that made it.  NEO_MPC_ERR_INVALID_ARGUMENT for a null handle.  The
 * call needs no world map, launches nothing and touches neither layer nor live nor their validity: the setting takes effect
 * with the next update, and an update with flags == 0 is enough to let a lowered max_age act.  It is handle configuration: it
 * survives neo_mpc_reset_world_scan_layer and neo_mpc_set_world_map, and a handle on which it was never called behaves as
 * before.  Memory: four bytes per world cell and a word while decay is on (16 MB on a 2000 x 2000 map), allocated by the
 * first update behind switching it on and by an update on a larger world -- that update may synchronise, and fills the
 * stamps; a later one with the same geometry allocates and copies nothing, so the tick stays capturable after one eager
 * call.  A captured HIP graph holds the max_age it was captured with; the clock is the device's and goes on counting. */
int neo_mpc_set_world_scan_decay(neo_mpc_handle* handle, uint32_t max_age);
/* The marks' ages as the last update left them, ages_out[WSY][WSX]: clock - stamp under a cell of the layer that is 254 -- 0
 * for a mark the last scan update made --, NEO_MPC_NO_AGE under every other cell.  For displays that fade marks, and for logs.
 * Host pointer, synchronous; waits for the update in flight as neo_mpc_get_world_scan_layer does, and returns
 * NEO_MPC_ERR_NO_COSTMAP where it does; NEO_MPC_ERR_UNSUPPORTED when the last update ran without decay.  A null ages_out only
 * asks whether there are any. */
int neo_mpc_get_world_scan_ages(neo_mpc_handle* handle, uint32_t* ages_out);

/* The plan check for `count` robots (neo_mpc_plan_check_batch above; K15).  Host pointers, synchronous: the records are in
 * `results` when it returns.  NEO_MPC_ERR_NO_COSTMAP without a world map; NEO_MPC_ERR_INVALID_ARGUMENT for a null handle or
 * record, a null plan_poses / plan_offsets / results with count > 0, max_cost outside 1 .. 254, unknown_blocks > 1,
 * outside_value > 255, reserved != 0, a footprint without footprint_points or the other way round, footprint_points outside
 * 3 .. 16, a count beyond 2^31 - 1 -- and, looked at on the host by this variant alone, plan_offsets that decrease and a
 * footprint vertex that is not finite.  Plan and robot poses are taken as they come: a coordinate that is not finite is off
 * the map, and the closest pose follows nav2's min_by.  count == 0 is NEO_MPC_OK and launches nothing. */
int neo_mpc_check_plans(neo_mpc_handle* handle, const neo_mpc_plan_check_batch* batch);
/* Same with every pointer in device memory; enqueued on `stream`, returns without waiting; no value behind a pointer is
 * looked at on the host.  The check orders itself like a roll, which reads the same map: it waits for the world map's writer
 * -- the copy, the inflation, the world-scan update that composed `live` -- and a later neo_mpc_set_world_map*,
 * neo_mpc_inflate_world_map* or world-scan update, on whatever stream, waits for its reads.  (Like a roll it also takes its
 * place among the launches on the device map, whose ordering carries this.)  Any time between a world-scan update and the
 * next one sees that update's map.  It allocates nothing, copies nothing and does not synchronise, so it can be captured in
 * a HIP graph with the rest of the tick. */
int neo_mpc_check_plans_device(neo_mpc_handle* handle, const neo_mpc_plan_check_batch* batch, void* stream);

/* The grid planner for `count` robots (neo_mpc_replan_batch above; K16).  Host pointers, synchronous: records and paths are in
 * the caller's arrays when it returns.  Refusals look at the record's shape alone: NEO_MPC_ERR_NO_COSTMAP without a world
 * map; NEO_MPC_ERR_INVALID_ARGUMENT for a null handle or record, a null starts / goals / path_cells / results with count > 0,
 * window outside 4 .. 128, max_cost outside 1 .. 254, unknown_cost > 252, neutral_cost outside 1 .. 255, max_path_cells == 0,
 * reserved != 0, a count beyond 2^31 - 1.  Coordinates are taken as they come: one that is not finite is off the map.
 * count == 0 is NEO_MPC_OK and launches nothing. */
int neo_mpc_replan_plans(neo_mpc_handle* handle, const neo_mpc_replan_batch* batch);
/* Same with every pointer in device memory; enqueued on `stream`, returns without waiting; no value behind a pointer is
 * looked at on the host.  It orders itself exactly like neo_mpc_check_plans_device, whose map it reads: behind the world
 * map's writer, and a later rewrite of that map waits for its reads.  `checks` may be the `results` of a
 * neo_mpc_check_plans_device call enqueued on the same stream before it: check and replan chain on the device.  It allocates
 * nothing, copies nothing and does not synchronise, so it can be captured in a HIP graph with the rest of the tick. */
int neo_mpc_replan_plans_device(neo_mpc_handle* handle, const neo_mpc_replan_batch* batch, void* stream);

/* ---- multi-GPU fleets: the one exchange step ------------------------------------------------
 * Instances of one tick shard embarrassingly over the GPUs of a node (one handle per GPU, costmap and parameters
 * replicated, per-instance state resident on its GPU); what `computeVelocityCommands` returns for every robot
 * (cpp:251-254) is collected with ONE all-gather of the packed `neo_mpc_batch.velocities` over RCCL (xGMI).
 * `comm` is an ncclComm_t of the caller's, or one made by neo_mpc_comm_init_all (a single process driving all
 * devices: bracket the per-device calls with neo_mpc_group_start / neo_mpc_group_end).  RCCL is bound at run time;
 * without librccl.so these return NEO_MPC_ERR_UNSUPPORTED and everything else keeps working.  No torch types. */
int neo_mpc_rccl_available(void);
int neo_mpc_comm_init_all(int ndev, const int* devices, void** comms_out);   /* ncclCommInitAll */
int neo_mpc_comm_destroy(void* comm);
int neo_mpc_group_start(void);
int neo_mpc_group_end(void);
/* d_local[count][3] of this rank -> d_all[world][count][3] on every rank, enqueued on `stream` (hipStream_t). */
int neo_mpc_allgather_velocities(const double* d_local, double* d_all, size_t count, void* comm, void* stream);
/* One-off: rank `root`'s raw costmap cells to every rank (in place), then neo_mpc_set_costmap_device per rank. */
int neo_mpc_broadcast_costmap(uint8_t* d_cells, size_t bytes, int root, void* comm, void* stream);

/* Bytes of LDS and costmap reach (cells) the solve kernel uses with the current params/map. */
int neo_mpc_kernel_info(const neo_mpc_handle* handle, uint32_t* lds_bytes, uint32_t* reach_cells,
                        uint32_t* tile_in_lds);

#ifdef __cplusplus
}
#endif
#endif /* NEO_MPC_H_ */
