// neo_mpc_kernels.hip -- gfx950 (CDNA4 / MI355X) kernels of the batched MPC solver.
//
// Replaces, for thousands of independent instances per launch, what the reference does
// one request at a time in Python: `MpcOptimizationServer.optimizer`
// (neo_mpc_planner2/mpc_optimization_server.py:349-403), i.e. the SciPy SLSQP `minimize`
// call (py:363-364) over `objective` (py:204-269) with the box bounds and the
// translational-speed disc (py:125-134, 157-158), followed by the low-pass, collision
// check, stop latch, acceleration clamp and warm-start shift (py:365-403).
//
//   K1 k_solve        k1_solve.h; this unit holds its dense-Newton and L-BFGS variants, neo_mpc_riccati.hip the others.
//   K2 postprocess    py:365-403, fused as the epilogue of K1 and launchable on its own.
//   K3 k_ingest       costmap_ingest.h: raw nav2 costmap -> device map with a lethal border and 128-byte row pitch (16 B per
//                     lane, HBM-streaming); the stream over a padded map and its grid, which K7's fill shares.
//   K4 k_carrot       the step before the solver: plan pruning + look-ahead point
//                     (src/NeoMpcPlanner.cpp:83-104, 157-189, 221-232), HBM-streaming.
//   k_objective       py:204-269 for given controls (parity checks of the objective).
//   K5 k_dispatch_order  which instance each workgroup of a K1 launch solves (balanced dispatch).
//   K6 k_footprint_gate  footprint_gate.h: the footprint gate in front of the carrot (cpp:218-219), one wave per robot.
//   K7 k_roll_index, k_roll_fill  rolling_window.h: a fleet's rolling costmap windows cut from one world map, HBM-streaming.
//   K8 k_stamp_boxes, k_stamp_fleet  fleet_stamp.h: the fleet's robots stamped into each other's windows, inflation ring included.
//   K9 k_inflate_world  world_inflation.h: nav2's inflation layer on the world map, in place (inflation.h: what it shares with K8 and K10).
//   K10 k_scan_shift, k_scan_rays, k_scan_apply  scan_layer.h: the obstacle layer of every window, fed from sensor points.
//   K11 k_laser_project  laser_projection.h: LaserScan ranges of every scanner of every robot -> those points, HBM-streaming.
//   K12 k_world_scan_rays, k_world_scan_footprints, k_world_scan_compose  world_scan_layer.h: one obstacle layer for the fleet on the world map.
//   K13 k_world_scan_denoise  world_scan_denoise.h: that layer's speckle filter, groups of fewer than G occupied cells, in front of K12's composition.
//   K14 k_world_scan_tick, k_world_scan_stamp_fill, k_world_scan_marks_stamped, k_world_scan_decay  world_scan_decay.h: that layer's old marks expire, counted in scan updates.
//   K15 k_plan_check  plan_check.h: which of the fleet's global plans the live world map blocks, one wave per plan, HBM-streaming;
//                     K4's closest-pose stream lives there too.
//   K16 k_replan  grid_planner.h: detours for the blocked plans on that map, one workgroup per robot, the search in LDS.
#include "k1_solve.h"
#include "costmap_ingest.h"
#include "footprint_gate.h"
#include "rolling_window.h"
#include "fleet_stamp.h"
#include "world_inflation.h"
#include "scan_layer.h"
#include "laser_projection.h"
#include "world_scan_layer.h"
#include "world_scan_denoise.h"
#include "world_scan_decay.h"
#include "plan_check.h"
#include "grid_planner.h"

namespace neo_mpc {
namespace {

// K2 on its own: `solution` supplies x.x, `success` supplies x.success
__global__ __launch_bounds__(kLanes) void k_postprocess(const SolveArgs args) {
  extern __shared__ __align__(16) double L[];
  SolveArgs a = args;
  const int lane = threadIdx.x;
  const uint32_t b = blockIdx.x;
  if (b >= a.count) return;
  const int nv = 3 * a.p.n;
  load_records(a, L, b, lane);
  if (uniform_int(reinterpret_cast<const int*>(L + a.lds.prob)[PI_SKIP]) == 1) { skip_instance(a, b, lane, true); return; }   // (no request this tick: see k_solve)
  select_map(a.map, L + a.lds.prob);
  int flags = reset_and_warm(a, L, b, lane) ? NEO_MPC_FLAG_RESET : 0;
  const double fcost = footprint_cost(a, L, b, lane);
  Ctx c;
  make_ctx_wave(a.p, a.map, L + a.lds.prob, fcost, c, lane);
  load_tile(a, c, L, lane);
  if (c.tile_geom & kTileWall) flags |= NEO_MPC_FLAG_WALL_IN_REACH;
  double* u = L + a.lds.u;
  for (int k = lane; k < nv; k += kLanes) u[k] = a.solution[(size_t)b * nv + k];
  WAVE_SYNC();
  double f = rollout_cost(a, c, L, [&](int i, double& b0, double& b1, double& b2) {
    b0 = u[3 * i]; b1 = u[3 * i + 1]; b2 = u[3 * i + 2];
  });
  f = __shfl(f, 0);
  const bool success = a.success ? a.success[b] != 0 : true;
  postprocess(a, c, L, b, lane, u, success, fcost, flags, f, success ? 0 : 1, 0, 1);
}

// py:204-269 for given controls, one lane per instance -- the PARITY kernel: it follows the reference statement by
// statement (the solver's own rollout forms the world position as X0 + Rot(psi0) (x, y) from the base-frame rollout;
// this one accumulates odom_yaw, pos_x and pos_y step by step like py:234-236, takes the square root of the distance and
// squares it again like py:250-252, and divides by control_steps where the reference does), so that it differs from the
// reference only in the last bits of sin / cos / atan2.
__global__ __launch_bounds__(256) void k_objective(const ObjectiveArgs a) {
  __shared__ double cost_of[256];   // getCost by raw cell value: occupancy / 100 (the build's costmap contract)
  cost_of[threadIdx.x] = raw_cost((int)threadIdx.x);
  __syncthreads();
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.count) return;
  DevMap map = a.map;
  const double* P = reinterpret_cast<const double*>(a.problems + b);
  select_map<false>(map, P);
  const int n = a.p.n;
  const double dt = a.p.dt, w_trans = a.w_trans, w_orient = a.w_orient, w_control = a.w_control;
  const double target_yaw = yaw_of(P + P_CARROT_Q);                       // py:211
  const double final_yaw = yaw_of(P + P_GOAL_Q);                          // py:212
  const double q0[4] = {P[P_CUR_Q], P[P_CUR_Q + 1], P[P_CUR_Q + 2],
                        (a.p.compat & NEO_MPC_COMPAT_ODOM_YAW_GOAL_W) ? P[P_GOAL_Q + 3] : P[P_CUR_Q + 3]};
  double odom_yaw = yaw_of(q0);                                           // py:213 (the goal's w: reference quirk)
  const double* u = a.u + (size_t)b * 3 * n;
  const double footprint = P[P_FOOTPRINT];
  double total = 0.0, x = 0.0, y = 0.0, z = 0.0;
  double pos_x = P[P_CUR_X], pos_y = P[P_CUR_Y];                          // py:220-221
  for (int i = 0; i < n; ++i) {
    const double vx = u[3 * i], vy = u[3 * i + 1], wz = u[3 * i + 2];
    z += wz * dt;                                                         // py:230
    double sz, cz;
    sincos(z, &sz, &cz);
    x += (vx * cz * dt - vy * sz * dt);                                   // py:231
    y += (vx * sz * dt + vy * cz * dt);                                   // py:232
    odom_yaw += wz * dt;                                                  // py:234
    double so, co;
    sincos(odom_yaw, &so, &co);
    pos_x += vx * co * dt - vy * so * dt;                                 // py:235
    pos_y += vx * so * dt + vy * co * dt;                                 // py:236
    const int mx = cell_of(pos_x, map.origin_x, map.resolution, map.inv_resolution);   // py:246
    const int my = cell_of(pos_y, map.origin_y, map.resolution, map.inv_resolution);
    const double c = cost_of[map_raw(map, mx, my)];
    const double costmap_cost = c * c;                                    // py:247
    const double ddx = P[P_CARROT_X] - x, ddy = P[P_CARROT_Y] - y;
    const double dist = sqrt(ddx * ddx + ddy * ddy);                      // py:250
    const double eth = target_yaw - z;                                    // py:251
    total += ((w_trans * (dist * dist)) + (w_orient * (eth * eth))) / n;  // py:252
    const double e0 = P[P_VEL] - vx, e1 = P[P_VEL + 1] - vy, e2 = P[P_VEL + 2] - wz;
    total += w_control * sqrt(e0 * e0 + e1 * e1 + e2 * e2) / n;           // py:253-254
    if (c == 1.0) total += costmap_cost * 1000 / n;                       // py:257-258
    else total += a.w_costmap * costmap_cost / n;                         // py:260
    if (footprint == 1.0) total += (footprint * footprint) * a.p.w_footprint / n;   // py:262-263
  }
  const double gdx = P[P_CARROT_X] - P[P_GOAL], gdy = P[P_CARROT_Y] - P[P_GOAL + 1];
  const double gdist = sqrt(gdx * gdx + gdy * gdy);                       // py:266
  const double eth = final_yaw - z;                                       // py:267
  total += ((w_trans * (gdist * gdist)) + (w_orient * (eth * eth))) * a.w_terminal;   // py:268
  a.cost[b] = total;
}

// K4: carrot selection, one wavefront per robot.  Lanes stride over the plan poses (24 B each,
// consecutive lanes read consecutive poses: one contiguous 1.5 KB segment per wave load), so the
// kernel streams the plans once for the closest-pose search (cpp:83-88) and re-reads only the
// kept window [begin, end) for the cut-off and look-ahead scans (cpp:102-106, 177-186).
__global__ __launch_bounds__(kLanes) void k_carrot(const CarrotArgs a) {
  const int lane = threadIdx.x;
  const size_t b = blockIdx.x;
  if (b >= a.b.count) return;
  const uint32_t o0 = a.b.plan_offsets[b], np = a.b.plan_offsets[b + 1] - o0;
  const double* poses = a.b.plan_poses + 3 * (size_t)o0;
  const double rx = a.b.robot_poses[3 * b], ry = a.b.robot_poses[3 * b + 1], rth = a.b.robot_poses[3 * b + 2];
  int slow = a.b.slow_down[b];
  neo_mpc_carrot out;
  out.xy[0] = 0.0; out.xy[1] = 0.0; out.q[0] = 0.0; out.q[1] = 0.0; out.q[2] = 0.0; out.q[3] = 1.0;
  out.lookahead_dist = 0.0; out.begin = 0; out.end = 0; out.closer_to_goal = 0; out.slow_down = slow;
  out.status = 0; out.reserved = 0;
  if (np == 0) {                                                        // cpp:69-71
    out.status = 1;
    if (lane == 0) { a.b.carrots[b] = out; if (a.b.problems) a.b.problems[b].skip = 1; }   // (a throw: no request this tick)
    return;
  }
  // closest pose, first minimum (min_by, cpp:83-88): the stream K15 shares (plan_check.h)
  const uint32_t begin = closest_pose(poses, np, rx, ry, lane);
  out.closer_to_goal = hypot(poses[3 * (np - 1)] - rx, poses[3 * (np - 1) + 1] - ry) <=
                       a.lp.lookahead_dist_close_to_goal ? 1 : 0;       // cpp:95-100
  double la = a.lp.lookahead_dist_min;                                  // cpp:161-169
  if (!slow || out.closer_to_goal) {
    la = a.lp.lookahead_dist_max;
    if (out.closer_to_goal) la = a.lp.lookahead_dist_close_to_goal;
  }
  double sn, cs;
  sincos(rth, &sn, &cs);
  // one scan from `begin`: first pose beyond the costmap (cpp:102-106) and first pose at least the
  // look-ahead distance away in the base frame (cpp:177-181)
  uint32_t end = np, pick = 0xffffffffu;
  for (uint32_t base = begin; base < np; base += kLanes) {
    const uint32_t k = base + lane;
    bool far = false, hit = false;
    if (k < np) {
      const double dx = poses[3 * k] - rx, dy = poses[3 * k + 1] - ry;
      far = hypot(dx, dy) > a.lp.max_transform_dist;
      hit = hypot(cs * dx + sn * dy, -sn * dx + cs * dy) >= la;
    }
    const unsigned long long mfar = __ballot(far), mhit = __ballot(hit);
    if (pick == 0xffffffffu && mhit) pick = base + (uint32_t)__ffsll((long long)mhit) - 1;
    if (mfar) { end = base + (uint32_t)__ffsll((long long)mfar) - 1; break; }
  }
  out.begin = begin; out.end = end;
  if (end == begin) {                                                   // cpp:130-132
    out.status = 2;
    if (lane == 0) { a.b.carrots[b] = out; if (a.b.problems) a.b.problems[b].skip = 1; }
    return;
  }
  out.lookahead_dist = la;
  if (pick == 0xffffffffu || pick >= end) pick = end - 1;               // cpp:183-186
  const double dx = poses[3 * pick] - rx, dy = poses[3 * pick + 1] - ry;
  const double yaw_local = poses[3 * pick + 2] - rth;
  out.xy[0] = cs * dx + sn * dy; out.xy[1] = -sn * dx + cs * dy;
  double qs, qc;
  sincos(0.5 * yaw_local, &qs, &qc);
  out.q[2] = qs; out.q[3] = qc;
  const double cy = fabs(atan2(2.0 * qc * qs, 1.0 - 2.0 * qs * qs));  // createYawFromQuat (cpp:54-62)
  slow = (cy >= 1.0 && a.b.footprint_costs && a.b.footprint_costs[b] > 200.0) ? 1 : 0;   // cpp:221-232
  out.slow_down = slow;
  // cpp:234-236: a footprint cost of 255 makes the plugin throw here -- after the slow_down_ update, before the
  // optimizer request: this robot makes no request this tick
  const bool no_request = a.b.footprint_costs && a.b.footprint_costs[b] == 255.0;
  if (no_request) out.status = 3;
  if (lane == 0) {
    a.b.carrots[b] = out;
    a.b.slow_down[b] = slow;
    if (a.b.problems) {
      neo_mpc_problem* pr = a.b.problems + b;
      pr->carrot_xy[0] = out.xy[0]; pr->carrot_xy[1] = out.xy[1];
      pr->carrot_q[0] = 0.0; pr->carrot_q[1] = 0.0; pr->carrot_q[2] = qs; pr->carrot_q[3] = qc;
      pr->switch_opt = out.closer_to_goal;   // cpp:245
      pr->skip = no_request ? 1 : 0;
    }
  }
}

}  // namespace

// K1: the dense-Newton and L-BFGS rows of the dispatch table; the stage-wise and routed rows: neo_mpc_riccati.hip
void launch_solve_riccati(const SolveArgs& a, const LaunchTuning& tuning, void* stream, void* ev_start, void* ev_stop);

void launch_solve(const SolveArgs& a, const LaunchTuning& tuning, void* stream, void* ev_start, void* ev_stop) {
  if (a.count == 0) return;
  const bool generic = a.p.mem != 4;  // (the control_steps-3 L-BFGS specialisation carves LDS for four pairs)
  const K1Launch launch(a, tuning, stream, ev_start, ev_stop);   // (k1_solve.h: what both tables know before they pick a row)
  const bool disc = launch.disc, small_tile = launch.small_tile;
  const size_t lds = launch.lds;
  if (a.p.newton == 2) { launch_solve_riccati(a, tuning, stream, ev_start, ev_stop); return; }
  if (a.p.n == 3 && a.p.newton == 1) {  // projected Newton, dense 9 x 9 system (its layout does not depend on lbfgs_memory)
    // (the general variant at 4 waves/SIMD spills 7 VGPRs -- 32 bytes of scratch -- and is still the faster one: measured
    // on the "cut" parameter set, same box, tools/ab_general.py: 0.123 ms against 0.133 ms per 4096 instances at 3
    // waves/SIMD -- 4096 waves are one residency round at 4 --, 55.9 M against 51.3 M solves/s at 65 536)
    const int w = solve_variant(tuning, 4);
    if (a.p.routed) { launch_solve_riccati(a, tuning, stream, ev_start, ev_stop); return; }   // AUTO: direction by neighbourhood (k_solve_routed)
    if (disc && w == 4 && small_tile) launch(k_solve<4, 3, 1, true, 1024>, 0);   // (the static variant takes no dynamic LDS)
    else if (disc) launch(NEO_K1_BY_WAVES(w, k_solve, 3, 1, true), lds);
    else launch(NEO_K1_BY_WAVES(w, k_solve, 3, 1), lds);
  } else if (a.p.n == 3 && a.p.newton == 0 && !generic) {
    launch(NEO_K1_BY_WAVES(solve_variant(tuning, 3), k_solve, 3), lds);
  } else if (a.p.newton == 1) {  // control_steps <= kNewtonMaxSteps, dense system with run-time size
    // (a 24-entry row per lane: 158 VGPRs, 187 without the tame specialisation -- spill-free at 3 and 2 waves/SIMD)
    const int w = solve_variant(tuning, disc ? 3 : 2);
    if (disc && w == 3 && small_tile) launch(k_solve<3, 0, 1, true, 1024>, 0);
    else if (disc) launch(NEO_K1_BY_WAVES(w, k_solve, 0, 1, true), lds);
    else launch(NEO_K1_BY_WAVES(w, k_solve, 0, 1), lds);
  } else {  // projected L-BFGS, any control_steps
    const int w = solve_variant(tuning, 3);
    if (disc) launch(NEO_K1_BY_WAVES(w, k_solve, 0, 0, true), lds);
    else launch(NEO_K1_BY_WAVES(w, k_solve, 0, 0), lds);
  }
}
void launch_carrots(const CarrotArgs& a, void* stream) {
  if (a.b.count == 0) return;
  hipLaunchKernelGGL(k_carrot, dim3((unsigned)a.b.count), dim3(kLanes), 0, (hipStream_t)stream, a);
}
void launch_postprocess(const SolveArgs& a, void* stream) {
  if (a.count == 0) return;
  hipLaunchKernelGGL(k_postprocess, dim3(a.count), dim3(kLanes), a.lds.total_bytes, (hipStream_t)stream, a);
}
void launch_objective(const ObjectiveArgs& a, void* stream) {
  if (a.count == 0) return;
  hipLaunchKernelGGL(k_objective, dim3((a.count + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
}
// K5.  A launch of up to 4096 instances is one residency round: workgroups w, w + 1024, w + 2048 and w + 3072 share a SIMD
// (measured with the XCC id in the hardware key) and the SIMD with the largest sum of iterations ends the
// launch -- 23.5 iteration-slots against a mean of 13.9 in the closed loop of 4096 robots.  Robots keep their habits from one
// tick to the next (correlation of the iteration counts of consecutive ticks 0.79: stopped robots 2, cruising robots 3,
// robots along a wall 8 and more), so past counts predict this tick's load: instances sorted by them, longest first, and
// dealt over the 1024 SIMDs in snake order (slot 0 left to right, slot 1 right to left, ...) bring the maximum down to 21
// with the last tick's counts alone, to 20.3 with `load` = an exponential average over the calls (decay 1/2: the handle
// keeps it between calls; on the mirror's closed loop, the order rebuilt every 5th tick).  One workgroup, a counting sort
// over 512 bins of a quarter of an iteration; ranks among equals come from atomics (any order of equals is as good as
// another).  Counts that are not a multiple of 1024 or beyond 4096 (more than one round: the hardware deals waves as slots
// free up) get the identity.
__global__ __launch_bounds__(1024) void k_dispatch_order(const neo_mpc_command* commands, float* load, uint32_t* order,
                                                         uint32_t count, int fresh) {
  constexpr uint32_t kBins = 512;
  __shared__ uint32_t hist[kBins], scan[kBins];
  const uint32_t t = threadIdx.x;
  if (count % kDispatchSimds != 0 || count > 4 * kDispatchSimds) {
    for (uint32_t i = t; i < count; i += 1024) order[i] = i;
    return;
  }
  if (t < kBins) hist[t] = 0;
  __syncthreads();
  uint32_t key[4], rank[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t i = t + 1024u * k;
    if (i < count) {
      const int it = commands[i].iterations;
      const float now = (float)(it < 0 ? 0 : it > 127 ? 127 : it);
      const float e = fresh ? 2.0f * now : 0.5f * load[i] + now;     // (a fresh average starts at its steady state)
      load[i] = e;
      const uint32_t q = (uint32_t)fminf(2.0f * e + 0.5f, (float)(kBins - 1));   // (e is twice the count in the steady state)
      key[k] = kBins - 1u - q;                                        // ascending key = descending load
      rank[k] = atomicAdd(&hist[key[k]], 1u);
    }
  }
  __syncthreads();
  // exclusive prefix sum over the bins (Hillis-Steele, 9 steps, two buffers)
  uint32_t* src = hist;
  uint32_t* dst = scan;
  for (uint32_t d = 1; d < kBins; d <<= 1) {
    if (t < kBins) dst[t] = src[t] + (t >= d ? src[t - d] : 0u);
    __syncthreads();
    uint32_t* tmp = src; src = dst; dst = tmp;
  }
  // (src holds the inclusive sums)
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t i = t + 1024u * k;
    if (i < count) {
      const uint32_t pos = (key[k] ? src[key[k] - 1u] : 0u) + rank[k], slot = pos / kDispatchSimds;
      uint32_t lane = pos % kDispatchSimds;
      if (slot & 1u) lane = kDispatchSimds - 1u - lane;
      order[slot * kDispatchSimds + lane] = i;
    }
  }
}
void launch_dispatch_order(const neo_mpc_command* commands, float* load, uint32_t* order, uint32_t count, bool fresh, void* stream) {
  if (count == 0) return;
  hipLaunchKernelGGL(k_dispatch_order, dim3(1), dim3(1024), 0, (hipStream_t)stream, commands, load, order, count, fresh ? 1 : 0);
}
void launch_footprint_gate(const FootprintGateArgs& a, void* stream) {
  if (a.count == 0) return;
  hipLaunchKernelGGL(k_footprint_gate, dim3((a.count + kGateWaves - 1) / kGateWaves), dim3(kLanes * kGateWaves), 0,
                     (hipStream_t)stream, a);
}
// K7: origins and index tables first (one wave per window), then the fill -- two launches, so that a window's new origin is
// final before any workgroup fills that window
void launch_roll(const RollArgs& a, void* stream) {
  if (a.count == 0) return;
  hipLaunchKernelGGL(k_roll_index, dim3((a.count + kRollWaves - 1) / kRollWaves), dim3(kLanes * kRollWaves), 0,
                     (hipStream_t)stream, a);
  hipLaunchKernelGGL(k_roll_fill, padded_map_grid(a.rows, a.pitch, kRollUnroll, a.count), dim3(256), 0, (hipStream_t)stream, a);
}
// K8: polygons and bounding boxes first (one thread per robot), then one wave per window -- two launches, so that every box is
// final before any window searches the fleet
void launch_stamp(const StampArgs& a, void* stream) {
  if (a.count == 0) return;
  hipLaunchKernelGGL(k_stamp_boxes, dim3((a.count + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(k_stamp_fleet, dim3(a.count), dim3(kLanes), 0, (hipStream_t)stream, a);
}
// K9: one workgroup per tile of 64 x 64 cells of the world map
void launch_inflate_world(const InflateArgs& a, void* stream) {
  if (a.wsx <= 0 || a.wsy <= 0) return;
  hipLaunchKernelGGL(k_inflate_world, dim3((a.wsx + kInflateTile - 1) / kInflateTile, (a.wsy + kInflateTile - 1) / kInflateTile),
                     dim3(kLanes * kInflateWaves), 0, (hipStream_t)stream, a);
}
// K10: the shift, then the clears, then the marks, then the windows -- four launches on one stream, each behind the one before:
// every layer is in place before a ray touches it, every clear before every mark, every mark before the seeds are read
void launch_scan_layer(const ScanArgs& a, void* stream) {
  if (a.count == 0) return;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_scan_shift, dim3((a.size_y + kScanShiftRows - 1) / kScanShiftRows, a.count), dim3(256), 0, st, a);
  const dim3 rays((a.max_points + kScanRayThreads - 1) / kScanRayThreads, a.count);
  if (a.max_points > 0 && (a.flags & NEO_MPC_SCAN_CLEAR)) hipLaunchKernelGGL(k_scan_rays<false>, rays, dim3(kScanRayThreads), 0, st, a);
  if (a.max_points > 0 && (a.flags & NEO_MPC_SCAN_MARK)) hipLaunchKernelGGL(k_scan_rays<true>, rays, dim3(kScanRayThreads), 0, st, a);
  hipLaunchKernelGGL(k_scan_apply, dim3((a.size_x + kInflateTile - 1) / kInflateTile, (a.size_y + kInflateTile - 1) / kInflateTile, a.count),
                     dim3(kLanes * kInflateWaves), 0, st, a);
}
// K11: one workgroup per robot and source
void launch_laser_project(const LaserArgs& a, void* stream) {
  if (a.count == 0) return;
  hipLaunchKernelGGL(k_laser_project, dim3(a.count, a.sources), dim3(kLaserThreads), 0, (hipStream_t)stream, a);
}
// K12: the reset (a fill), every clear of every robot, every mark, the footprints, then the composition -- each behind the one
// before on one stream: every mark lies behind every clear, the footprints behind every mark, the seeds are final when read.
// With the speckle filter on (K13), one more launch in front of the composition, which then reads D where it reads the layer;
// the window compiled in is the smallest of 3, 7, 15 and 31 rows that holds G - 1 steps either way.
// With decay on (K14): on the first such update the fill of `stamp`, in front of everything; in a scan update -- MARK in the
// flags, count > 0 -- the tick in front of the marks, which then stamp what they mark; and in every update the sweep between the
// marks and the footprints.  With decay off none of the four is enqueued and the marking launch is K12a's.
void launch_world_scan(const WorldScanArgs& a, void* stream) {
  if (a.wsx <= 0 || a.wsy <= 0) return;
  hipStream_t st = (hipStream_t)stream;
  if (a.reset) (void)hipMemsetAsync(a.layer, (int)a.s.unknown, (size_t)a.wsx * (size_t)a.wsy, st);
  const dim3 rays((a.s.max_points + kScanRayThreads - 1) / kScanRayThreads, a.s.count);
  const bool any = a.s.count > 0 && a.s.max_points > 0;
  if (any && (a.s.flags & NEO_MPC_SCAN_CLEAR)) hipLaunchKernelGGL(k_world_scan_rays<false>, rays, dim3(kScanRayThreads), 0, st, a);
  if (a.max_age == 0u) {
    if (any && (a.s.flags & NEO_MPC_SCAN_MARK)) hipLaunchKernelGGL(k_world_scan_rays<true>, rays, dim3(kScanRayThreads), 0, st, a);
  } else {
    const int64_t cells = (int64_t)a.wsx * a.wsy;
    const int64_t fill = (cells >> 2) + (cells & 3), sweep = cells / kDecayCells + cells % kDecayCells;   // lanes: < 2^31 * 256
    if (a.stamp_fresh) hipLaunchKernelGGL(k_world_scan_stamp_fill, dim3((uint32_t)((fill + kDecayThreads - 1) / kDecayThreads)), dim3(kDecayThreads), 0, st, a);
    if (a.s.count > 0 && (a.s.flags & NEO_MPC_SCAN_MARK)) {
      hipLaunchKernelGGL(k_world_scan_tick, dim3(1), dim3(kLanes), 0, st, a);
      if (any) hipLaunchKernelGGL(k_world_scan_marks_stamped, rays, dim3(kScanRayThreads), 0, st, a);
    }
    hipLaunchKernelGGL(k_world_scan_decay, dim3((uint32_t)((sweep + kDecayThreads - 1) / kDecayThreads)), dim3(kDecayThreads), 0, st, a);
  }
  if (a.clear && a.s.count > 0) hipLaunchKernelGGL(k_world_scan_footprints, dim3(a.s.count), dim3(kLanes), 0, st, a);
  const dim3 tiles((a.wsx + kInflateTile - 1) / kInflateTile, (a.wsy + kInflateTile - 1) / kInflateTile), tile(kLanes * kInflateWaves);
  if (a.group < 2u) { hipLaunchKernelGGL(k_world_scan_compose, tiles, tile, 0, st, a); return; }
  if (a.group <= 2u) hipLaunchKernelGGL(k_world_scan_denoise<1>, tiles, tile, 0, st, a);
  else if (a.group <= 4u) hipLaunchKernelGGL(k_world_scan_denoise<3>, tiles, tile, 0, st, a);
  else if (a.group <= 8u) hipLaunchKernelGGL(k_world_scan_denoise<7>, tiles, tile, 0, st, a);
  else hipLaunchKernelGGL(k_world_scan_denoise<15>, tiles, tile, 0, st, a);
  WorldScanArgs filtered = a;
  filtered.layer = a.denoised;
  hipLaunchKernelGGL(k_world_scan_compose, tiles, tile, 0, st, filtered);
}
// K15: one wave per plan; the mode is the kernel's (a polygon or none: uniform over the launch)
void launch_plan_check(const PlanCheckArgs& a, void* stream) {
  if (a.count == 0) return;
  if (a.footprint_points != 0) hipLaunchKernelGGL(k_plan_check<true>, dim3(a.count), dim3(kLanes), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(k_plan_check<false>, dim3(a.count), dim3(kLanes), 0, (hipStream_t)stream, a);
}
// K16: one workgroup per robot; the kernel's static LDS follows the window (7.9 KB to 32, 30 KB to 64, 115 KB to 128 cells)
void launch_replan(const ReplanArgs& a, void* stream) {
  if (a.count == 0) return;
  const dim3 grid(a.count), block(kReplanThreads);
  if (a.window <= 32) hipLaunchKernelGGL(k_replan<32>, grid, block, 0, (hipStream_t)stream, a);
  else if (a.window <= 64) hipLaunchKernelGGL(k_replan<64>, grid, block, 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(k_replan<128>, grid, block, 0, (hipStream_t)stream, a);
}
void launch_ingest(const IngestArgs& a, const LaunchTuning& tuning, void* stream) {
  hipLaunchKernelGGL(k_ingest, padded_map_grid(a.rows, a.pitch, kIngestUnroll, a.maps > 0 ? a.maps : 1), dim3(256), 0,
                     (hipStream_t)stream, a);
}

}  // namespace neo_mpc
