// neo_mpc_device.h -- host/device shared argument blocks of the gfx950 kernels.
// Internal to libneo_mpc.so (the public surface is include/neo_mpc.h).
#pragma once
#include <stdint.h>

#include "../../include/neo_mpc.h"
#include "solver_rules.h"

namespace neo_mpc {

constexpr int kLanes = 64;          // one CDNA4 wavefront per MPC instance
constexpr int kMapBorder = 64;      // lethal border (cells) K3 adds around a single costmap
constexpr int kPoolBorder = 16;     // ... around each map of a pool (every lookup is bounds-checked anyway)
constexpr int kMaxTileWidth = NEO_RULE_MAX_TILE_WIDTH;  // widest reach tile staged in LDS (bytes per row; solver_rules.h)
constexpr int kCompatNoUnshift = 0x10000;   // DevParams.compat (internal bit): searches always start at the warm start (NEO_MPC_COMPAT_REFERENCE_START)
constexpr int kDumpGradient = 0x40000000;  // DevParams.max_it value of the gradient test hook (neo_mpc_gradient_batch)

// Constants of one solver configuration, precomputed on the host in float64 exactly as
// the reference evaluates them (mpc_optimization_server.py:137, 252-268).
struct DevParams {
  double dt;                 // prediction_horizon / control_steps (py:137)
  double wt_n, wo_n, wc_n;   // w_trans/N, w_orient/N, w_control/N (py:252-254)
  double wterm_o;            // w_terminal * w_orient (py:268)
  double wterm_t;            // w_terminal * w_trans  (py:268, constant in u)
  double w_footprint;        // py:263 (constant in u)
  double lo[3], hi[3];       // box bounds vx, vy, omega (py:127-133)
  double r;                  // max_vel_trans (py:158)
  double acc[3];             // post clamp (py:385-391)
  double low_pass_gain;      // py:367
  double xtol;               // step tolerance
  double early_tol;          // Newton: stop when the full step is below this (= xtol; 0 disables, A/B)
  double final_tol;          // Newton: a full step below this is the last one (= opt_tolerance)
  double ftol;               // relative cost decrease below which an iteration counts as stalled
  double stall_step;         // ... or max|du| below this
  double wtol;               // three iterations in a row gaining less than this (relative) end the search; 0: off
  double wtol_late;          // ... the same from iteration kLateIteration on (the control_steps-3 window)
  double kink_radius;        // |u_i - v_cur| below which a block is handled by the prox step only
  double kink_radius_stagewise;  // ... for the instances the routed kernel sends to the stage-wise direction
  double btol_map, btol_free;  // dense Newton direction: kBlockedRun consecutive iterations not won by a decent Newton step that
                             // together gain less than this end the search (with / without a costmap term under the rollout); 0: off
  double hop_min_drop;       // stage-wise direction: a cheaper neighbour cell is worth a hop candidate when its costmap
                             // term is lower by more than this (0.1 * opt_tolerance)
  double hop_range;          // ... and its edge is closer than this (cells): min(0.25, 0.05 m/s * dt / resolution)
  double scan_resume_gain;   // cell scan (cell_scan.h): the search is taken up again behind a scan that gained more than this
  int32_t n;                 // control_steps
  int32_t max_it;
  int32_t mem;               // L-BFGS pairs
  int32_t compat;
  int32_t disc_in_box;       // the max_vel_trans disc lies inside the vx/vy box (README params)
  int32_t tame;              // disc_in_box and max|omega| * horizon <= 0.78 rad: the kTame kernels apply
  int32_t scan_reach;        // cell scan: no cell further than this from the robot's own cell (= the reach tile's radius)
  int32_t newton;            // search direction of lanes 32-63: 0 projected L-BFGS, 1 projected Newton with
                             // the dense system (control_steps <= 8), 2 projected Newton by the Riccati sweep
  int32_t routed;            // direction by neighbourhood (AUTO at control_steps 3, solver_rules.h): `newton` is the direction of
                             // the instances whose reach tile is all free, the others take the stage-wise one (k_solve_routed)
};

// Device costmap written by the ingest kernel (K3): raw nav2 costs with a lethal border of
// kMapBorder cells and a 128-byte row pitch; `cells` points at cell (0, 0).
struct DevMap {
  const uint8_t* cells;
  int32_t size_x, size_y;
  int32_t pitch;
  double resolution, inv_resolution, origin_x, origin_y;
  // costmap pool (neo_mpc_set_costmap_pool): pool_count bordered maps of this geometry back to back,
  // pool_stride bytes apart, their origins in pool_origins[2k], [2k+1]; 0: the single map above
  int32_t pool_count;
  int32_t border;    // lethal cells around the map in device memory (multiple of 16)
  int64_t pool_stride;
  const double* pool_origins;
};

// LDS carve-up of the solve kernel, in doubles from the start of dynamic LDS.
struct LdsLayout {
  int32_t prob, state, tol, term, u, gs, gt, gr, d, u_prev, gt_prev, u_new, S, Y, rho;
  int32_t cs, sn, dxs, dys, rx, ry, rt, nx, ny, mode;  // per-step scratch
  int32_t hess;        // Newton: (3N)^2 Hessian, only when 3N <= 24
  int32_t ric;         // Riccati: float32 stage records (28 N floats; the gains overwrite part of them), riccati.h
  int32_t keep;        // Riccati: the 12 N floats the gains overwrite, kept for a second sweep (riccati_keep_linear_terms)
  int32_t tile;        // byte tile starts here (double index)
  int32_t total_bytes;
  int32_t tile_w;      // row stride of the tile in bytes (power of two), 0: no tile
  int32_t tile_h;      // rows
  int32_t reach;       // R: the tile spans [m0 - R, m0 + R]
};

// The carve-up depends on control_steps and the L-BFGS memory only, so the control_steps
// specialisations of K1 evaluate it at compile time (offsets become immediates); the host uses the
// same function and adds the reach tile geometry.
// corners: the feasible set has corners (the vx/vy box cuts the max_vel_trans disc) -- the Riccati kernel then keeps room
// for a second sweep with another active set.
constexpr LdsLayout make_lds_layout(int n, int mem, bool riccati, bool corners = false) {
  LdsLayout l{};
  const int nv = 3 * n;
  int off = 0;
  l.prob = off; off += 32;
  l.state = off; off += 16;
  l.tol = off; off += 32;   // (= kTolDoubles, solver_context.h) stop tolerances + two cold per-instance constants (read once per iteration; kept out of the scalar
                            // registers), then the hop candidates of the current iteration (solver_context.h)
  l.term = off; off += 256;
  l.u = off; off += nv;
  l.gs = off; off += nv;
  l.gt = off; off += nv;
  l.gr = off; off += nv;
  // (Riccati: the direction takes the place of the total gradient -- the sweep has consumed it before the
  // forward pass writes d, and the next tangent-cone pass rewrites it after the candidates have read d)
  if (riccati) l.d = l.gt;
  else { l.d = off; off += nv; }
  if (riccati) {
    // the Riccati kernel keeps no previous iterate / gradient and no quasi-Newton pairs; the winner is
    // staged where the reduced gradient lived (disjoint lifetimes inside an iteration); of the per-step
    // float64 scratch it uses nx, ny and rt (disc curvature) only; its stage records and gains are float32
    l.u_new = l.gr;
    l.u_prev = l.u; l.gt_prev = l.u; l.S = off; l.Y = off; l.rho = off;
    l.cs = off; l.sn = off; l.dxs = off; l.dys = off; l.rx = off; l.ry = off;
    l.rt = off; off += n;
    l.nx = off; off += n;
    l.ny = off; off += n;
    l.mode = off; off += 2 * n;
    l.hess = off;
    off = (off + 1) & ~1;                   // (16-byte aligned: the records are read as 16-byte words)
    l.ric = off; off += 14 * n;             // 28 floats per stage, riccati.h
    l.keep = off; off += corners ? 6 * n : 0;   // (16-byte aligned: 14 n is even)
  } else {
    l.u_prev = off; off += nv;
    l.gt_prev = off; off += nv;
    l.u_new = off; off += nv;
    l.S = off; off += mem * nv;
    l.Y = off; off += mem * nv;
    l.rho = off; off += NEO_MPC_MAX_LBFGS_MEMORY;
    l.cs = off; off += n;
    l.sn = off; off += n;
    l.dxs = off; off += n;
    l.dys = off; off += n;
    l.rx = off; off += n;
    l.ry = off; off += n;
    l.rt = off; off += n;
    l.nx = off; off += n;
    l.ny = off; off += n;
    l.mode = off; off += 2 * n;  // int[4n]: mode, omega-frozen, near-kink, near-kink at the previous iterate
    l.hess = off; off += (nv <= 24) ? nv * nv : 0;
    l.ric = off;
    l.keep = off;
  }
  off = (off + 1) & ~1;        // 16-byte align the tile
  l.tile = off;
  l.total_bytes = off * 8;
  return l;
}

struct SolveArgs {
  const neo_mpc_problem* problems;
  neo_mpc_state* states;
  double* warm;
  neo_mpc_command* commands;
  double* solution;        // optional
  double* path;            // optional
  const double* footprints;  // optional
  const int32_t* success;    // postprocess only, optional
  double* velocities;        // optional packed [count][3] copy of the commands
  neo_mpc_state* states_out; // where K2 writes the state / the warm start back: the arrays they were read from
  double* warm_out;          // (device batches), or the caller's page-locked host arrays (neo_mpc_solve_batch)
  const double* term_table;  // [256] per-step costmap term by raw cell value
  const uint32_t* order;     // optional: workgroup w solves instance order[w] (neo_mpc_balance_dispatch_device); null: w
  uint32_t footprint_points;
  uint32_t count;
  DevParams p;
  DevMap map;
  LdsLayout lds;
};

struct ObjectiveArgs {
  const neo_mpc_problem* problems;
  const double* u;
  double* cost;
  const double* term_table;
  uint32_t count;
  DevParams p;
  DevMap map;
  double w_trans, w_orient, w_control, w_terminal, w_costmap;   // undivided, as the reference uses them (py:252-268)
};

struct IngestArgs {
  const uint8_t* src;  // raw nav2 costmap(s), row-major size_x * size_y each, back to back
  uint8_t* dst;        // padded map base (row 0 of the border) of the first map
  int32_t size_x, size_y, pitch, rows;  // rows = size_y + 2*border
  int32_t maps;        // number of maps (blockIdx.y)
  int32_t border;
  int64_t dst_stride;  // bytes between padded maps
};

struct CarrotArgs {
  neo_mpc_lookahead_params lp;
  neo_mpc_plan_batch b;  // device pointers
};

// K6: the footprint gate (neo_mpc_footprint_batch, device pointers) on the handle's map(s)
struct FootprintGateArgs {
  const double* footprint;     // [points][2], or [count][points][2] with per_robot
  const double* poses;         // optional [count][3]
  const int32_t* map_indices;  // optional [count]
  neo_mpc_problem* problems;   // optional [count]
  double* footprint_costs;     // [count]
  double* footprints_out;      // optional [count][points][2]
  uint32_t count;
  uint32_t footprint_points;
  uint32_t per_robot;
  DevMap map;
};

// K7: the rolling windows (neo_mpc_window_batch, device pointers) cut from the handle's world map into its map pool
struct RollArgs {
  const double* poses;              // optional [count][3]
  const neo_mpc_problem* problems;  // optional [count], read when poses is null
  double* origins;                  // [count][2] in/out
  int32_t* tables;                  // [count][tab_stride] handle-owned: the fill's column and row indices (rolling_window.h)
  const uint8_t* world;             // the world map, row-major wsx * wsy
  uint8_t* dst;                     // padded map base (row 0 of the border) of the first window
  double res, wres, wox, woy;
  int64_t dst_stride;               // bytes between padded maps
  int32_t wsx, wsy;
  int32_t size_x, size_y, pitch, rows;  // rows = size_y + 2*border
  int32_t border;
  int32_t tab_x, tab_stride;        // column entries per window (size_x rounded up to 16), entries per window
  uint32_t count;
  uint32_t outside;                 // outside_value
};

// K8: the fleet's robots stamped into each other's windows (neo_mpc_stamp_batch, device pointers) -- the handle's map pool
struct StampArgs {
  const double* polygons;           // [count][points][2] global frame, or null: footprint + poses / problems
  const double* footprint;          // [points][2], or [count][points][2] with per_robot
  const double* poses;              // optional [count][3]
  const neo_mpc_problem* problems;  // optional [count], read when poses is null
  double* polys;                    // [count][points][2] handle-owned: the oriented polygons (written without `polygons`)
  double* boxes;                    // [count][4] handle-owned: the polygons' bounding boxes, min x, min y, max x, max y
  const uint8_t* table;             // [reach^2 + 1]: cost by squared cell distance (neo_mpc_inflation_costs)
  uint8_t* cells;                   // cell (0, 0) of the first window
  const double* origins;            // [count][2]
  double res;
  int64_t stride;                   // bytes between windows
  int32_t size_x, size_y, pitch;
  int32_t reach;                    // R, cells: 0 .. NEO_MPC_MAX_INFLATION_CELLS
  uint32_t count;
  uint32_t points;
  uint32_t per_robot;
};

// K9: nav2's inflation layer on the handle's copy of the world map (neo_mpc_inflate_world_map), in place
struct InflateArgs {
  uint8_t* world;                   // the world map, row-major wsx * wsy: read and rewritten
  const uint8_t* table;             // [reach^2 + 1]: cost by squared cell distance (neo_mpc_inflation_costs at the world's resolution)
  int32_t wsx, wsy;
  int32_t reach;                    // R, cells: 0 .. NEO_MPC_MAX_INFLATION_CELLS
};

// K10: the scan obstacle layer (neo_mpc_scan_batch, device pointers) -- the handle's map pool and its two layer buffers
struct ScanArgs {
  const double* points;             // [count][max_points][2] global frame (read with NEO_MPC_SCAN_CLEAR / _MARK only)
  const uint32_t* point_counts;     // optional [count]
  const double* sensor_origins;     // [count][sources][2]: point p of a robot was seen from its source p / points_per_source
  const uint8_t* table;             // [reach^2 + 1]: cost by squared cell distance (neo_mpc_inflation_costs)
  uint8_t* layer;                   // handle-owned: the layers between updates, layer_pitch bytes a row, no border
  uint8_t* work;                    // handle-owned: this update's layers, same shape
  double* layer_origins;            // [count][2] handle-owned: where the layers of `layer` lie
  uint8_t* cells;                   // cell (0, 0) of the first window
  const double* origins;            // [count][2]
  double res;
  double obstacle_max, obstacle_min, raytrace_max, raytrace_min;
  int64_t stride;                   // bytes between windows
  int64_t layer_stride;             // bytes between layers
  int32_t size_x, size_y, pitch;
  int32_t layer_pitch;              // size_x rounded up to 64
  int32_t reach;                    // R, cells: 0 .. NEO_MPC_MAX_INFLATION_CELLS
  uint32_t count;
  uint32_t max_points;
  uint32_t sources;                 // K10: 1; K11: the scanners of a robot
  uint32_t points_per_source;       // K10: max_points (every point is source 0's); K11: beams, max_points = sources * beams
  uint32_t flags;                   // NEO_MPC_SCAN_*
  uint32_t unknown;                 // 0 or 255
  uint32_t reset;                   // 1: the layers start from `unknown` at the windows' origins
};

// K12: the fleet's shared obstacle layer on the world map (neo_mpc_update_world_scan_layer, device pointers) -- the handle's
// world map, its layer and the map the roll reads; every row of the three is wsx bytes
struct WorldScanArgs {
  ScanArgs s;                       // the rays as K10 takes them (count: robots; flags, ranges, sources) and table / reach at wres
  uint8_t* layer;                   // handle-owned: the layer, {255, 0, 254}, persistent
  const uint8_t* world;             // the static world map
  uint8_t* live;                    // handle-owned: the world map with the layer merged in and inflated
  uint8_t* denoised;                // K13, handle-owned: D, the layer as the composition reads it (null with group < 2)
  uint32_t* stamp;                  // K14, handle-owned: [wsy][wsx] the clock when the cell was last marked (null with max_age == 0)
  uint32_t* clock;                  // K14, handle-owned: the scan updates so far, advanced on the device (null with max_age == 0)
  const double* polygons;           // fleet footprint clearing (neo_mpc_fleet_clear): as StampArgs; all null with clear == 0
  const double* footprint;
  const double* poses;
  const neo_mpc_problem* problems;
  double padding;                   // m
  double wres, wox, woy;
  int32_t wsx, wsy;
  uint32_t points;                  // footprint_points
  uint32_t per_robot;
  uint32_t clear;                   // 1: step 3 runs
  uint32_t reset;                   // 1: the layer starts from s.unknown
  uint32_t group;                   // K13: G, 2 .. NEO_MPC_MAX_DENOISE_GROUP; 0: the filter is off and step 3b is not launched
  uint32_t connectivity;            // K13: 4 or 8
  uint32_t max_age;                 // K14: A, scan updates; 0: decay is off and nothing of step 2b is launched
  uint32_t stamp_fresh;             // K14: 1: the first update with decay on, `stamp` is filled with the clock first
};

// K11: LaserScan ranges projected into global-frame points and sensor origins (neo_mpc_laser_batch, device pointers)
struct LaserSource {                // one neo_mpc_scanner as the kernel needs it
  double mount_x, mount_y;
  double range_min, range_max;
  double inf_range;                 // range_max - 1e-4, formed on the host in float64
  uint32_t inf_is_valid;            // NEO_MPC_LASER_INF_IS_VALID
  uint32_t pad;
};
struct LaserArgs {
  const float* ranges;              // [count][sources][beams]
  const double* poses;              // [count][3]
  const double* table;              // [sources][beams][2] handle-owned: cos, sin of every beam's angle in the base frame
  double* points;                   // [count][sources][beams][2], 16-byte aligned
  double* origins;                  // [count][sources][2]
  LaserSource source[NEO_MPC_MAX_SCAN_SOURCES];
  uint32_t count, sources, beams;
};

// K15: the plan check (neo_mpc_plan_check_batch, device pointers) on the world map the next roll would read
struct PlanCheckArgs {
  const double* plan_poses;         // [plan_offsets[count]][3]
  const uint32_t* plan_offsets;     // [count + 1]
  const double* robot_poses;        // optional [count][3]; null: every check starts at pose 0
  const double* footprint;          // [footprint_points][2] base frame, shared; null: point mode
  neo_mpc_plan_check* results;      // [count]
  const uint8_t* world;             // the world map or K12's composition, row-major wsx * wsy
  double wres, winv, wox, woy;      // winv = 1 / wres (cell_of redoes the division where it matters)
  int32_t wsx, wsy;
  uint32_t count;
  uint32_t footprint_points;        // 0: point mode
  uint32_t max_cost, unknown_blocks, outside, max_poses;
};

// K16: the grid planner (neo_mpc_replan_batch, device pointers) on the map K15 reads
struct ReplanArgs {
  const double* starts;             // [count][2]
  const double* goals;              // [count][2]
  const neo_mpc_plan_check* checks; // optional [count]: K15's records as a mask
  int32_t* path_cells;              // [count][max_path_cells][2]
  double* path_poses;               // optional [count][max_path_cells][3]
  neo_mpc_replan* results;          // [count]
  const uint8_t* world;             // the world map or K12's composition, row-major wsx * wsy
  double wres, winv, wox, woy;      // winv = 1 / wres (cell_of redoes the division where it matters)
  int32_t wsx, wsy;
  uint32_t count;
  uint32_t window;                  // 4 .. 128
  uint32_t max_cost, unknown_cost, neutral_cost, max_path_cells;
};

// A/B switches of the measurement tools: read from the environment ONCE, by neo_mpc_create (include/neo_mpc.h), kept in
// the handle -- nothing on the solve path looks at the environment.
struct LaunchTuning {
  int solve_waves = 0;         // NEO_MPC_SOLVE_WAVES=2|3|4: occupancy variant of K1 (0: what was measured fastest)
  bool no_tame = false;        // NEO_MPC_NO_TAME_SPECIALISATION: the general kernels for README-like parameters too
  bool dynamic_lds = false;    // NEO_MPC_DYNAMIC_LDS: the dynamic-LDS build of the control_steps specialisations
};

void launch_solve(const SolveArgs& a, const LaunchTuning& t, void* stream, void* ev_start = nullptr, void* ev_stop = nullptr);
void launch_carrots(const CarrotArgs& a, void* stream);
void launch_postprocess(const SolveArgs& a, void* stream);
void launch_objective(const ObjectiveArgs& a, void* stream);
void launch_ingest(const IngestArgs& a, const LaunchTuning& t, void* stream);
void launch_footprint_gate(const FootprintGateArgs& a, void* stream);
void launch_roll(const RollArgs& a, void* stream);   // K7: k_roll_index, then k_roll_fill
void launch_stamp(const StampArgs& a, void* stream); // K8: k_stamp_boxes, then k_stamp_fleet
void launch_inflate_world(const InflateArgs& a, void* stream);   // K9: k_inflate_world
void launch_scan_layer(const ScanArgs& a, void* stream);         // K10: k_scan_shift, k_scan_rays (clear, mark), k_scan_apply
void launch_laser_project(const LaserArgs& a, void* stream);     // K11: k_laser_project
void launch_world_scan(const WorldScanArgs& a, void* stream);    // K12: k_world_scan_rays (clear, mark), [K14: k_world_scan_decay,] k_world_scan_footprints, [K13: k_world_scan_denoise,] k_world_scan_compose
void launch_plan_check(const PlanCheckArgs& a, void* stream);    // K15: k_plan_check (point or footprint mode)
void launch_replan(const ReplanArgs& a, void* stream);           // K16: k_replan (a window of up to 32, 64 or 128 cells)
// K5: dispatch order of the next launch from the iteration counts of the previous one (neo_mpc_balance_dispatch_device)
void launch_dispatch_order(const neo_mpc_command* commands, float* load, uint32_t* order, uint32_t count, bool fresh, void* stream);
constexpr uint32_t kDispatchSimds = 1024;   // a 4096-instance launch is one residency round: workgroups w, w + 1024, w + 2048, w + 3072 share a SIMD

}  // namespace neo_mpc
