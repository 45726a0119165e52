"""Binary layout shared by the Python host side and the C-ABI (`include/neo_mpc.h`).

The records mirror the fields of the reference's ``neo_srvs2/srv/Optimizer`` request
and response (call sites src/NeoMpcPlanner.cpp:240-252 and
neo_mpc_planner2/mpc_optimization_server.py:349-403) plus the per-node state the
reference keeps between calls (mpc_optimization_server.py:115-152).
All floating point fields are float64, like the ROS messages.
"""
import collections
import ctypes as _C

import numpy as np

#: field type code -> (ctypes type, NumPy type); a pointer and a size_t are 8-byte addresses on the NumPy side
_TYPES = {"f8": (_C.c_double, "<f8"), "i4": (_C.c_int32, "<i4"), "u4": (_C.c_uint32, "<u4"), "u8": (_C.c_uint64, "<u8"),
          "ptr": (_C.c_void_p, "<u8"), "size": (_C.c_size_t, "<u8")}

Record = collections.namedtuple("Record", "struct dtype size")
#: every record struct of include/neo_mpc.h by its C name -> (ctypes.Structure, NumPy dtype, sizeof in bytes)
RECORDS = {}


def _record(c_name, size, doc, fields):
    """One record of include/neo_mpc.h, declared once: `fields` = (name, type code[, array length]) in the header's order,
    `size` its sizeof there.  Enters it in RECORDS -> (its ctypes.Structure, its NumPy dtype)."""
    ctypes_fields = [(f[0], _TYPES[f[1]][0] * f[2] if len(f) > 2 else _TYPES[f[1]][0]) for f in fields]
    struct = type("NeoMpc" + c_name[len("neo_mpc_"):].title().replace("_", ""), (_C.Structure,),
                  {"_fields_": ctypes_fields, "__doc__": doc})
    dtype = np.dtype([(f[0], _TYPES[f[1]][1]) + tuple((n,) for n in f[2:]) for f in fields], align=False)
    assert _C.sizeof(struct) == dtype.itemsize == size, c_name
    RECORDS[c_name] = Record(struct, dtype, size)
    return struct, dtype


NeoMpcParams, _ = _record("neo_mpc_params", 232, """`neo_mpc_params` (include/neo_mpc.h): the reference node's ROS parameters, same
    names (mpc_optimization_server.py:49-75), then the build's solver options.""", [(n, "f8") for n in (
        "acc_x_limit", "acc_y_limit", "acc_theta_limit",
        "min_vel_x", "min_vel_y", "min_vel_trans", "min_vel_theta",
        "max_vel_x", "max_vel_y", "max_vel_trans", "max_vel_theta",
        "w_trans", "w_orient", "w_control", "w_terminal", "w_costmap", "w_footprint",
        "waiting_time", "low_pass_gain", "opt_tolerance", "prediction_horizon")] + [
        ("control_steps", "i4"), ("max_iterations", "i4"),
        ("lbfgs_memory", "i4"), ("compat_flags", "i4"),
        ("step_tolerance", "f8"), ("cost_tolerance", "f8"),
        ("kink_radius", "f8"), ("stall_step", "f8"),
        ("method", "i4"), ("reserved_i", "i4"),
        ("window_tolerance", "f8")])
ROS_PARAM_NAMES = tuple(n for n, _ in NeoMpcParams._fields_[:22])

#: one Optimizer.srv request -> `neo_mpc_problem` (256 bytes)
_, PROBLEM_DTYPE = _record("neo_mpc_problem", 256, "`neo_mpc_problem` (include/neo_mpc.h): one Optimizer.srv request.", [
    ("cur_xy", "f8", 2),            # request.current_pose.pose.position.{x,y}   (costmap frame)
    ("cur_q", "f8", 4),             # request.current_pose.pose.orientation x,y,z,w
    ("carrot_xy", "f8", 2),         # request.carrot_pose.pose.position.{x,y}    (base frame)
    ("carrot_q", "f8", 4),          # request.carrot_pose.pose.orientation x,y,z,w
    ("goal_xyz", "f8", 3),          # request.goal_pose.position x,y,z           (plan frame)
    ("goal_q", "f8", 4),            # request.goal_pose.orientation x,y,z,w
    ("cur_vel", "f8", 3),           # request.current_vel linear.x, linear.y, angular.z
    ("control_interval", "f8"),     # request.control_interval = 1/controller_frequency
    ("delta_t", "f8"),              # wall-clock seconds since the previous call (py:369-371)
    ("footprint_cost", "f8"),       # getFootprintCost(published footprint), normalised; used when
                                    # no polygon is supplied (py:262, 343)
    ("map_index", "i4"),            # which costmap of a pool (BatchSolver.set_costmap_pool); else ignored
    ("switch_opt", "i4"),           # request.switch_opt (cpp:245; stored py:354, never read)
    ("skip", "i4"),                 # 1: no request is made for this robot this tick (cpp:234-236); state untouched.  0: solve.
                                    # Anything else: host batches are refused, device batches solve the robot (include/neo_mpc.h)
    ("reserved_i", "i4"),
    ("reserved", "f8", 5),
])

#: per-instance persistent node state -> `neo_mpc_state` (128 bytes); the warm start
#: (py:136 `initial_guess`) is a separate float64[3*control_steps] row per instance.
_, STATE_DTYPE = _record("neo_mpc_state", 128, "`neo_mpc_state` (include/neo_mpc.h): what the node keeps between requests.", [
    ("last_control", "f8", 3),      # py:117
    ("old_goal", "f8", 7),          # py:146 / py:402: goal position xyz + orientation xyzw
    ("waiting_time", "f8"),         # py:103, 361, 378-382
    ("has_old_goal", "i4"),         # 0 until the first call (py:146 PoseStamped != Pose)
    ("collision", "i4"),            # py:148 latch
    ("collision_footprint", "i4"),  # py:149
    ("has_prev_u0", "i4"),            # the build's own hint (no node attribute): 1 = prev_u0 is there
    ("prev_u0", "f8", 3),             # ... the previous solve's first control block before the low-pass (py:366-367)
])

#: Optimizer.srv response + solver diagnostics -> `neo_mpc_command` (48 bytes)
_, COMMAND_DTYPE = _record("neo_mpc_command", 48, "`neo_mpc_command` (include/neo_mpc.h): the response and diagnostics.", [
    ("vel", "f8", 3),               # response.output_vel.twist linear.x, linear.y, angular.z
    ("cost", "f8"),                 # objective value at the raw solver output (`x.fun`)
    ("status", "i4"),               # NEO_MPC_STATUS_* (0 converged -> `x.success`)
    ("iterations", "i4"),           # projected-gradient iterations (`x.nit`)
    ("evaluations", "i4"),          # objective evaluations per lane (`x.nfev` analogue)
    ("flags", "i4"),                # bit0 reset-on-new-goal taken, bit1 stopped by collision latch
])

NeoMpcBatch, _ = _record("neo_mpc_batch", 80, "`neo_mpc_batch` (include/neo_mpc.h).", [
    ("count", "size"), ("problems", "ptr"), ("states", "ptr"),
    ("warm_start", "ptr"), ("commands", "ptr"), ("solution", "ptr"),
    ("predicted_path", "ptr"), ("footprints", "ptr"),
    ("footprint_points", "u4"), ("reserved", "u4"), ("velocities", "ptr")])

NeoMpcLookaheadParams, _ = _record(
    "neo_mpc_lookahead_params", 32, "`neo_mpc_lookahead_params`: `<plugin>.lookahead_dist_*` (NeoMpcPlanner.cpp:311-322).", [
        ("lookahead_dist_min", "f8"), ("lookahead_dist_max", "f8"),
        ("lookahead_dist_close_to_goal", "f8"), ("max_transform_dist", "f8")])

#: `neo_mpc_carrot` (80 bytes): result of the plan pruning + look-ahead selection
#: (NeoMpcPlanner.cpp:83-104, 157-189, 221-232)
_, CARROT_DTYPE = _record("neo_mpc_carrot", 80, "`neo_mpc_carrot` (include/neo_mpc.h): one robot's carrot.", [
    ("xy", "f8", 2), ("q", "f8", 4), ("lookahead_dist", "f8"),
    ("begin", "u4"), ("end", "u4"), ("closer_to_goal", "i4"), ("slow_down", "i4"),
    ("status", "i4"), ("reserved", "i4"),
])

NeoMpcPlanBatch, _ = _record("neo_mpc_plan_batch", 64, "`neo_mpc_plan_batch` (include/neo_mpc.h).", [
    ("count", "size"), ("plan_poses", "ptr"), ("plan_offsets", "ptr"),
    ("robot_poses", "ptr"), ("footprint_costs", "ptr"), ("slow_down", "ptr"),
    ("carrots", "ptr"), ("problems", "ptr")])

NeoMpcFootprintBatch, _ = _record(
    "neo_mpc_footprint_batch", 64,
    "`neo_mpc_footprint_batch` (include/neo_mpc.h): one footprint gate call (NeoMpcPlanner.cpp:218-219).", [
        ("count", "size"), ("footprint", "ptr"), ("footprint_points", "u4"),
        ("per_robot_footprints", "u4"), ("poses", "ptr"), ("map_indices", "ptr"),
        ("problems", "ptr"), ("footprint_costs", "ptr"), ("footprints_out", "ptr")])

NeoMpcPlanCheckBatch, _ = _record(
    "neo_mpc_plan_check_batch", 72,
    "`neo_mpc_plan_check_batch` (include/neo_mpc.h): the fleet's plans checked against the live world map (K15).", [
        ("count", "size"), ("plan_poses", "ptr"), ("plan_offsets", "ptr"),
        ("robot_poses", "ptr"), ("footprint", "ptr"), ("footprint_points", "u4"),
        ("max_cost", "u4"), ("unknown_blocks", "u4"), ("outside_value", "u4"),
        ("max_poses", "u4"), ("reserved", "u4"), ("results", "ptr")])

#: `neo_mpc_plan_check` (24 bytes), and as a NumPy dtype
NeoMpcPlanCheck, PLAN_CHECK_DTYPE = _record(
    "neo_mpc_plan_check", 24, "`neo_mpc_plan_check` (include/neo_mpc.h): one robot's result of the plan check.", [
        ("begin", "u4"), ("end", "u4"), ("first_blocked", "u4"), ("status", "i4"),
        ("value", "u4"), ("reserved", "u4")])

NeoMpcReplanBatch, _ = _record(
    "neo_mpc_replan_batch", 80,
    "`neo_mpc_replan_batch` (include/neo_mpc.h): detours for the fleet's blocked plans, searched on the live world map (K16).", [
        ("count", "size"), ("starts", "ptr"), ("goals", "ptr"), ("checks", "ptr"),
        ("window", "u4"), ("max_cost", "u4"), ("unknown_cost", "u4"), ("neutral_cost", "u4"),
        ("max_path_cells", "u4"), ("reserved", "u4"), ("path_cells", "ptr"), ("path_poses", "ptr"), ("results", "ptr")])

#: `neo_mpc_replan` (24 bytes), and as a NumPy dtype
NeoMpcReplan, REPLAN_DTYPE = _record(
    "neo_mpc_replan", 24, "`neo_mpc_replan` (include/neo_mpc.h): one robot's result of the grid planner.", [
        ("status", "i4"), ("length", "u4"), ("cost", "u4"), ("window_x0", "i4"), ("window_y0", "i4"), ("reserved", "u4")])

NeoMpcWindowBatch, _ = _record(
    "neo_mpc_window_batch", 56,
    "`neo_mpc_window_batch` (include/neo_mpc.h): one roll of a fleet's costmap windows over the world map.", [
        ("count", "size"), ("size_x", "u4"), ("size_y", "u4"), ("resolution", "f8"),
        ("poses", "ptr"), ("problems", "ptr"), ("origins", "ptr"),
        ("outside_value", "u4"), ("reserved", "u4")])

NeoMpcStampBatch, _ = _record(
    "neo_mpc_stamp_batch", 80,
    "`neo_mpc_stamp_batch` (include/neo_mpc.h): the fleet's robots stamped into each other's windows.", [
        ("count", "size"), ("polygons", "ptr"), ("footprint", "ptr"),
        ("footprint_points", "u4"), ("per_robot_footprints", "u4"), ("poses", "ptr"),
        ("problems", "ptr"), ("inscribed_radius", "f8"), ("inflation_radius", "f8"),
        ("cost_scaling_factor", "f8"), ("reserved", "u8")])

#: `neo_mpc_scan_batch` (104 bytes), and as a NumPy dtype (the pointers as addresses)
NeoMpcScanBatch, SCAN_BATCH_DTYPE = _record(
    "neo_mpc_scan_batch", 104,
    "`neo_mpc_scan_batch` (include/neo_mpc.h): one update of the windows' obstacle layers from sensor points.", [
        ("count", "size"), ("points", "ptr"), ("point_counts", "ptr"),
        ("sensor_origins", "ptr"), ("max_points", "u4"), ("flags", "u4"),
        ("obstacle_max_range", "f8"), ("obstacle_min_range", "f8"),
        ("raytrace_max_range", "f8"), ("raytrace_min_range", "f8"),
        ("inscribed_radius", "f8"), ("inflation_radius", "f8"), ("cost_scaling_factor", "f8"),
        ("unknown_value", "u4"), ("reserved", "u4")])

#: `neo_mpc_scanner` (64 bytes), and as a NumPy dtype
NeoMpcScanner, SCANNER_DTYPE = _record(
    "neo_mpc_scanner", 64,
    "`neo_mpc_scanner` (include/neo_mpc.h): one scanner of a robot -- its mount and its LaserScan geometry.", [
        ("mount_x", "f8"), ("mount_y", "f8"), ("mount_yaw", "f8"),
        ("angle_min", "f8"), ("angle_increment", "f8"),
        ("range_min", "f8"), ("range_max", "f8"),
        ("flags", "u4"), ("reserved", "u4")])

#: `neo_mpc_laser_batch` (128 bytes), and as a NumPy dtype (the pointers as addresses)
NeoMpcLaserBatch, LASER_BATCH_DTYPE = _record(
    "neo_mpc_laser_batch", 128, """`neo_mpc_laser_batch` (include/neo_mpc.h): LaserScan ranges of every scanner of every robot,
    projected and -- for the update -- put into the windows' obstacle layers.""", [
        ("count", "size"), ("ranges", "ptr"), ("poses", "ptr"), ("scanners", "ptr"),
        ("sources", "u4"), ("beams", "u4"), ("points_out", "ptr"), ("origins_out", "ptr"),
        ("scan_flags", "u4"), ("unknown_value", "u4"),
        ("obstacle_max_range", "f8"), ("obstacle_min_range", "f8"),
        ("raytrace_max_range", "f8"), ("raytrace_min_range", "f8"),
        ("inscribed_radius", "f8"), ("inflation_radius", "f8"), ("cost_scaling_factor", "f8"),
        ("reserved", "u8")])

#: `neo_mpc_fleet_clear` (64 bytes), and as a NumPy dtype (the pointers as addresses)
NeoMpcFleetClear, FLEET_CLEAR_DTYPE = _record(
    "neo_mpc_fleet_clear", 64,
    "`neo_mpc_fleet_clear` (include/neo_mpc.h): the robots' outlines set free in the fleet's shared obstacle layer.", [
        ("count", "size"), ("polygons", "ptr"), ("footprint", "ptr"),
        ("footprint_points", "u4"), ("per_robot_footprints", "u4"), ("poses", "ptr"),
        ("problems", "ptr"), ("padding", "f8"), ("reserved", "u8")])

STATUS_CONVERGED = 0
STATUS_MAX_ITER = 1

FLAG_RESET = 1
FLAG_STOPPED = 2
FLAG_SKIPPED = 4
FLAG_WALL_IN_REACH = 8   # a lethal cell within the robot's reach tile (AUTO at control_steps 3: solved by the stage-wise direction)

ABI_VERSION = 2          # NEO_MPC_ABI_VERSION of include/neo_mpc.h
COMPAT_ODOM_YAW_GOAL_W = 1
COMPAT_REFERENCE_START = 2

MAX_INFLATION_CELLS = 64
MAX_SCAN_POINTS = 8192
SCAN_CLEAR = 1           # NEO_MPC_SCAN_CLEAR: raytrace the layer free from the sensor origin to every point
SCAN_MARK = 2            # NEO_MPC_SCAN_MARK: mark the points' cells lethal in the layer
MAX_SCAN_SOURCES = 4
MAX_DENOISE_GROUP = 16   # NEO_MPC_MAX_DENOISE_GROUP
NO_AGE = 0xFFFFFFFF       # NEO_MPC_NO_AGE
LASER_INF_IS_VALID = 1   # NEO_MPC_LASER_INF_IS_VALID: a range of +inf is a beam that met nothing, at range_max - 1e-4


def new_states(count, control_steps, waiting_time=3.0):
    """Fresh node state for `count` instances (py:115-152) and their warm starts (py:136)."""
    st = np.zeros(count, dtype=STATE_DTYPE)
    st["waiting_time"] = waiting_time
    warm = np.zeros((count, 3 * control_steps), dtype=np.float64)
    return st, warm


def scanner_array(scanners):
    """One scanner or a sequence of them -> a NumPy array of SCANNER_DTYPE.  A scanner is a mapping with the record's field
    names (flags and reserved default to 0), a NeoMpcScanner, or an element of such an array already."""
    if isinstance(scanners, np.ndarray) and scanners.dtype == SCANNER_DTYPE:
        return np.ascontiguousarray(scanners).reshape(-1)
    if isinstance(scanners, (dict, NeoMpcScanner)):
        scanners = [scanners]
    out = np.zeros(len(scanners), dtype=SCANNER_DTYPE)
    for k, sc in enumerate(scanners):
        for name in SCANNER_DTYPE.names:
            if isinstance(sc, dict):
                if name in sc:
                    out[k][name] = sc[name]
                else:
                    assert name in ("flags", "reserved"), "scanner %d lacks %s" % (k, name)
            else:
                out[k][name] = getattr(sc, name) if hasattr(sc, name) else sc[name]
    return out


def params_struct(params=None, **over):
    """dict of ROS parameter names (+ solver options) -> NeoMpcParams.  Missing names take
    the reference node's declared defaults (py:49-75)."""
    d = dict(
        acc_x_limit=0.5, acc_y_limit=0.5, acc_theta_limit=0.5,
        min_vel_x=-0.5, min_vel_y=-0.5, min_vel_trans=0.5, min_vel_theta=-0.5,
        max_vel_x=0.5, max_vel_y=0.5, max_vel_trans=0.5, max_vel_theta=0.5,
        w_trans=0.5, w_orient=0.5, w_control=0.5, w_terminal=0.5, w_costmap=0.5,
        w_footprint=2000.0, waiting_time=3.0, low_pass_gain=0.5, opt_tolerance=1e-5,
        prediction_horizon=0.5, control_steps=3,
        max_iterations=100, lbfgs_memory=4, compat_flags=COMPAT_ODOM_YAW_GOAL_W,
        step_tolerance=0.0, cost_tolerance=0.0, kink_radius=0.0, stall_step=0.0, method=0, reserved_i=0,
        window_tolerance=0.0)
    if params:
        d.update(params)
    d.update(over)
    s = NeoMpcParams()
    for name, ctype in NeoMpcParams._fields_:
        if name == "reserved":
            continue
        setattr(s, name, int(d[name]) if ctype is _C.c_int32 else float(d[name]))
    return s


def batch_struct(problems, states, warm, commands, solution=None, predicted_path=None,
                 footprints=None, ptr=lambda a: a.ctypes.data):
    """Build a NeoMpcBatch over arrays (NumPy by default; `ptr` extracts the address)."""
    b = NeoMpcBatch()
    b.count = int(problems.shape[0])
    b.problems = ptr(problems)
    b.states = ptr(states)
    b.warm_start = ptr(warm)
    b.commands = ptr(commands)
    b.solution = ptr(solution) if solution is not None else None
    b.predicted_path = ptr(predicted_path) if predicted_path is not None else None
    if footprints is not None:
        b.footprints = ptr(footprints)
        b.footprint_points = int(footprints.shape[1])
    else:
        b.footprints = None
        b.footprint_points = 0
    return b
