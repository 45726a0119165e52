"""Binary layout shared by the Python host side and the C-ABI (`include/neo_mpc.h`).

The records mirror the fields of the reference's ``neo_srvs2/srv/Optimizer`` request
and response (call sites src/NeoMpcPlanner.cpp:240-252 and
neo_mpc_planner2/mpc_optimization_server.py:349-403) plus the per-node state the
reference keeps between calls (mpc_optimization_server.py:115-152).
All floating point fields are float64, like the ROS messages.
"""
import numpy as np

#: one Optimizer.srv request -> `neo_mpc_problem` (256 bytes)
PROBLEM_DTYPE = np.dtype([
    ("cur_xy", "<f8", (2,)),        # request.current_pose.pose.position.{x,y}   (costmap frame)
    ("cur_q", "<f8", (4,)),         # request.current_pose.pose.orientation x,y,z,w
    ("carrot_xy", "<f8", (2,)),     # request.carrot_pose.pose.position.{x,y}    (base frame)
    ("carrot_q", "<f8", (4,)),      # request.carrot_pose.pose.orientation x,y,z,w
    ("goal_xyz", "<f8", (3,)),      # request.goal_pose.position x,y,z           (plan frame)
    ("goal_q", "<f8", (4,)),        # request.goal_pose.orientation x,y,z,w
    ("cur_vel", "<f8", (3,)),       # request.current_vel linear.x, linear.y, angular.z
    ("control_interval", "<f8"),    # request.control_interval = 1/controller_frequency
    ("delta_t", "<f8"),             # wall-clock seconds since the previous call (py:369-371)
    ("footprint_cost", "<f8"),      # getFootprintCost(published footprint), normalised; used when
                                    # no polygon is supplied (py:262, 343)
    ("map_index", "<i4"),           # which costmap of a pool (BatchSolver.set_costmap_pool); else ignored
    ("switch_opt", "<i4"),          # request.switch_opt (cpp:245; stored py:354, never read)
    ("skip", "<i4"),                # 1: no request is made for this robot this tick (cpp:234-236); state untouched.  0: solve.
                                    # Anything else: host batches are refused, device batches solve the robot (include/neo_mpc.h)
    ("reserved_i", "<i4"),
    ("reserved", "<f8", (5,)),
], align=False)
assert PROBLEM_DTYPE.itemsize == 256

#: per-instance persistent node state -> `neo_mpc_state` (128 bytes); the warm start
#: (py:136 `initial_guess`) is a separate float64[3*control_steps] row per instance.
STATE_DTYPE = np.dtype([
    ("last_control", "<f8", (3,)),  # py:117
    ("old_goal", "<f8", (7,)),      # py:146 / py:402: goal position xyz + orientation xyzw
    ("waiting_time", "<f8"),        # py:103, 361, 378-382
    ("has_old_goal", "<i4"),        # 0 until the first call (py:146 PoseStamped != Pose)
    ("collision", "<i4"),           # py:148 latch
    ("collision_footprint", "<i4"), # py:149
    ("has_prev_u0", "<i4"),           # the build's own hint (no node attribute): 1 = prev_u0 is there
    ("prev_u0", "<f8", (3,)),         # ... the previous solve's first control block before the low-pass (py:366-367)
], align=False)
assert STATE_DTYPE.itemsize == 128

#: Optimizer.srv response + solver diagnostics -> `neo_mpc_command` (48 bytes)
COMMAND_DTYPE = np.dtype([
    ("vel", "<f8", (3,)),           # response.output_vel.twist linear.x, linear.y, angular.z
    ("cost", "<f8"),                # objective value at the raw solver output (`x.fun`)
    ("status", "<i4"),              # NEO_MPC_STATUS_* (0 converged -> `x.success`)
    ("iterations", "<i4"),          # projected-gradient iterations (`x.nit`)
    ("evaluations", "<i4"),         # objective evaluations per lane (`x.nfev` analogue)
    ("flags", "<i4"),               # bit0 reset-on-new-goal taken, bit1 stopped by collision latch
], align=False)
assert COMMAND_DTYPE.itemsize == 48

#: `neo_mpc_carrot` (80 bytes): result of the plan pruning + look-ahead selection
#: (NeoMpcPlanner.cpp:83-104, 157-189, 221-232)
CARROT_DTYPE = np.dtype([
    ("xy", "<f8", (2,)), ("q", "<f8", (4,)), ("lookahead_dist", "<f8"),
    ("begin", "<u4"), ("end", "<u4"), ("closer_to_goal", "<i4"), ("slow_down", "<i4"),
    ("status", "<i4"), ("reserved", "<i4"),
], align=False)
assert CARROT_DTYPE.itemsize == 80

STATUS_CONVERGED = 0
STATUS_MAX_ITER = 1

FLAG_RESET = 1
FLAG_STOPPED = 2
FLAG_SKIPPED = 4
FLAG_WALL_IN_REACH = 8   # a lethal cell within the robot's reach tile (AUTO at control_steps 3: solved by the stage-wise direction)

ABI_VERSION = 2          # NEO_MPC_ABI_VERSION of include/neo_mpc.h
COMPAT_ODOM_YAW_GOAL_W = 1
COMPAT_REFERENCE_START = 2


def new_states(count, control_steps, waiting_time=3.0):
    """Fresh node state for `count` instances (py:115-152) and their warm starts (py:136)."""
    st = np.zeros(count, dtype=STATE_DTYPE)
    st["waiting_time"] = waiting_time
    warm = np.zeros((count, 3 * control_steps), dtype=np.float64)
    return st, warm


# ---------------------------------------------------------------------- ctypes mirrors
import ctypes as _C  # noqa: E402


class NeoMpcParams(_C.Structure):
    """`neo_mpc_params` (include/neo_mpc.h): the reference node's ROS parameters, same
    names (mpc_optimization_server.py:49-75), then the build's solver options."""
    _fields_ = [(n, _C.c_double) for n in (
        "acc_x_limit", "acc_y_limit", "acc_theta_limit",
        "min_vel_x", "min_vel_y", "min_vel_trans", "min_vel_theta",
        "max_vel_x", "max_vel_y", "max_vel_trans", "max_vel_theta",
        "w_trans", "w_orient", "w_control", "w_terminal", "w_costmap", "w_footprint",
        "waiting_time", "low_pass_gain", "opt_tolerance", "prediction_horizon")] + [
        ("control_steps", _C.c_int32), ("max_iterations", _C.c_int32),
        ("lbfgs_memory", _C.c_int32), ("compat_flags", _C.c_int32),
        ("step_tolerance", _C.c_double), ("cost_tolerance", _C.c_double),
        ("kink_radius", _C.c_double), ("stall_step", _C.c_double),
        ("method", _C.c_int32), ("reserved_i", _C.c_int32),
        ("window_tolerance", _C.c_double)]


ROS_PARAM_NAMES = tuple(n for n, _ in NeoMpcParams._fields_[:22])
COMPAT_ODOM_YAW_GOAL_W = 1


class NeoMpcBatch(_C.Structure):
    """`neo_mpc_batch` (include/neo_mpc.h)."""
    _fields_ = [("count", _C.c_size_t), ("problems", _C.c_void_p), ("states", _C.c_void_p),
                ("warm_start", _C.c_void_p), ("commands", _C.c_void_p), ("solution", _C.c_void_p),
                ("predicted_path", _C.c_void_p), ("footprints", _C.c_void_p),
                ("footprint_points", _C.c_uint32), ("reserved", _C.c_uint32), ("velocities", _C.c_void_p)]


class NeoMpcLookaheadParams(_C.Structure):
    """`neo_mpc_lookahead_params`: `<plugin>.lookahead_dist_*` (NeoMpcPlanner.cpp:311-322)."""
    _fields_ = [("lookahead_dist_min", _C.c_double), ("lookahead_dist_max", _C.c_double),
                ("lookahead_dist_close_to_goal", _C.c_double), ("max_transform_dist", _C.c_double)]


class NeoMpcPlanBatch(_C.Structure):
    """`neo_mpc_plan_batch` (include/neo_mpc.h)."""
    _fields_ = [("count", _C.c_size_t), ("plan_poses", _C.c_void_p), ("plan_offsets", _C.c_void_p),
                ("robot_poses", _C.c_void_p), ("footprint_costs", _C.c_void_p), ("slow_down", _C.c_void_p),
                ("carrots", _C.c_void_p), ("problems", _C.c_void_p)]


class NeoMpcFootprintBatch(_C.Structure):
    """`neo_mpc_footprint_batch` (include/neo_mpc.h): one footprint gate call (NeoMpcPlanner.cpp:218-219)."""
    _fields_ = [("count", _C.c_size_t), ("footprint", _C.c_void_p), ("footprint_points", _C.c_uint32),
                ("per_robot_footprints", _C.c_uint32), ("poses", _C.c_void_p), ("map_indices", _C.c_void_p),
                ("problems", _C.c_void_p), ("footprint_costs", _C.c_void_p), ("footprints_out", _C.c_void_p)]


class NeoMpcPlanCheckBatch(_C.Structure):
    """`neo_mpc_plan_check_batch` (include/neo_mpc.h): the fleet's plans checked against the live world map (K15)."""
    _fields_ = [("count", _C.c_size_t), ("plan_poses", _C.c_void_p), ("plan_offsets", _C.c_void_p),
                ("robot_poses", _C.c_void_p), ("footprint", _C.c_void_p), ("footprint_points", _C.c_uint32),
                ("max_cost", _C.c_uint32), ("unknown_blocks", _C.c_uint32), ("outside_value", _C.c_uint32),
                ("max_poses", _C.c_uint32), ("reserved", _C.c_uint32), ("results", _C.c_void_p)]


class NeoMpcPlanCheck(_C.Structure):
    """`neo_mpc_plan_check` (include/neo_mpc.h): one robot's result of the plan check."""
    _fields_ = [("begin", _C.c_uint32), ("end", _C.c_uint32), ("first_blocked", _C.c_uint32), ("status", _C.c_int32),
                ("value", _C.c_uint32), ("reserved", _C.c_uint32)]


#: `neo_mpc_plan_check` (24 bytes) as a NumPy dtype
PLAN_CHECK_DTYPE = np.dtype([
    ("begin", "<u4"), ("end", "<u4"), ("first_blocked", "<u4"), ("status", "<i4"), ("value", "<u4"), ("reserved", "<u4"),
], align=False)
assert PLAN_CHECK_DTYPE.itemsize == 24 == _C.sizeof(NeoMpcPlanCheck) and _C.sizeof(NeoMpcPlanCheckBatch) == 72


class NeoMpcWindowBatch(_C.Structure):
    """`neo_mpc_window_batch` (include/neo_mpc.h): one roll of a fleet's costmap windows over the world map."""
    _fields_ = [("count", _C.c_size_t), ("size_x", _C.c_uint32), ("size_y", _C.c_uint32), ("resolution", _C.c_double),
                ("poses", _C.c_void_p), ("problems", _C.c_void_p), ("origins", _C.c_void_p),
                ("outside_value", _C.c_uint32), ("reserved", _C.c_uint32)]


class NeoMpcStampBatch(_C.Structure):
    """`neo_mpc_stamp_batch` (include/neo_mpc.h): the fleet's robots stamped into each other's windows."""
    _fields_ = [("count", _C.c_size_t), ("polygons", _C.c_void_p), ("footprint", _C.c_void_p),
                ("footprint_points", _C.c_uint32), ("per_robot_footprints", _C.c_uint32), ("poses", _C.c_void_p),
                ("problems", _C.c_void_p), ("inscribed_radius", _C.c_double), ("inflation_radius", _C.c_double),
                ("cost_scaling_factor", _C.c_double), ("reserved", _C.c_uint64)]


MAX_INFLATION_CELLS = 64


class NeoMpcScanBatch(_C.Structure):
    """`neo_mpc_scan_batch` (include/neo_mpc.h): one update of the windows' obstacle layers from sensor points."""
    _fields_ = [("count", _C.c_size_t), ("points", _C.c_void_p), ("point_counts", _C.c_void_p),
                ("sensor_origins", _C.c_void_p), ("max_points", _C.c_uint32), ("flags", _C.c_uint32),
                ("obstacle_max_range", _C.c_double), ("obstacle_min_range", _C.c_double),
                ("raytrace_max_range", _C.c_double), ("raytrace_min_range", _C.c_double),
                ("inscribed_radius", _C.c_double), ("inflation_radius", _C.c_double), ("cost_scaling_factor", _C.c_double),
                ("unknown_value", _C.c_uint32), ("reserved", _C.c_uint32)]


#: the same record as a NumPy dtype (104 bytes; the pointers as addresses)
SCAN_BATCH_DTYPE = np.dtype([
    ("count", "<u8"), ("points", "<u8"), ("point_counts", "<u8"), ("sensor_origins", "<u8"),
    ("max_points", "<u4"), ("flags", "<u4"),
    ("obstacle_max_range", "<f8"), ("obstacle_min_range", "<f8"),
    ("raytrace_max_range", "<f8"), ("raytrace_min_range", "<f8"),
    ("inscribed_radius", "<f8"), ("inflation_radius", "<f8"), ("cost_scaling_factor", "<f8"),
    ("unknown_value", "<u4"), ("reserved", "<u4"),
], align=False)
assert SCAN_BATCH_DTYPE.itemsize == 104 == _C.sizeof(NeoMpcScanBatch)

MAX_SCAN_POINTS = 8192
SCAN_CLEAR = 1           # NEO_MPC_SCAN_CLEAR: raytrace the layer free from the sensor origin to every point
SCAN_MARK = 2            # NEO_MPC_SCAN_MARK: mark the points' cells lethal in the layer


class NeoMpcScanner(_C.Structure):
    """`neo_mpc_scanner` (include/neo_mpc.h): one scanner of a robot -- its mount and its LaserScan geometry."""
    _fields_ = [("mount_x", _C.c_double), ("mount_y", _C.c_double), ("mount_yaw", _C.c_double),
                ("angle_min", _C.c_double), ("angle_increment", _C.c_double),
                ("range_min", _C.c_double), ("range_max", _C.c_double),
                ("flags", _C.c_uint32), ("reserved", _C.c_uint32)]


#: the same record as a NumPy dtype (64 bytes)
SCANNER_DTYPE = np.dtype([
    ("mount_x", "<f8"), ("mount_y", "<f8"), ("mount_yaw", "<f8"), ("angle_min", "<f8"), ("angle_increment", "<f8"),
    ("range_min", "<f8"), ("range_max", "<f8"), ("flags", "<u4"), ("reserved", "<u4"),
], align=False)
assert SCANNER_DTYPE.itemsize == 64 == _C.sizeof(NeoMpcScanner)


class NeoMpcLaserBatch(_C.Structure):
    """`neo_mpc_laser_batch` (include/neo_mpc.h): LaserScan ranges of every scanner of every robot, projected and -- for
    the update -- put into the windows' obstacle layers."""
    _fields_ = [("count", _C.c_size_t), ("ranges", _C.c_void_p), ("poses", _C.c_void_p), ("scanners", _C.c_void_p),
                ("sources", _C.c_uint32), ("beams", _C.c_uint32), ("points_out", _C.c_void_p), ("origins_out", _C.c_void_p),
                ("scan_flags", _C.c_uint32), ("unknown_value", _C.c_uint32),
                ("obstacle_max_range", _C.c_double), ("obstacle_min_range", _C.c_double),
                ("raytrace_max_range", _C.c_double), ("raytrace_min_range", _C.c_double),
                ("inscribed_radius", _C.c_double), ("inflation_radius", _C.c_double), ("cost_scaling_factor", _C.c_double),
                ("reserved", _C.c_uint64)]


#: the same record as a NumPy dtype (128 bytes; the pointers as addresses)
LASER_BATCH_DTYPE = np.dtype([
    ("count", "<u8"), ("ranges", "<u8"), ("poses", "<u8"), ("scanners", "<u8"), ("sources", "<u4"), ("beams", "<u4"),
    ("points_out", "<u8"), ("origins_out", "<u8"), ("scan_flags", "<u4"), ("unknown_value", "<u4"),
    ("obstacle_max_range", "<f8"), ("obstacle_min_range", "<f8"),
    ("raytrace_max_range", "<f8"), ("raytrace_min_range", "<f8"),
    ("inscribed_radius", "<f8"), ("inflation_radius", "<f8"), ("cost_scaling_factor", "<f8"), ("reserved", "<u8"),
], align=False)
assert LASER_BATCH_DTYPE.itemsize == 128 == _C.sizeof(NeoMpcLaserBatch)

MAX_SCAN_SOURCES = 4
MAX_DENOISE_GROUP = 16   # NEO_MPC_MAX_DENOISE_GROUP
NO_AGE = 0xFFFFFFFF       # NEO_MPC_NO_AGE
LASER_INF_IS_VALID = 1   # NEO_MPC_LASER_INF_IS_VALID: a range of +inf is a beam that met nothing, at range_max - 1e-4


class NeoMpcFleetClear(_C.Structure):
    """`neo_mpc_fleet_clear` (include/neo_mpc.h): the robots' outlines set free in the fleet's shared obstacle layer."""
    _fields_ = [("count", _C.c_size_t), ("polygons", _C.c_void_p), ("footprint", _C.c_void_p),
                ("footprint_points", _C.c_uint32), ("per_robot_footprints", _C.c_uint32), ("poses", _C.c_void_p),
                ("problems", _C.c_void_p), ("padding", _C.c_double), ("reserved", _C.c_uint64)]


#: the same record as a NumPy dtype (64 bytes; the pointers as addresses)
FLEET_CLEAR_DTYPE = np.dtype([
    ("count", "<u8"), ("polygons", "<u8"), ("footprint", "<u8"), ("footprint_points", "<u4"), ("per_robot_footprints", "<u4"),
    ("poses", "<u8"), ("problems", "<u8"), ("padding", "<f8"), ("reserved", "<u8"),
], align=False)
assert FLEET_CLEAR_DTYPE.itemsize == 64 == _C.sizeof(NeoMpcFleetClear)


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
