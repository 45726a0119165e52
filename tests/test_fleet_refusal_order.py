"""The order and the texts of the refusals of the fleet-layer entry points (K6, K8, K10, K11, K12).

The refusal tests next to each feature set one field wrong at a time and look at the return code.  Here every record has TWO
things wrong, and the call must report the one the C-ABI looks at first: the return code, and a fragment of
`neo_mpc_last_error()` that only that refusal's text holds.  The tables below list each check function's refusals in the
order they come in; `adjacent()` pairs every refusal with the one behind it.  Every call here is refused before it reaches the
device, so the device variants are handed the same host arrays (never read) and a null stream.  The value checks are the host
variants' alone and are never sent to a device variant."""
import ctypes as C

import numpy as np
import pytest

from neo_mpc_planner2_amd import abi, synthetic

INVALID, NO_COSTMAP, UNSUPPORTED = -1, -4, -5
ROBOTS, WINDOW, MAX_POINTS, BEAMS, RES = 3, 24, 64, 21, 0.1
NAN = float("nan")

# the smallest fleet the refusal tests of K8 to K12 use: a 40 x 40 world at 10 cm, 3 robots with 24 x 24 windows, 64 points a
# robot, one scanner of 21 beams, a 4-point rectangle
WORLD = np.zeros((40, 40), dtype=np.uint8)
POOL = np.zeros((ROBOTS, WINDOW, WINDOW), dtype=np.uint8)
SENSORS = np.array([[1.0, 1.0], [2.0, 1.5], [1.5, 2.5]])
ORIGINS = SENSORS - WINDOW * RES / 2
BEARINGS = np.linspace(0.0, 6.0, MAX_POINTS)
POINTS = SENSORS[:, None, :] + 0.8 * np.stack([np.cos(BEARINGS), np.sin(BEARINGS)], 1)[None]
COUNTS = np.full(ROBOTS, MAX_POINTS, dtype=np.uint32)
POSES = np.concatenate([SENSORS, np.zeros((ROBOTS, 1))], 1)
RECT = np.asarray(synthetic.RECT_FOOTPRINT, dtype=np.float64)
POLYGONS = np.ascontiguousarray(SENSORS[:, None, :] + RECT[None])
RANGES = np.full((ROBOTS, 1, BEAMS), 1.0, dtype=np.float32)
SCANNER = dict(mount_x=0.1, mount_y=0.0, mount_yaw=0.0, angle_min=-1.0, angle_increment=0.1, range_min=0.05, range_max=5.0)
POINTS_OUT = np.zeros((ROBOTS, 1, BEAMS, 2))
ORIGINS_OUT = np.zeros((ROBOTS, 1, 2))
COSTS_OUT = np.zeros(ROBOTS)
SETTINGS = dict(obstacle_max_range=2.5, obstacle_min_range=0.0, raytrace_max_range=3.0, raytrace_min_range=0.0,
                inscribed_radius=0.1, inflation_radius=0.25, cost_scaling_factor=3.0)   # R = 3 cells


def spoilt(a, index, value):
    b = np.array(a, copy=True)
    b[index] = value
    return b


BAD_COUNTS_1, BAD_COUNTS_2 = spoilt(COUNTS, 1, MAX_POINTS + 1), spoilt(COUNTS, 2, MAX_POINTS + 1)
BAD_SENSORS_1 = spoilt(SENSORS, (1, 0), np.inf)
BAD_POSES_0, BAD_POSES_1 = spoilt(POSES, (0, 2), NAN), spoilt(POSES, (1, 1), np.inf)
BAD_POLYGONS = spoilt(POLYGONS, (1, 2, 0), NAN)
BAD_RECT = spoilt(RECT, (3, 1), NAN)

# ------------------------------------------------------------------------------------------ the refusals, in their order
# (what to set wrong, the return code, a fragment of that refusal's text alone [, where it applies])
NULL_HANDLE = (dict(_handle=None), INVALID, "null argument")
RANGES_AND_RADII = [
    (dict(obstacle_max_range=-1.0), INVALID, "range -1 must be finite"),
    (dict(obstacle_min_range=-2.0), INVALID, "range -2 must be finite"),
    (dict(raytrace_max_range=-3.0), INVALID, "range -3 must be finite"),
    (dict(raytrace_min_range=-4.0), INVALID, "range -4 must be finite"),
    (dict(cost_scaling_factor=-1.0), INVALID, "cost_scaling_factor -1 must be finite"),
]
RADII = RANGES_AND_RADII[-1]
REACH = (dict(inflation_radius=6.6), UNSUPPORTED, "is more than 64 cells")          # 66 cells at 10 cm
# check_pool_batch: the handle's states exclude one another, so each is paired with the refusal in front and the reach behind
NO_POOL_MAP = (dict(), NO_COSTMAP, "the handle holds no costmap")
SINGLE_MAP = (dict(), UNSUPPORTED, "single costmap, not a pool")
POOL_COUNT = (dict(count=ROBOTS - 1), INVALID, "2 robots for a pool of 3 windows")
# check_world_scan
NO_WORLD_MAP = (dict(), NO_COSTMAP, "neo_mpc_set_world_map has not been called")
WORLD_COUNT = (dict(count=65536), INVALID, "65536 robots: at most")

SCAN_RECORD = [
    NULL_HANDLE,
    (dict(reserved=1), INVALID, "neo_mpc_scan_batch.reserved must be zero"),
    (dict(flags=4), INVALID, "unknown flags 0x4"),
    (dict(unknown_value=1), INVALID, "unknown_value 1 is neither 0 nor 255"),
    (dict(max_points=8193), INVALID, "max_points 8193: at most"),
    (dict(points=None), INVALID, "points and sensor_origins must not be null"),
] + RANGES_AND_RADII

LASER_RECORD = [
    NULL_HANDLE,
    (dict(reserved=1), INVALID, "neo_mpc_laser_batch.reserved must be zero"),
    (dict(sources=0), INVALID, "sources 0 outside"),
    (dict(beams=0), INVALID, "beams 0: at least 1"),
    (dict(scanners=None), INVALID, "scanners must not be null"),
    (dict(ranges=None), INVALID, "ranges and poses must not be null"),
    (dict(origins_out=None), INVALID, "points_out and origins_out must not be null", "project"),
    (dict(points_out=POINTS_OUT.ctypes.data + 8), INVALID, "points_out is not 16-byte aligned", "device"),
    (dict(scan_flags=0), INVALID, "scan_flags 0x0: NEO_MPC_SCAN_CLEAR", "update"),
    (dict(unknown_value=7), INVALID, "unknown_value 7 is neither 0 nor 255", "update"),
    (dict(scanner=dict(reserved=1)), INVALID, "neo_mpc_scanner.reserved of scanner 0"),
    (dict(scanner=dict(flags=2)), INVALID, "unknown flags 0x2 of scanner 0"),
    (dict(scanner=dict(mount_yaw=NAN)), INVALID, "of scanner 0 is not finite"),
    (dict(scanner=dict(range_min=-1.0)), INVALID, "scanner 0: range_min -1"),
] + [r + ("update",) for r in RANGES_AND_RADII]

CLEAR_RECORD = [
    (dict(reserved=1), INVALID, "neo_mpc_fleet_clear.reserved must be zero"),
    (dict(footprint_points=2), INVALID, "footprint_points 2 outside"),
    (dict(per_robot_footprints=2), INVALID, "per_robot_footprints must be 0 or 1"),
    (dict(padding=-1.0), INVALID, "padding -1 must be finite"),
    (dict(count=ROBOTS - 1), INVALID, "2 outlines for 3 robots"),
    (dict(polygons=None), INVALID, "neither polygons nor a footprint"),
]

STAMP_RECORD = [
    NULL_HANDLE,
    (dict(reserved=1), INVALID, "neo_mpc_stamp_batch.reserved must be zero"),
    (dict(footprint_points=17), INVALID, "footprint_points 17 outside"),
    (dict(per_robot_footprints=2), INVALID, "per_robot_footprints must be 0 or 1"),
    (dict(inscribed_radius=-0.5), INVALID, "inscribed_radius -0.5"),
    (dict(polygons=None), INVALID, "neither polygons nor a footprint"),
]

GATE_RECORD = [     # (behind NULL_HANDLE and "neo_mpc_set_costmap has not been called", which test_footprint_batch pairs by hand)
    (dict(footprint_points=2), INVALID, "footprint_points 2 outside"),
    (dict(per_robot_footprints=2), INVALID, "per_robot_footprints must be 0 or 1"),
    (dict(count=1 << 31), INVALID, "count too large"),
    (dict(footprint_costs=None), INVALID, "footprint/footprint_costs must not be null"),
    (dict(poses=None), INVALID, "poses and problems are both null"),
]


def merged(a, b):
    out = dict(a)
    for k, v in b.items():
        out[k] = dict(out[k], **v) if isinstance(v, dict) and k in out else v
    return out


def adjacent(order, *tags):
    """Every refusal of `order` that applies under `tags`, set wrong together with the one behind it -> (overrides, code,
    fragment) of the one in front."""
    rows = [r for r in order if len(r) == 3 or r[3] in tags]
    return [(merged(front[0], behind[0]), front[1], front[2]) for front, behind in zip(rows, rows[1:])]


# ------------------------------------------------------------------------------------------ records and calls
def record(cls, base, over, keep):
    r = cls()
    for k, v in merged(base, over).items():
        if k == "scanner":
            sc = abi.scanner_array(dict(SCANNER, **v))
            keep.append(sc)
            r.scanners = sc.ctypes.data
        elif k != "_handle":
            setattr(r, k, v.ctypes.data if isinstance(v, np.ndarray) else v)
    return r


def scan_base():
    return dict(SETTINGS, count=ROBOTS, points=POINTS, point_counts=COUNTS, sensor_origins=SENSORS, max_points=MAX_POINTS,
                flags=3, unknown_value=255)


def laser_base(update):
    base = dict(count=ROBOTS, ranges=RANGES, poses=POSES, scanner={}, sources=1, beams=BEAMS)
    if not update:
        return dict(base, points_out=POINTS_OUT, origins_out=ORIGINS_OUT)
    return dict(base, scan_flags=3, unknown_value=255, **SETTINGS)


def clear_base():
    return dict(count=ROBOTS, polygons=POLYGONS, footprint_points=4, padding=0.1)


STAMP_BASE = dict(count=ROBOTS, polygons=POLYGONS, footprint_points=4, inscribed_radius=0.1, inflation_radius=0.25,
                  cost_scaling_factor=3.0)
GATE_BASE = dict(count=ROBOTS, footprint=RECT, footprint_points=4, poses=POSES, footprint_costs=COSTS_OUT)


class Calls:
    """The entry points of one handle, by record: call(name, device, overrides[, clear overrides]) -> (code, text)."""

    def __init__(self, solver):
        self.lib, self.h = solver._lib, solver._handle

    def __call__(self, name, device, over, clear=None):
        cls, base = {"update_scan_layer": (abi.NeoMpcScanBatch, scan_base()),
                     "update_world_scan_layer": (abi.NeoMpcScanBatch, scan_base()),
                     "project_laser": (abi.NeoMpcLaserBatch, laser_base(False)),
                     "update_scan_layer_from_ranges": (abi.NeoMpcLaserBatch, laser_base(True)),
                     "update_world_scan_layer_from_ranges": (abi.NeoMpcLaserBatch, laser_base(True)),
                     "stamp_fleet": (abi.NeoMpcStampBatch, STAMP_BASE), "footprint_gate": (abi.NeoMpcFootprintBatch, GATE_BASE)}[name]
        keep = []
        args = [self.h if "_handle" not in over else None, C.byref(record(cls, base, over, keep))]
        if "world" in name:
            args.append(C.byref(record(abi.NeoMpcFleetClear, clear_base(), clear, keep)) if clear is not None else None)
        if device:
            args.append(None)
        code = getattr(self.lib, "neo_mpc_" + name + ("_device" if device else ""))(*args)
        return code, (self.lib.neo_mpc_last_error() or b"").decode()

    def expect(self, name, device, over, code, fragment, clear=None):
        got = self(name, device, over, clear)
        assert got[0] == code and fragment in got[1], (name, "device" if device else "host", over, clear, got, (code, fragment))

    def both(self, name, rows, clear_rows=()):
        for device in (False, True):
            for over, code, fragment in rows:
                self.expect(name, device, over, code, fragment)
            for over, code, fragment in clear_rows:
                self.expect(name, device, {}, code, fragment, clear=over)


def solver():
    from neo_mpc_planner2_amd.solver import BatchSolver
    return BatchSolver({})


def pool_states(s, call, name, record_rows, tags=()):
    """check_pool_batch behind a record's own refusals: without a map, with a single one, with the pool."""
    call.both(name, adjacent([RADII, NO_POOL_MAP, REACH]))
    s.set_costmap(POOL[0], RES, 0.0, 0.0)
    call.both(name, adjacent([RADII, SINGLE_MAP, REACH]))
    s.set_costmap_pool(POOL, RES, ORIGINS)
    for device in (False, True):
        t = tags + (("device",) if device else ())
        for over, code, fragment in adjacent(record_rows + [POOL_COUNT, REACH], *t):
            call.expect(name, device, over, code, fragment)


# ------------------------------------------------------------------------------------------ the tests, one per record type
@pytest.mark.gpu
def test_scan_batch():
    with solver() as s:
        call = Calls(s)
        call.both("update_world_scan_layer", adjacent([RADII, NO_WORLD_MAP, REACH]))
        pool_states(s, call, "update_scan_layer", SCAN_RECORD)
        s.set_world_map(WORLD, RES, 0.0, 0.0)
        call.both("update_world_scan_layer", adjacent(SCAN_RECORD + [WORLD_COUNT, REACH]))
        # the host variants' value checks, robot by robot: the counts entry in front of the sensor origin
        for name in ("update_scan_layer", "update_world_scan_layer"):
            call.expect(name, False, dict(point_counts=BAD_COUNTS_2, sensor_origins=BAD_SENSORS_1), INVALID,
                        "the sensor origin of robot 1")
            call.expect(name, False, dict(point_counts=BAD_COUNTS_1, sensor_origins=BAD_SENSORS_1), INVALID, "point_counts[1] = 65")


@pytest.mark.gpu
def test_laser_batch():
    with solver() as s:
        call = Calls(s)
        for device in (False, True):
            t = ("device",) if device else ()
            for over, code, fragment in adjacent(LASER_RECORD, "project", *t):
                call.expect("project_laser", device, over, code, fragment)
            for over, code, fragment in adjacent([RADII, NO_WORLD_MAP, REACH]):
                call.expect("update_world_scan_layer_from_ranges", device, over, code, fragment)
        pool_states(s, call, "update_scan_layer_from_ranges", LASER_RECORD, ("update",))
        s.set_world_map(WORLD, RES, 0.0, 0.0)
        for device in (False, True):
            t = ("update", "device") if device else ("update",)
            for over, code, fragment in adjacent(LASER_RECORD + [WORLD_COUNT, REACH], *t):
                call.expect("update_world_scan_layer_from_ranges", device, over, code, fragment)


@pytest.mark.gpu
def test_fleet_clear():
    with solver() as s:
        call = Calls(s)
        s.set_world_map(WORLD, RES, 0.0, 0.0)
        for name in ("update_world_scan_layer", "update_world_scan_layer_from_ranges"):
            call.both(name, (), adjacent(CLEAR_RECORD))
            for device in (False, True):
                # across the records: the scan record's last refusal in front of the clear record's first, the clear record's in
                # front of "count == 0: nothing to do"
                call.expect(name, device, REACH[0], UNSUPPORTED, REACH[2], clear=dict(reserved=1))
                call.expect(name, device, dict(count=0), INVALID, "neo_mpc_fleet_clear.reserved", clear=dict(count=0, reserved=1))
                call.expect(name, device, dict(count=0), INVALID, "1 outlines for 0 robots", clear=dict(count=1, polygons=None))
        # the host variants' value checks: the observation's in front of the clear record's, a vertex in front of a pose
        footprint = dict(polygons=None, footprint=BAD_RECT, poses=BAD_POSES_1)
        call.expect("update_world_scan_layer", False, dict(sensor_origins=BAD_SENSORS_1), INVALID, "the sensor origin of robot 1",
                    clear=dict(polygons=BAD_POLYGONS))
        call.expect("update_world_scan_layer", False, dict(point_counts=BAD_COUNTS_2), INVALID, "point_counts[2] = 65",
                    clear=footprint)
        call.expect("update_world_scan_layer_from_ranges", False, dict(poses=BAD_POSES_0), INVALID, "the pose of robot 0",
                    clear=dict(polygons=BAD_POLYGONS))
        for name in ("update_world_scan_layer", "update_world_scan_layer_from_ranges"):
            call.expect(name, False, {}, INVALID, "vertex 3 of polygon 0", clear=footprint)


@pytest.mark.gpu
def test_stamp_batch():
    with solver() as s:
        call = Calls(s)
        pool_states(s, call, "stamp_fleet", STAMP_RECORD)
        # the host variant's value checks: a vertex in front of a pose
        call.expect("stamp_fleet", False, dict(polygons=None, footprint=BAD_RECT, poses=BAD_POSES_1), INVALID,
                    "vertex 3 of polygon 0")


@pytest.mark.gpu
def test_footprint_batch():
    with solver() as s:
        call = Calls(s)
        call.both("footprint_gate", [(dict(_handle=None, footprint_points=2), INVALID, "null argument"),
                                     (dict(footprint_points=2), NO_COSTMAP, "neo_mpc_set_costmap has not been called")])
        s.set_costmap(POOL[0], RES, 0.0, 0.0)
        call.both("footprint_gate", adjacent(GATE_RECORD))
        # the host variant's value checks: a vertex in front of a pose
        call.expect("footprint_gate", False, dict(footprint=BAD_RECT, poses=BAD_POSES_1), INVALID,
                    "footprint vertex 3 of polygon 0")
