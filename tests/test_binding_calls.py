"""CPU net under the Python binding's marshalling (neo_mpc_planner2_amd/solver.py): a `BatchSolver` made with `object.__new__`
whose `_lib` is a recording stand-in.  With NumPy inputs of the smallest shapes that still tell the fields apart -- 2 robots,
3 footprint points, a 4 x 5 window, 2 sources x 3 beams, ragged plans of 0, 1 and 3 poses -- every public method with a host
variant is called once: which entry point it calls, every scalar field of the record it passes, each pointer field (the
address of the array that was passed where it needed no conversion, 0 where it was left unset) and what it returns; then the
refusals that are Python assertions.  No GPU and no kernel runs; the device variants are the GPU suite's."""
import ctypes as C

import numpy as np
import pytest

from neo_mpc_planner2_amd import abi
from neo_mpc_planner2_amd.solver import BatchSolver

HANDLE = 0xBEEF
WORLD = dict(size_x=7, size_y=6, resolution=0.25, origin_x=-1.0, origin_y=2.0)
TICKET = 5
KERNEL_INFO = (4096, 17, 1)
BY_REFERENCE = type(C.byref(C.c_int()))
SOME = object()          # a pointer field that is set, to an array the method made itself
F64, F32, I32, U32, U8 = np.float64, np.float32, np.int32, np.uint32, np.uint8


class Recorder:
    """Stands in for the loaded library: every neo_mpc_* attribute records (name, arguments) and returns 0.  An argument is
    kept as its value: an address for a void pointer (None: NULL), a copy of a record passed by reference, "out" for any other
    reference -- those of the size getters, the kernel info and the ticket are answered with the fixed values above."""

    def __init__(self):
        self.calls = []
        self.armed = 0       # the count neo_mpc_get_dispatch_order answers with

    def __getattr__(self, name):
        if not name.startswith("neo_mpc_"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append((name, [self.seen(a) for a in args]))
            outs = [a._obj for a in args if isinstance(a, BY_REFERENCE) and not isinstance(a._obj, C.Structure)]
            answer = {"neo_mpc_get_world_map": tuple(WORLD.values()), "neo_mpc_kernel_info": KERNEL_INFO,
                      "neo_mpc_solve_batch_begin": (TICKET,), "neo_mpc_get_dispatch_order": (self.armed,)}.get(name, ())
            if name == "neo_mpc_get_world_map":          # (asked for the size alone, for the whole geometry, or for the cells)
                answer = answer[:len(outs)]
            assert len(outs) == len(answer), (name, len(outs))
            for out, value in zip(outs, answer):
                out.value = value
            return 0
        return entry

    @staticmethod
    def seen(a):
        if isinstance(a, BY_REFERENCE):
            return type(a._obj).from_buffer_copy(bytes(a._obj)) if isinstance(a._obj, C.Structure) else "out"
        return a.value if isinstance(a, C._SimpleCData) else a

    def take(self):
        calls, self.calls = self.calls, []
        return calls


def stand_in(map_shape=None):
    s = object.__new__(BatchSolver)
    s._lib = Recorder()
    s._handle = C.c_void_p(HANDLE)
    s.params, s.control_steps, s.device = {}, 3, 0
    s._keep = s._last_call = s._world_device = None
    s._in_flight = {}
    s._map_shape = map_shape
    return s


def one_call(s, name):
    """The one call the method under test made: `name`, the handle first -> the other arguments."""
    calls = s._lib.take()
    assert [c[0] for c in calls] == [name], calls
    assert calls[0][1][0] == HANDLE
    return calls[0][1][1:]


def record_is(rec, kind, **want):
    """`rec` is a `kind` whose fields are `want` -- an address for a pointer, SOME for one that only has to be set -- and 0 or
    NULL everywhere else."""
    assert type(rec) is kind
    names = [n for n, _ in kind._fields_]
    assert set(want) <= set(names), set(want) - set(names)
    for n in names:
        got = getattr(rec, n) or 0
        if want.get(n, 0) is SOME:
            assert got != 0, n
        else:
            assert got == want.get(n, 0), (n, got)


def at(a):
    return a.ctypes.data


def requests(count=2):
    problems = np.zeros(count, dtype=abi.PROBLEM_DTYPE)
    states, warm = abi.new_states(count, 3)
    return problems, states, warm


RADII = dict(inscribed_radius=0.2, inflation_radius=0.6, cost_scaling_factor=3.0)
RANGES = dict(obstacle_max_range=2.25, obstacle_min_range=0.125, raytrace_max_range=3.5, raytrace_min_range=0.25)
FOOTPRINT = np.array([(0.3, 0.0), (-0.2, 0.2), (-0.2, -0.2)])                    # 3 points, shared
POSES = np.array([(0.5, 0.25, 0.1), (1.5, -0.75, -2.0)])                         # 2 robots
POLYGONS = np.arange(12, dtype=F64).reshape(2, 3, 2)
SCANNERS = [dict(mount_x=0.1, mount_y=0.0, mount_yaw=0.0, angle_min=-0.5, angle_increment=0.5, range_min=0.1, range_max=9.0),
            dict(mount_x=-0.1, mount_y=0.0, mount_yaw=3.0, angle_min=-0.25, angle_increment=0.25, range_min=0.2, range_max=8.0,
                 flags=abi.LASER_INF_IS_VALID)]
LASER_RANGES = np.arange(1, 13, dtype=F32).reshape(2, 2, 3)                      # 2 robots x 2 sources x 3 beams
PLAN_POSES = np.arange(12, dtype=F64).reshape(4, 3)
PLAN_OFFSETS = np.array([0, 0, 1, 4], dtype=U32)                                  # plans of 0, 1 and 3 poses
ROBOT_POSES = np.array([(0.0, 0.0, 0.0), (1.0, 0.0, 0.5), (2.0, 1.0, -0.5)])


# ------------------------------------------------------------------------------------------ configuration and maps
def test_lifecycle_and_configuration():
    s = stand_in()
    s.set_params(w_trans=0.4, max_iterations=7)
    ps, = one_call(s, "neo_mpc_set_params")
    assert type(ps) is abi.NeoMpcParams and ps.w_trans == 0.4 and ps.max_iterations == 7 and ps.control_steps == 3
    assert ps.w_footprint == 2000.0 and s.params == dict(w_trans=0.4, max_iterations=7)
    with pytest.raises(ValueError):
        s.set_params(control_steps=4)
    assert s._lib.take() == [] and s.params == dict(w_trans=0.4, max_iterations=7)
    for mode, value in BatchSolver.HOST_PATHS.items():
        s.set_host_path(mode)
        assert one_call(s, "neo_mpc_set_host_path") == [value]
    assert BatchSolver.HOST_PATHS == {"auto": 0, "staged": 1, "zerocopy": 2, "zerocopy_out": 3}
    assert s.kernel_info() == dict(lds_bytes=4096, reach_cells=17, tile_in_lds=True)
    assert one_call(s, "neo_mpc_kernel_info") == ["out", "out", "out"]
    assert s.balance_dispatch(None) is None
    assert one_call(s, "neo_mpc_balance_dispatch_device") == [None, 0, None]
    assert s.dispatch_order() is None                                        # disarmed: asked for the count alone
    assert one_call(s, "neo_mpc_get_dispatch_order") == [None, None, "out"]
    for s._lib.armed, sorted_count in ((2048, True), (1500, False), (5120, False)):
        order, load = s.dispatch_order()
        assert order.shape == (s._lib.armed,) and order.dtype == U32
        assert (load.shape == order.shape and load.dtype == F32) if sorted_count else load is None
        assert s._lib.take() == [("neo_mpc_get_dispatch_order", [HANDLE, None, None, "out"]),
                                 ("neo_mpc_get_dispatch_order", [HANDLE, at(order), at(load) if sorted_count else None, "out"])]
    s._last_call, s._keep, s._in_flight = "x", "y", {1: "z"}
    s.close()
    assert one_call(s, "neo_mpc_destroy") == [] and s._handle is None
    assert s._last_call is None and s._keep is None and s._in_flight == {}
    s.close()
    assert s._lib.take() == []


def test_costmap_setters():
    s = stand_in()
    cells = np.arange(20, dtype=U8).reshape(5, 4)
    assert s.set_costmap(cells, 0.05, -1.0, 2.0) is None
    assert one_call(s, "neo_mpc_set_costmap") == [at(cells), 4, 5, 0.05, -1.0, 2.0] and s._map_shape == (1, 5, 4)
    s.set_costmap(cells.astype(np.int64), 1, 2, 3)                           # converted, not refused
    args = one_call(s, "neo_mpc_set_costmap")
    assert args[0] not in (None, at(cells)) and args[1:] == [4, 5, 1.0, 2.0, 3.0] and all(type(a) is float for a in args[3:])
    pool, origins = np.zeros((2, 5, 4), dtype=U8), np.array([(0.0, 1.0), (2.0, 3.0)])
    assert s.set_costmap_pool(pool, 0.05, origins) is None
    assert one_call(s, "neo_mpc_set_costmap_pool") == [at(pool), 2, 4, 5, 0.05, at(origins)] and s._map_shape == (2, 5, 4)
    assert not hasattr(s, "_pool_origins")                                   # (only device origins are retained)
    with pytest.raises(AssertionError):
        s.set_costmap_pool(pool, 0.05, origins[:1])
    with pytest.raises(ValueError):
        s.set_costmap(pool, 0.05, 0.0, 0.0)                                  # three dimensions
    assert s._lib.take() == [] and s._map_shape == (2, 5, 4)


def test_world_map_and_inflation():
    s = stand_in()
    s._world_device = "stale"
    world = np.arange(42, dtype=U8).reshape(6, 7)
    assert s.set_world_map(world, 0.25, -1.0, 2.0) is None
    assert one_call(s, "neo_mpc_set_world_map") == [at(world), 7, 6, 0.25, -1.0, 2.0]
    assert s._world_device is None and s._map_shape is None
    assert s.inflate_world_map(0.2, 0.6, 3) is None
    assert one_call(s, "neo_mpc_inflate_world_map") == [0.2, 0.6, 3.0]
    cells, res, ox, oy = s.get_world_map()
    assert cells.shape == (6, 7) and cells.dtype == U8 and (res, ox, oy) == (0.25, -1.0, 2.0)
    assert s._lib.take() == [("neo_mpc_get_world_map", [HANDLE, None, "out", "out", "out", "out", "out"]),
                             ("neo_mpc_get_world_map", [HANDLE, at(cells), None, None, None, None, None])]


def test_roll_costmap_pool():
    s = stand_in()
    origins = np.array([(0.0, 1.0), (2.0, 3.0)])
    problems = requests()[0]
    assert s.roll_costmap_pool(4, 5, 0.05, origins, poses=POSES, problems=problems, outside_value=254) is None
    b, = one_call(s, "neo_mpc_roll_costmap_pool")
    record_is(b, abi.NeoMpcWindowBatch, count=2, size_x=4, size_y=5, resolution=0.05, poses=at(POSES), problems=at(problems),
              origins=at(origins), outside_value=254)
    assert s._map_shape == (2, 5, 4) and not hasattr(s, "_pool_origins")
    s.roll_costmap_pool(4, 5, 0.05, origins, poses=POSES.ravel().tolist())    # flat poses are taken three by three
    b, = one_call(s, "neo_mpc_roll_costmap_pool")
    record_is(b, abi.NeoMpcWindowBatch, count=2, size_x=4, size_y=5, resolution=0.05, poses=SOME, origins=at(origins),
              outside_value=255)
    s._map_shape = "kept"
    s.roll_costmap_pool(4, 5, 0.05, np.zeros((0, 2)))                          # no window: the shape on record stays
    b, = one_call(s, "neo_mpc_roll_costmap_pool")
    assert b.count == 0 and s._map_shape == "kept"
    for bad in (dict(origins=origins.astype(F32)), dict(origins=origins.T), dict(origins=np.zeros((2, 3))),
                dict(poses=POSES[:1]), dict(problems=problems[:1]),
                dict(problems=problems.view(U8).reshape(2, -1)), dict(problems=np.zeros(4, dtype=abi.PROBLEM_DTYPE)[::2])):
        with pytest.raises(AssertionError):
            s.roll_costmap_pool(4, 5, 0.05, **dict(dict(origins=origins), **bad))
    assert s._lib.take() == []


def test_pool_getters():
    s = stand_in()
    for getter in (s.get_costmap_pool, s.get_scan_layer):
        with pytest.raises(AssertionError):
            getter()
    s._map_shape = (3, 5, 4)
    for getter, name in ((s.get_costmap_pool, "neo_mpc_get_costmap_pool"), (s.get_scan_layer, "neo_mpc_get_scan_layer")):
        cells, origins = getter()
        assert cells.shape == (3, 5, 4) and cells.dtype == U8 and origins.shape == (3, 2) and origins.dtype == F64
        assert one_call(s, name) == [0, 3, at(cells), at(origins)]
        cells, origins = getter(first=1)
        assert cells.shape == (2, 5, 4) and one_call(s, name) == [1, 2, at(cells), at(origins)]
        cells, origins = getter(1, 1)
        assert cells.shape == (1, 5, 4) and origins.shape == (1, 2) and one_call(s, name) == [1, 1, at(cells), at(origins)]


# ------------------------------------------------------------------------------------------ the fleet's layers
def test_stamp_fleet():
    s = stand_in()
    problems = requests()[0]
    radii = dict(RADII, reserved=0)
    assert s.stamp_fleet(0.2, 0.6, 3.0, polygons=POLYGONS) is None
    b, = one_call(s, "neo_mpc_stamp_fleet")
    record_is(b, abi.NeoMpcStampBatch, count=2, polygons=at(POLYGONS), footprint_points=3, **radii)
    s.stamp_fleet(0.2, 0.6, 3.0, footprint=FOOTPRINT, poses=POSES)
    b, = one_call(s, "neo_mpc_stamp_fleet")
    record_is(b, abi.NeoMpcStampBatch, count=2, footprint=at(FOOTPRINT), footprint_points=3, poses=at(POSES), **radii)
    s.stamp_fleet(0.2, 0.6, 3.0, footprint=POLYGONS, problems=problems)       # (one base-frame outline per robot)
    b, = one_call(s, "neo_mpc_stamp_fleet")
    record_is(b, abi.NeoMpcStampBatch, count=2, footprint=at(POLYGONS), footprint_points=3, per_robot_footprints=1,
              problems=at(problems), **radii)
    s.stamp_fleet(0.2, 0.6, 3.0, footprint=FOOTPRINT.tolist(), poses=POSES.ravel().tolist())
    b, = one_call(s, "neo_mpc_stamp_fleet")
    record_is(b, abi.NeoMpcStampBatch, count=2, footprint=SOME, footprint_points=3, poses=SOME, **radii)
    s.stamp_fleet(0.2, 0.6, 3.0, footprint=FOOTPRINT)                          # nobody to stamp
    b, = one_call(s, "neo_mpc_stamp_fleet")
    record_is(b, abi.NeoMpcStampBatch, count=0, footprint=at(FOOTPRINT), footprint_points=3, **radii)
    for bad in (dict(), dict(polygons=POLYGONS[0]), dict(polygons=np.zeros((2, 3, 3))), dict(footprint=np.zeros((3, 3))),
                dict(footprint=POLYGONS[:1], poses=POSES),
                dict(footprint=FOOTPRINT, problems=problems.view(U8).reshape(2, -1)),
                dict(footprint=FOOTPRINT, problems=np.zeros(4, dtype=abi.PROBLEM_DTYPE)[::2])):
        with pytest.raises(AssertionError):
            s.stamp_fleet(0.2, 0.6, 3.0, **bad)
    assert s._lib.take() == []


def scan_fields(count, **more):
    return dict(dict(RADII, **RANGES), count=count, **more)


def test_update_scan_layer():
    s = stand_in()
    points, sensors, counts = np.arange(16, dtype=F64).reshape(2, 4, 2), POSES[:, :2].copy(), np.array([4, 1], dtype=U32)
    with pytest.raises(AssertionError):
        s.update_scan_layer(0.2, 0.6, 3.0)                                     # no costmap yet
    s._map_shape = (2, 5, 4)
    assert s.update_scan_layer(0.2, 0.6, 3.0, points, sensors, counts, unknown_value=3, **RANGES) is None
    b, = one_call(s, "neo_mpc_update_scan_layer")
    record_is(b, abi.NeoMpcScanBatch, **scan_fields(2, points=at(points), sensor_origins=at(sensors), point_counts=at(counts),
                                                    max_points=4, flags=3, unknown_value=3))
    s.update_scan_layer(0.2, 0.6, 3.0, points.tolist(), sensors, counts.astype(np.int64), flags=abi.SCAN_MARK, **RANGES)
    b, = one_call(s, "neo_mpc_update_scan_layer")
    record_is(b, abi.NeoMpcScanBatch, **scan_fields(2, points=SOME, sensor_origins=at(sensors), point_counts=SOME, max_points=4,
                                                    flags=2, unknown_value=255))
    s.update_scan_layer(0.2, 0.6, 3.0)                                         # no new observation; nav2's ranges
    b, = one_call(s, "neo_mpc_update_scan_layer")
    record_is(b, abi.NeoMpcScanBatch, count=2, unknown_value=255, obstacle_max_range=2.5, raytrace_max_range=3.0, **RADII)
    s.update_scan_layer(0.2, 0.6, 3.0, on_device=False)
    one_call(s, "neo_mpc_update_scan_layer")
    for bad in (dict(points=points[:1]), dict(points=points[0]), dict(points=np.zeros((2, 4, 3))),
                dict(sensor_origins=POSES), dict(point_counts=counts[:1]), dict(sensor_origins=None)):
        with pytest.raises(AssertionError):
            s.update_scan_layer(0.2, 0.6, 3.0, **dict(dict(points=points, sensor_origins=sensors, point_counts=counts), **bad))
    assert s.reset_scan_layer() is None and one_call(s, "neo_mpc_reset_scan_layer") == []
    assert s._lib.take() == []


def laser_fields(scan, **more):
    """What every laser record of LASER_RANGES, POSES and SCANNERS holds; `scan`: the update's fields as well."""
    update = dict(dict(RADII, **RANGES), scan_flags=3, unknown_value=255) if scan else {}
    return dict(dict(update, count=2, sources=2, beams=3, poses=at(POSES), ranges=at(LASER_RANGES), scanners=SOME), **more)


def test_laser_batches():
    s = stand_in()
    points, sensors = s.project_laser(LASER_RANGES, POSES, SCANNERS)
    assert points.shape == (2, 2, 3, 2) and sensors.shape == (2, 2, 2) and points.dtype == sensors.dtype == F64
    b, = one_call(s, "neo_mpc_project_laser")
    record_is(b, abi.NeoMpcLaserBatch, **laser_fields(False, points_out=at(points), origins_out=at(sensors)))
    table = abi.scanner_array(SCANNERS)
    got = np.frombuffer(C.string_at(b.scanners, 128), dtype=abi.SCANNER_DTYPE)      # (the scanner table is alive: `keep`)
    assert got.tobytes() == table.tobytes() and got["flags"].tolist() == [0, 1]
    mine = np.ones_like(points)
    got_points, got_sensors = s.project_laser(LASER_RANGES.tolist(), POSES, table, points_out=mine)
    assert got_points is mine and got_sensors.shape == (2, 2, 2)
    b, = one_call(s, "neo_mpc_project_laser")
    record_is(b, abi.NeoMpcLaserBatch, **laser_fields(False, ranges=SOME, points_out=at(mine), origins_out=at(got_sensors),
                                                      scanners=at(table)))
    assert s.update_scan_layer_from_ranges(0.2, 0.6, 3.0, LASER_RANGES, POSES, SCANNERS, **RANGES) is None
    b, = one_call(s, "neo_mpc_update_scan_layer_from_ranges")
    record_is(b, abi.NeoMpcLaserBatch, **laser_fields(True))                         # (nothing projected is handed back)
    s.update_scan_layer_from_ranges(0.2, 0.6, 3.0, LASER_RANGES, POSES, SCANNERS, flags=abi.SCAN_CLEAR, points_out=mine,
                                    origins_out=sensors, unknown_value=9, **RANGES)
    b, = one_call(s, "neo_mpc_update_scan_layer_from_ranges")
    record_is(b, abi.NeoMpcLaserBatch, **laser_fields(True, scan_flags=1, unknown_value=9, points_out=at(mine),
                                                      origins_out=at(sensors)))
    for bad in (dict(ranges=LASER_RANGES[0]), dict(ranges=LASER_RANGES[:, :1]), dict(poses=POSES[:1]), dict(poses=POSES[:, :2]),
                dict(points_out=mine.astype(F32)), dict(points_out=mine[:, :, :2]), dict(points_out=mine.tolist()),
                dict(origins_out=np.zeros((2, 2, 3)))):
        with pytest.raises(AssertionError):
            s.project_laser(**dict(dict(ranges=LASER_RANGES, poses=POSES, scanners=SCANNERS), **bad))
    assert s._lib.take() == []


def test_world_scan_layer_updates():
    s = stand_in()                                                                   # (not tied to a pool: no costmap needed)
    points, sensors = np.arange(24, dtype=F64).reshape(3, 4, 2), np.zeros((3, 2))
    clear = dict(padding=0.1, footprint=FOOTPRINT, poses=ROBOT_POSES)
    assert s.update_world_scan_layer(0.2, 0.6, 3.0, points, sensors, clear=clear, **RANGES) is None
    b, c = one_call(s, "neo_mpc_update_world_scan_layer")
    record_is(b, abi.NeoMpcScanBatch, **scan_fields(3, points=at(points), sensor_origins=at(sensors), max_points=4, flags=3,
                                                    unknown_value=255))
    record_is(c, abi.NeoMpcFleetClear, count=3, footprint=at(FOOTPRINT), footprint_points=3, poses=at(ROBOT_POSES), padding=0.1)
    s.update_world_scan_layer(0.2, 0.6, 3.0, clear=dict(polygons=POLYGONS), **RANGES)    # the count is the clear's
    b, c = one_call(s, "neo_mpc_update_world_scan_layer")
    record_is(b, abi.NeoMpcScanBatch, **scan_fields(2, unknown_value=255))
    record_is(c, abi.NeoMpcFleetClear, count=2, polygons=at(POLYGONS), footprint_points=3)
    s.update_world_scan_layer(0.2, 0.6, 3.0)
    b, c = one_call(s, "neo_mpc_update_world_scan_layer")
    assert b.count == 1 and c is None
    s.update_world_scan_layer(0.2, 0.6, 3.0, count=4)
    assert one_call(s, "neo_mpc_update_world_scan_layer")[0].count == 4
    for bad in (dict(points=points, sensor_origins=sensors, clear=dict(polygons=POLYGONS)),      # 3 robots, 2 outlines
                dict(clear=dict(polygons=POLYGONS, margin=0.1)), dict(clear=dict(padding=0.1, footprint=FOOTPRINT[:, :1],
                                                                                 poses=POSES))):
        with pytest.raises(AssertionError):
            s.update_world_scan_layer(0.2, 0.6, 3.0, **bad)
    problems = requests()[0]
    s.update_world_scan_layer_from_ranges(0.2, 0.6, 3.0, LASER_RANGES, POSES, SCANNERS, **RANGES,
                                          clear=dict(padding=0.25, footprint=POLYGONS, problems=problems))
    b, c = one_call(s, "neo_mpc_update_world_scan_layer_from_ranges")
    record_is(b, abi.NeoMpcLaserBatch, **laser_fields(True))
    record_is(c, abi.NeoMpcFleetClear, count=2, footprint=at(POLYGONS), footprint_points=3, per_robot_footprints=1,
              problems=at(problems), padding=0.25)
    s.update_world_scan_layer_from_ranges(0.2, 0.6, 3.0, LASER_RANGES, POSES, SCANNERS, flags=abi.SCAN_MARK, **RANGES)
    b, c = one_call(s, "neo_mpc_update_world_scan_layer_from_ranges")
    record_is(b, abi.NeoMpcLaserBatch, **laser_fields(True, scan_flags=2))
    assert c is None
    with pytest.raises(AssertionError):
        s.update_world_scan_layer_from_ranges(0.2, 0.6, 3.0, LASER_RANGES, POSES, SCANNERS, clear=dict(polygons=POLYGONS[:1]))
    assert s._lib.take() == []


def test_world_scan_layer_configuration_and_getters():
    s = stand_in()
    assert s.set_world_scan_denoise(3) is None and one_call(s, "neo_mpc_set_world_scan_denoise") == [3, 8]
    assert s.set_world_scan_denoise(2.0, connectivity=4) is None and one_call(s, "neo_mpc_set_world_scan_denoise") == [2, 4]
    assert s.set_world_scan_decay(5) is None and one_call(s, "neo_mpc_set_world_scan_decay") == [5]
    assert s.reset_world_scan_layer() is None and one_call(s, "neo_mpc_reset_world_scan_layer") == []
    size = ("neo_mpc_get_world_map", [HANDLE, None, "out", "out", None, None, None])
    layer, live = s.get_world_scan_layer()
    assert layer.shape == live.shape == (6, 7) and layer.dtype == live.dtype == U8 and layer is not live
    assert s._lib.take() == [("neo_mpc_get_world_scan_layer", [HANDLE, None, None]), size,
                             ("neo_mpc_get_world_scan_layer", [HANDLE, at(layer), at(live)])]
    cells = s.get_world_scan_denoised()
    assert cells.shape == (6, 7) and cells.dtype == U8
    assert s._lib.take() == [("neo_mpc_get_world_scan_denoised", [HANDLE, None]), size,
                             ("neo_mpc_get_world_scan_denoised", [HANDLE, at(cells)])]
    ages = s.get_world_scan_ages()
    assert ages.shape == (6, 7) and ages.dtype == U32
    assert s._lib.take() == [("neo_mpc_get_world_scan_ages", [HANDLE, None]), size,
                             ("neo_mpc_get_world_scan_ages", [HANDLE, at(ages)])]


# ------------------------------------------------------------------------------------------ the solver's own calls
def test_solve_marshals_a_batch_and_reuses_it():
    s = stand_in()
    problems, states, warm = requests()
    commands, solution = s.solve(problems, states, warm)
    assert commands.dtype == abi.COMMAND_DTYPE and commands.shape == (2,) and solution.shape == (2, 9) and solution.dtype == F64
    b, = one_call(s, "neo_mpc_solve_batch")
    plain = dict(count=2, problems=at(problems), states=at(states), warm_start=at(warm))
    record_is(b, abi.NeoMpcBatch, commands=at(commands), solution=at(solution), **plain)
    assert s._last_call is None and s._keep[0] is problems
    footprints = np.zeros((2, 3, 2))
    commands, solution, path = s.solve(problems, states, warm, want_path=True, footprints=footprints)
    assert path.shape == (2, 3, 3) and path.dtype == F64
    b, = one_call(s, "neo_mpc_solve_batch")
    record_is(b, abi.NeoMpcBatch, commands=at(commands), solution=at(solution), predicted_path=at(path), footprints=at(footprints),
              footprint_points=3, **plain)
    out = (np.zeros(2, dtype=abi.COMMAND_DTYPE), np.zeros((2, 9)))
    assert s.solve(problems, states, warm, out=out) is not None and s._last_call is not None
    first, = one_call(s, "neo_mpc_solve_batch")
    record_is(first, abi.NeoMpcBatch, commands=at(out[0]), solution=at(out[1]), **plain)
    marshalled = s._last_call
    assert s.solve(problems, states, warm, out=out) is out and s._last_call is marshalled     # the same arrays: reused
    again, = one_call(s, "neo_mpc_solve_batch")
    assert bytes(again) == bytes(first)
    other = warm.copy()
    s.solve(problems, states, other, out=out)                                                 # another array: marshalled anew
    b, = one_call(s, "neo_mpc_solve_batch")
    assert b.warm_start == at(other) and s._last_call is not marshalled
    for bad in (dict(states=states[:1]), dict(states=states.view(U8).reshape(2, -1)), dict(warm=warm.astype(F32)),
                dict(warm=np.zeros((2, 6))), dict(out=(out[0], np.zeros((2, 6)))), dict(out=(out[0][:1], out[1])),
                dict(footprints=np.zeros((1, 3, 2))), dict(footprints=np.zeros((2, 3, 3)))):
        with pytest.raises(AssertionError):
            s.solve(**dict(dict(problems=problems, states=states, warm=warm), **bad))
    assert s._lib.take() == []


def test_split_solve_postprocess_and_the_test_hooks():
    s = stand_in()
    problems, states, warm = requests()
    out = (np.zeros(2, dtype=abi.COMMAND_DTYPE), np.zeros((2, 9)))
    assert s.solve_begin(problems, states, warm, out) == TICKET
    b, ticket = one_call(s, "neo_mpc_solve_batch_begin")
    plain = dict(count=2, problems=at(problems), states=at(states), warm_start=at(warm))
    record_is(b, abi.NeoMpcBatch, commands=at(out[0]), solution=at(out[1]), **plain)
    assert ticket == "out" and list(s._in_flight) == [TICKET] and s._in_flight[TICKET][1:] == (problems, states, warm, out)
    assert s.solve_wait(TICKET) is out and one_call(s, "neo_mpc_solve_batch_wait") == [TICKET] and s._in_flight == {}
    with pytest.raises(AssertionError):
        s.solve_begin(problems.view(U8).reshape(2, -1), states, warm, out)
    solution, success = np.ones((2, 9)), np.array([1, 0], dtype=I32)
    commands = s.postprocess(problems, states, warm, solution, success=success)
    assert commands.dtype == abi.COMMAND_DTYPE and commands.shape == (2,)
    b, flags = one_call(s, "neo_mpc_postprocess_batch")
    record_is(b, abi.NeoMpcBatch, commands=at(commands), solution=at(solution), **plain)
    assert flags == at(success)
    commands, path = s.postprocess(problems, states, warm, solution, want_path=True)
    b, flags = one_call(s, "neo_mpc_postprocess_batch")
    record_is(b, abi.NeoMpcBatch, commands=at(commands), solution=at(solution), predicted_path=at(path), **plain)
    assert flags is None and path.shape == (2, 3, 3)
    u = np.ones((2, 9))
    f = s.objective(problems, u)
    assert f.shape == (2,) and one_call(s, "neo_mpc_objective_batch") == [at(problems), at(u), at(f), 2]
    g = s.gradient(problems, u)
    assert g.shape == (2, 9) and one_call(s, "neo_mpc_gradient_batch") == [at(problems), at(u), at(g), 2]
    d = s.direction(problems, u, 4)
    assert np.isnan(d).all() and d.shape == (2, 9)
    assert one_call(s, "neo_mpc_direction_batch") == [at(problems), at(u), at(d), 2, 4]


# ------------------------------------------------------------------------------------------ gate, carrots, plan check
def test_footprint_gate():
    s = stand_in()
    problems, indices = requests()[0], np.array([1, 0], dtype=I32)
    costs = s.footprint_gate(FOOTPRINT, poses=POSES)
    assert costs.shape == (2,) and costs.dtype == F64
    b, = one_call(s, "neo_mpc_footprint_gate")
    record_is(b, abi.NeoMpcFootprintBatch, count=2, footprint=at(FOOTPRINT), footprint_points=3, poses=at(POSES),
              footprint_costs=at(costs))
    costs, polygons = s.footprint_gate(POLYGONS, problems=problems, map_indices=indices, want_polygons=True)
    assert polygons.shape == (2, 3, 2) and polygons.dtype == F64
    b, = one_call(s, "neo_mpc_footprint_gate")
    record_is(b, abi.NeoMpcFootprintBatch, count=2, footprint=at(POLYGONS), footprint_points=3, per_robot_footprints=1,
              problems=at(problems), map_indices=at(indices), footprint_costs=at(costs), footprints_out=at(polygons))
    s.footprint_gate(FOOTPRINT.tolist(), poses=POSES.ravel(), problems=problems, map_indices=[1, 0])
    b, = one_call(s, "neo_mpc_footprint_gate")
    record_is(b, abi.NeoMpcFootprintBatch, count=2, footprint=SOME, footprint_points=3, poses=at(POSES), problems=at(problems),
              map_indices=SOME, footprint_costs=SOME)
    for bad in (dict(), dict(footprint=FOOTPRINT[0], poses=POSES), dict(footprint=np.zeros((3, 3)), poses=POSES),
                dict(footprint=POLYGONS[:1], poses=POSES), dict(poses=POSES, problems=problems[:1]),
                dict(problems=problems.view(U8).reshape(2, -1)), dict(poses=POSES, map_indices=indices[:1])):
        with pytest.raises(AssertionError):
            s.footprint_gate(**dict(dict(footprint=FOOTPRINT), **bad))
    assert s._lib.take() == []


def test_select_carrots():
    s = stand_in()
    slow_down, costs, problems = np.ones(3, dtype=I32), np.array([0.0, 254.0, 255.0]), requests(3)[0]
    carrots = s.select_carrots(PLAN_POSES, PLAN_OFFSETS, ROBOT_POSES, slow_down)
    assert carrots.dtype == abi.CARROT_DTYPE and carrots.shape == (3,)
    lp, b = one_call(s, "neo_mpc_select_carrots")
    record_is(lp, abi.NeoMpcLookaheadParams, lookahead_dist_min=0.5, lookahead_dist_max=0.5, lookahead_dist_close_to_goal=0.5,
              max_transform_dist=1e9)
    record_is(b, abi.NeoMpcPlanBatch, count=3, plan_poses=at(PLAN_POSES), plan_offsets=at(PLAN_OFFSETS),
              robot_poses=at(ROBOT_POSES), slow_down=at(slow_down), carrots=at(carrots))
    carrots = s.select_carrots(PLAN_POSES.ravel().tolist(), PLAN_OFFSETS.astype(np.int64), ROBOT_POSES, slow_down, costs, problems,
                               lookahead_dist_min=0.2, lookahead_dist_max=0.8, lookahead_dist_close_to_goal=0.3,
                               max_transform_dist=4.0)
    lp, b = one_call(s, "neo_mpc_select_carrots")
    record_is(lp, abi.NeoMpcLookaheadParams, lookahead_dist_min=0.2, lookahead_dist_max=0.8, lookahead_dist_close_to_goal=0.3,
              max_transform_dist=4.0)
    record_is(b, abi.NeoMpcPlanBatch, count=3, plan_poses=SOME, plan_offsets=SOME, robot_poses=at(ROBOT_POSES),
              footprint_costs=at(costs), slow_down=at(slow_down), carrots=at(carrots), problems=at(problems))
    for bad in (dict(plan_offsets=PLAN_OFFSETS[:3]), dict(slow_down=slow_down.astype(np.int64)), dict(slow_down=slow_down[:2]),
                dict(problems=problems.view(U8).reshape(3, -1))):
        with pytest.raises(AssertionError):
            s.select_carrots(**dict(dict(plan_poses=PLAN_POSES, plan_offsets=PLAN_OFFSETS, robot_poses=ROBOT_POSES,
                                         slow_down=slow_down), **bad))
    assert s._lib.take() == []


def test_check_plans():
    s = stand_in()
    results = s.check_plans(PLAN_POSES, PLAN_OFFSETS)
    assert results.dtype == abi.PLAN_CHECK_DTYPE and results.shape == (3,)
    b, = one_call(s, "neo_mpc_check_plans")
    record_is(b, abi.NeoMpcPlanCheckBatch, count=3, plan_poses=at(PLAN_POSES), plan_offsets=at(PLAN_OFFSETS), max_cost=253,
              outside_value=255, results=at(results))
    results = s.check_plans(PLAN_POSES.tolist(), PLAN_OFFSETS, robot_poses=ROBOT_POSES, footprint=FOOTPRINT, max_cost=100,
                            unknown_blocks=True, outside_value=0, max_poses=2)
    b, = one_call(s, "neo_mpc_check_plans")
    record_is(b, abi.NeoMpcPlanCheckBatch, count=3, plan_poses=SOME, plan_offsets=at(PLAN_OFFSETS), robot_poses=at(ROBOT_POSES),
              footprint=at(FOOTPRINT), footprint_points=3, max_cost=100, unknown_blocks=1, max_poses=2, results=at(results))
    for bad in (dict(robot_poses=POSES), dict(footprint=POLYGONS), dict(footprint=np.zeros((3, 3)))):
        with pytest.raises(AssertionError):
            s.check_plans(PLAN_POSES, PLAN_OFFSETS, **bad)
    assert s._lib.take() == []
