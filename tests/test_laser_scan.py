"""The scan step fed from LaserScan ranges (K11): the ranges of every scanner of every robot are projected into global-frame
points and sensor origins on the device, and the scan layer is updated from all scanners -- every clear, then every mark:
roll -> scan (points or ranges) -> stamp -> gate -> carrots -> solve.

laser_geometry and nav2 cannot be built here, so the contract is the text in include/neo_mpc.h (neo_mpc_laser_batch) and its
executable form the transcription in tests/laser_scan_reference.py.  The projection is float64 + - * with a cos / sin table
from the host's libm -- exact against the transcription -- and ONE device sincos of the robot's yaw, which is where the one
tolerance of this file comes from (test_projection_on_the_device).  Everything behind the projection is compared bit for
bit: the layer update is fed with the points the device produced."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from neo_mpc_planner2_amd import _lib, abi
from tests import laser_scan_reference as ref
from tests import scan_layer_reference as scan_ref
from tests.c_probe import check_entry_points, check_layout, probe_header
from tests.fleet_kit import F32, RECT, Side, capture_fleet, gpu, inflation_for, replay_against_direct, same, scanner, standing_fleet, window_state

ENTRY_POINTS = ("neo_mpc_laser_beam_table", "neo_mpc_project_laser", "neo_mpc_project_laser_device",
                "neo_mpc_update_scan_layer_from_ranges", "neo_mpc_update_scan_layer_from_ranges_device")


def f32(v):
    """A LaserScan field as the caller hands it over: float32 on the wire, widened."""
    return float(F32(v))


# ------------------------------------------------------------------------------------------ 1: the hand-worked projection
def test_projection_by_hand():
    """A scanner at (0.2, 0) turned by pi/2 on a robot at (1, 2, 0); beam i looks along pi/2 + (-pi/2 + i pi/2) = i pi/2 in
    the base frame: +x, +y, -x, -y, +x, +y, +x.  range_min 0.5, range_max 8."""
    below = float(np.nextafter(F32(0.5), F32(0.0)))
    ranges = [1.0, math.nan, math.inf, -math.inf, 0.5, 8.0, below]
    sc = scanner((0.2, 0.0, math.pi / 2), -math.pi / 2, math.pi / 2, 0.5, 8.0)
    # the valid set: 1.0 and range_min itself; range_max is not (r < range_max), nor anything that is not a number in range
    assert [ref.valid_range(sc, r) for r in ranges] == [1.0, None, None, None, 0.5, None, None]
    with_inf = dict(sc, flags=ref.INF_IS_VALID)
    assert [ref.valid_range(with_inf, r) for r in ranges] == [1.0, None, 8.0 - 1e-4, None, 0.5, None, None]
    # ... and a substitute below range_min is as invalid as any other range there
    assert ref.valid_range(scanner((0, 0, 0), 0, 0, 8.0, 8.0, ref.INF_IS_VALID), math.inf) is None
    for flags, third in ((0, None), (ref.INF_IS_VALID, (1.0 + 0.2 - 7.9999, 2.0))):
        points, origins, _ = ref.project([[ranges]], [(1.0, 2.0, 0.0)], [dict(sc, flags=flags)])
        assert np.abs(origins[0, 0] - (1.2, 2.0)).max() <= 1e-12
        want = [(2.2, 2.0), None, third, None, (1.7, 2.0), None, None]
        for i, w in enumerate(want):
            if w is None:
                assert np.isnan(points[0, 0, i]).all(), i
            else:
                assert np.abs(points[0, 0, i] - w).max() <= 1e-12, (i, points[0, 0, i])
    # a turned robot: at yaw pi/2 the base frame's +x is the world's +y
    points, origins, _ = ref.project([[[1.0]]], [(1.0, 2.0, math.pi / 2)], [sc])
    assert np.abs(points[0, 0, 0] - (1.0, 2.0 + 1.2)).max() <= 1e-12 and np.abs(origins[0, 0] - (1.0, 2.2)).max() <= 1e-12


# ------------------------------------------------------------------------------------------ 2: the beam table
FRONT = scanner((0.3, 0.1, 0.2), f32(-2.35619), f32(0.0157603), 0.05, 10.0, ref.INF_IS_VALID)
REAR = scanner((-0.3, -0.05, 3.0), f32(-1.5708), f32(0.0105), 0.05, 10.0)


@pytest.mark.parametrize("beams", (1, 300, 1081))
def test_beam_table_equals_the_transcription(beams):
    from neo_mpc_planner2_amd.solver import laser_beam_table
    for sc in (FRONT, REAR):
        got, want = laser_beam_table(sc, beams), np.array(ref.beam_table(sc, beams))
        assert got.shape == (beams, 2) and got.tobytes() == want.tobytes()
    lib = _lib.load()
    bad = abi.scanner_array(dict(FRONT, range_min=-0.1))
    table = np.zeros((beams, 2))
    assert lib.neo_mpc_laser_beam_table(C.cast(bad.ctypes.data, C.POINTER(abi.NeoMpcScanner)), beams, table.ctypes.data) == -1
    assert lib.neo_mpc_laser_beam_table(None, beams, table.ctypes.data) == -1 and not table.any()


# ------------------------------------------------------------------------------------------ 3: records and entry points
def test_laser_records_layout_and_entry_points(tmp_path):
    got = probe_header(tmp_path, ["neo_mpc_scanner", "neo_mpc_laser_batch"], ["MAX_SCAN_SOURCES", "LASER_INF_IS_VALID"], ENTRY_POINTS)
    check_layout(got, "neo_mpc_scanner", 64, struct=abi.NeoMpcScanner, dtype=abi.SCANNER_DTYPE)
    check_layout(got, "neo_mpc_laser_batch", 128, struct=abi.NeoMpcLaserBatch, dtype=abi.LASER_BATCH_DTYPE)
    assert got["MAX_SCAN_SOURCES"] == abi.MAX_SCAN_SOURCES == 4 and got["LASER_INF_IS_VALID"] == abi.LASER_INF_IS_VALID == 1
    assert len(ENTRY_POINTS) == 5
    check_entry_points(ENTRY_POINTS)


# ------------------------------------------------------------------------------------------ 4: clear before mark, two scanners
TWO_RES, TWO_SIZE = 1.0, 32
TWO_POSE = np.array([(16.5, 16.5, 0.0)])
TWO_A = scanner((0.0, 0.0, 0.0), 0.0, 0.0, 0.1, 30.0)          # one beam along +x from (16.5, 16.5), range 4: ends in (20, 16)
TWO_B = scanner((-4.0, 0.0, 0.0), 0.0, 0.0, 0.1, 30.0)         # ... from (12.5, 16.5), range 12: through (20, 16) into (24, 16)
TWO_RANGES = np.array([[[4.0], [12.0]]], dtype=F32)
TWO_KW = dict(obstacle_max_range=20.0, obstacle_min_range=0.0, raytrace_max_range=20.0, raytrace_min_range=0.0)
TWO_INFLATION = (0.0, 0.0, 1.0)                                 # R = 0: the layer's cells and nothing around them


def check_two_scanners(together, one_after_the_other):
    """Layers [32, 32] of the one window after one two-source update, and after two single-source updates, A then B."""
    row = together[16]
    assert row[20] == 254 and row[24] == 254                                 # both marks stand
    assert (row[21:24] == 0).all() and (row[12:20] == 0).all()               # B's ray: free between the marks and before them
    assert (np.delete(together, 16, axis=0) == 255).all() and (row[:12] == 255).all() and (row[25:] == 255).all()
    assert one_after_the_other[16][20] == 0 and one_after_the_other[16][24] == 254   # B's rays erased A's mark: why K11 exists
    assert (one_after_the_other[16][12:24] == 0).all()


def test_every_clear_runs_before_every_mark_in_the_transcription():
    cells, origins = np.zeros((1, TWO_SIZE, TWO_SIZE), dtype=np.uint8), np.zeros((1, 2))
    points, sensors, _ = ref.project(TWO_RANGES, TWO_POSE, [TWO_A, TWO_B])
    assert scan_ref.world_to_map(*points[0, 0, 0], 0.0, 0.0, TWO_RES, TWO_SIZE, TWO_SIZE) == (20, 16)
    assert scan_ref.world_to_map(*points[0, 1, 0], 0.0, 0.0, TWO_RES, TWO_SIZE, TWO_SIZE) == (24, 16)
    assert sensors[0].tolist() == [[16.5, 16.5], [12.5, 16.5]]
    both = ref.LaserScanLayers()
    pool = both.update_sources(cells, origins, TWO_RES, *TWO_INFLATION, points, sensors, **TWO_KW)
    split = ref.LaserScanLayers()
    for s in (0, 1):
        split.update_sources(cells, origins, TWO_RES, *TWO_INFLATION, points[:, s:s + 1], sensors[:, s:s + 1], **TWO_KW)
    check_two_scanners(both.layers[0], split.layers[0])
    assert pool[0, 16, 20] == 254 and pool[0, 16, 24] == 254 and (pool == 254).sum() == 2


# ------------------------------------------------------------------------------------------ ranges for the GPU tests
def special_ranges(rng, shape, sc_min=0.05, sc_max=10.0, high=12.0):
    """float32 ranges [count, sources, beams] from `rng`, most of them valid, with every special value of the contract in
    every scan that has room for them: in the first chunk of 256 beams and, where there is one, in the tail behind it."""
    ranges = rng.uniform(0.0, high, size=shape).astype(F32)
    specials = np.array([np.nan, np.inf, -np.inf, sc_min, sc_max, np.nextafter(F32(sc_min), F32(0.0))], dtype=F32)
    beams = shape[2]
    for at in (3, 257):
        if at + 6 * 7 <= beams:
            ranges[:, :, at:at + 6 * 7:7] = specials
    return ranges


# ------------------------------------------------------------------------------------------ 5: the projection on the device
@functools.lru_cache(maxsize=None)
def projection_case():
    """3 robots, 2 scanners, 300 beams: more than one pass of 256 threads and not a multiple of one."""
    rng = np.random.default_rng(1101)
    ranges = special_ranges(rng, (3, 2, 300))
    xy = rng.uniform(-20.0, 20.0, size=(3, 2))
    yaws = rng.uniform(-math.pi, math.pi, size=(3, 1))
    ranges.setflags(write=False)
    return ranges, xy, yaws


@pytest.mark.gpu
def test_projection_on_the_device():
    """The NaN pattern is the transcription's exactly.  At yaw 0 the device's sincos is exact -- (0, 1) -- so points and
    origins equal the transcription bit for bit.  At random yaws |delta| <= 2^-49 (|x| + |y| + |bx| + |by|) per coordinate,
    derived, not measured: device sincos and libm are each within 1 ulp of the true sine and cosine, so at most 2 ulp <=
    2^-52 apart, which moves bx C and by S by at most 2^-52 (|bx| + |by|); the formula's three roundings on either side add
    at most 2 x 2^-53 (|bx| + (|x| + |bx|) + (|x| + |bx| + |by|)); together below 2^-50 of the sum, and a factor 2 of slack.
    The 1 ulp: the HIP math API reference lists a maximum error of 1 ulp for double-precision sin, cos and sincos; that
    document is not installed next to the compiler used here, so nothing was scaled."""
    import torch
    from neo_mpc_planner2_amd.solver import BatchSolver
    ranges, xy, yaws = projection_case()
    scanners = [FRONT, REAR]
    with BatchSolver({}) as s:
        for name, yaw in (("yaw 0", np.zeros((3, 1))), ("random yaws", yaws)):
            poses = np.concatenate([xy, yaw], 1)
            want_points, want_origins, base = ref.project(ranges, poses, scanners)
            nan = np.isnan(want_points)
            assert nan.any() and not nan.all() and (nan[..., 0] == nan[..., 1]).all()
            for how in ("device", "host"):
                if how == "device":
                    points, origins = s.project_laser(gpu(ranges), gpu(poses), scanners)
                    torch.cuda.synchronize()
                    points, origins = points.cpu().numpy(), origins.cpu().numpy()
                else:
                    points, origins = s.project_laser(ranges, poses, scanners)
                assert np.array_equal(np.isnan(points), nan), (name, how)
                if name == "yaw 0":
                    assert points[~nan].tobytes() == want_points[~nan].tobytes(), (name, how)
                    assert origins.tobytes() == want_origins.tobytes(), (name, how)
                    continue
                scale = np.abs(xy).sum(1)[:, None, None] + np.abs(base).sum(-1)                 # [3, 2, 300]
                err = np.abs(points - want_points).max(-1)
                worst = np.nanmax(err / scale)
                mounts = np.array([[abs(sc["mount_x"]) + abs(sc["mount_y"]) for sc in scanners]])
                err_o = np.abs(origins - want_origins).max(-1) / (np.abs(xy).sum(1)[:, None] + mounts)
                print("%s, %s: worst point error %.3g, worst origin error %.3g of the scale (bound %.3g)" %
                      (name, how, worst, err_o.max(), 2.0 ** -49))
                assert (err[~nan[..., 0]] <= 2.0 ** -49 * scale[~nan[..., 0]]).all(), (name, how)
                assert (err_o <= 2.0 ** -49).all(), (name, how)


# ------------------------------------------------------------------------------------------ 6: the update is the two steps
UPDATE_CASES = [(sx, sy, reach, unknown) for sx, sy in ((96, 80), (64, 64)) for reach in (0, 12) for unknown in (255, 0)]
UPDATE_RES, UPDATE_WINDOWS, UPDATE_BEAMS = 0.05, 4, 90
UPDATE_SCANNERS = [scanner((0.3, 0.1, 0.2), -1.6, 3.2 / 89, 0.05, 6.0, ref.INF_IS_VALID), scanner((-0.3, -0.05, 3.0), -1.6, 3.2 / 89, 0.05, 6.0)]
UPDATE_KW = dict(obstacle_max_range=2.0, obstacle_min_range=0.15, raytrace_max_range=2.4, raytrace_min_range=0.1)
UPDATE_MOVES = (np.zeros((UPDATE_WINDOWS, 2)), np.array([(3.0, -2.7), (-2.7, 3.0), (0.0, 0.0), (140.0, 1.0)]),
                np.array([(5.0, -2.7), (-2.7, 1.0), (0.0, 0.0), (141.0, 1.0)]))


@functools.lru_cache(maxsize=None)
def update_world():
    world = np.random.default_rng(77).choice(np.array([0, 0, 0, 0, 90, 254, 255, 255], dtype=np.uint8), size=(400, 400))
    world.setflags(write=False)
    return world, UPDATE_RES, -10.0, -10.0


@functools.lru_cache(maxsize=None)
def update_ticks(sx, sy, sources=2):
    """Three ticks: (poses [4, 3], ranges [4, sources, 90]); and the windows' start origins.  Ranges up to 3.5 m in windows
    of 4.8 m or 3.2 m: rays end inside and outside, marks fall inside and beyond obstacle_max_range."""
    rng = np.random.default_rng(1000 * sx + sources)
    home = rng.uniform(-4.0, 2.0, size=(UPDATE_WINDOWS, 2))
    start = home - ((sx - 0.5) * UPDATE_RES / 2, (sy - 0.5) * UPDATE_RES / 2) - 0.5 * UPDATE_RES
    ticks = []
    for move in UPDATE_MOVES:
        poses = np.concatenate([home + move * UPDATE_RES, rng.uniform(-3.0, 3.0, size=(UPDATE_WINDOWS, 1))], 1)
        ticks.append((poses, special_ranges(rng, (UPDATE_WINDOWS, sources, UPDATE_BEAMS), 0.05, 6.0, 3.5)))
    return tuple(ticks), start


@pytest.mark.gpu
@pytest.mark.parametrize("sx,sy,reach,unknown", UPDATE_CASES, ids=["%dx%d-R%d-unknown%d" % c for c in UPDATE_CASES])
def test_update_from_ranges_equals_projection_then_the_multi_source_transcription(sx, sy, reach, unknown):
    """Three ticks with a roll in front of each.  The transcription is fed with the pool the roll left and with the points
    and origins the device projected (project_laser, read back), so layers and pool are compared bit for bit wherever the
    points fall."""
    import torch
    from neo_mpc_planner2_amd.solver import BatchSolver
    world, wres, wox, woy = update_world()
    ticks, start = update_ticks(sx, sy)
    params = inflation_for(reach, UPDATE_RES)
    model = ref.LaserScanLayers()
    with BatchSolver({}) as s:
        assert BatchSolver.inflation_costs(UPDATE_RES, *params)[1] == reach
        s.set_world_map(gpu(world), wres, wox, woy)
        d_origins = gpu(start)
        for k, (poses, ranges) in enumerate(ticks):
            d_poses, d_ranges = gpu(poses), gpu(ranges)
            s.roll_costmap_pool(sx, sy, UPDATE_RES, d_origins, poses=d_poses)
            rolled, origins = s.get_costmap_pool()
            points, sensors = s.project_laser(d_ranges, d_poses, UPDATE_SCANNERS)
            torch.cuda.synchronize()
            points, sensors = points.cpu().numpy(), sensors.cpu().numpy()
            want = model.update_sources(rolled, origins, UPDATE_RES, *params, points, sensors, unknown_value=unknown, **UPDATE_KW)
            s.update_scan_layer_from_ranges(*params, d_ranges, d_poses, UPDATE_SCANNERS, unknown_value=unknown, **UPDATE_KW)
            got = window_state(s)
            print("tick %d: %d marks, %d free layer cells, %d window cells changed" %
                  (k, int((model.layers == 254).sum()), int((model.layers == 0).sum()), int((want != rolled).sum())))
            assert (model.layers == 254).any() and (want != rolled).any(), k
            assert got[1].tolist() == origins.tolist() == got[3].tolist(), k
            assert np.array_equal(got[0], model.layers), (k, int((got[0] != model.layers).sum()))
            assert np.array_equal(got[2], want), (k, int((got[2] != want).sum()))
        # the host variant on the last tick, from the layers of the tick before: the same bytes, and the projection handed out
        # (its points are the device's, so the comparison above carries over)
        s.roll_costmap_pool(sx, sy, UPDATE_RES, d_origins, poses=d_poses)
        out_p, out_o = np.zeros((UPDATE_WINDOWS, 2, UPDATE_BEAMS, 2)), np.zeros((UPDATE_WINDOWS, 2, 2))
        s.update_scan_layer_from_ranges(*params, ranges, poses, UPDATE_SCANNERS, unknown_value=unknown, points_out=out_p,
                                        origins_out=out_o, **UPDATE_KW)
        assert out_p.tobytes() == points.tobytes() and out_o.tobytes() == sensors.tobytes()
        again = model.update_sources(rolled, origins, UPDATE_RES, *params, points, sensors, unknown_value=unknown, **UPDATE_KW)
        got = window_state(s)
        assert np.array_equal(got[0], model.layers) and np.array_equal(got[2], again)


# ------------------------------------------------------------------------------------------ 7: one source is K10
@pytest.mark.gpu
def test_one_source_equals_the_update_from_points():
    import torch
    from neo_mpc_planner2_amd.solver import BatchSolver
    sx, sy, reach = 96, 80, 12
    world, wres, wox, woy = update_world()
    ticks, start = update_ticks(sx, sy, 1)
    params = inflation_for(reach, UPDATE_RES)
    with BatchSolver({}) as a, BatchSolver({}) as b:
        origins = []
        for s in (a, b):
            s.set_world_map(gpu(world), wres, wox, woy)
            origins.append(gpu(start))
        for k, (poses, ranges) in enumerate(ticks):
            d_poses, d_ranges = gpu(poses), gpu(ranges)
            for s, o in zip((a, b), origins):
                s.roll_costmap_pool(sx, sy, UPDATE_RES, o, poses=d_poses)
            a.update_scan_layer_from_ranges(*params, d_ranges, d_poses, UPDATE_SCANNERS[:1], **UPDATE_KW)
            points, sensors = b.project_laser(d_ranges, d_poses, UPDATE_SCANNERS[:1])
            b.update_scan_layer(*params, points=points.reshape(UPDATE_WINDOWS, UPDATE_BEAMS, 2),
                                sensor_origins=sensors.reshape(UPDATE_WINDOWS, 2), **UPDATE_KW)
            got, want = window_state(a), window_state(b)
            assert (want[0] == 254).any() and (want[0] == 0).any(), k
            assert same(got, want), k


# ------------------------------------------------------------------------------------------ 8: the two scanners on the device
@pytest.mark.gpu
def test_every_clear_runs_before_every_mark_on_the_device():
    from neo_mpc_planner2_amd.solver import BatchSolver
    cells, origins = np.zeros((1, TWO_SIZE, TWO_SIZE), dtype=np.uint8), np.zeros((1, 2))
    with BatchSolver({}) as s:
        for put in (gpu, np.array):                                       # the device and the host variants
            s.set_costmap_pool(cells, TWO_RES, origins)
            s.reset_scan_layer()
            s.update_scan_layer_from_ranges(*TWO_INFLATION, put(TWO_RANGES), put(TWO_POSE), [TWO_A, TWO_B], **TWO_KW)
            together, pool = window_state(s)[0][0], window_state(s)[2][0]
            s.set_costmap_pool(cells, TWO_RES, origins)
            s.reset_scan_layer()
            for k, sc in enumerate((TWO_A, TWO_B)):
                s.update_scan_layer_from_ranges(*TWO_INFLATION, put(TWO_RANGES[:, k:k + 1]), put(TWO_POSE), [sc], **TWO_KW)
            check_two_scanners(together, window_state(s)[0][0])
            assert pool[16, 20] == 254 and pool[16, 24] == 254 and (pool == 254).sum() == 2


# ------------------------------------------------------------------------------------------ 9: refusals
@pytest.mark.gpu
def test_refusals_leave_pool_layers_and_points_alone():
    import torch
    from neo_mpc_planner2_amd.solver import BatchSolver
    sx, sy = 64, 64
    ticks, start = update_ticks(sx, sy)
    poses, ranges = ticks[0]
    poses, ranges = poses.copy(), ranges.copy()
    params = inflation_for(3, UPDATE_RES)
    cells = np.random.default_rng(3).choice(np.array([0, 0, 90, 254, 255], dtype=np.uint8), size=(UPDATE_WINDOWS, sy, sx))
    sc = abi.scanner_array(UPDATE_SCANNERS)
    host_out = (np.full((UPDATE_WINDOWS, 2, UPDATE_BEAMS, 2), 7.0), np.full((UPDATE_WINDOWS, 2, 2), 7.0))
    bad_poses = poses.copy()
    bad_poses[2, 2] = np.inf
    with BatchSolver({}) as s:
        lib, h = s._lib, s._handle
        dev = (gpu(ranges), gpu(poses), gpu(host_out[0]), gpu(host_out[1]))

        def untouched():
            torch.cuda.synchronize()
            return all((a == 7.0).all() for a in host_out) and bool((dev[2] == 7.0).all()) and bool((dev[3] == 7.0).all())

        def call(entry="update", device=False, scanner_over=None, **over):
            b = abi.NeoMpcLaserBatch()
            scanners = sc.copy()
            for k, v in (scanner_over or {}).items():
                scanners[1][k] = v
            b.count, b.sources, b.beams, b.scanners = UPDATE_WINDOWS, 2, UPDATE_BEAMS, scanners.ctypes.data
            if device:
                b.ranges, b.poses, b.points_out, b.origins_out = (t.data_ptr() for t in dev)
            else:
                b.ranges, b.poses, b.points_out, b.origins_out = ranges.ctypes.data, poses.ctypes.data, host_out[0].ctypes.data, host_out[1].ctypes.data
            b.scan_flags, b.unknown_value = 3, 255
            b.inscribed_radius, b.inflation_radius, b.cost_scaling_factor = params
            for k, v in UPDATE_KW.items():
                setattr(b, k, v)
            for k, v in over.items():
                setattr(b, k, v)
            name = "neo_mpc_update_scan_layer_from_ranges" if entry == "update" else "neo_mpc_project_laser"
            if device:
                return getattr(lib, name + "_device")(h, C.byref(b), None)
            return getattr(lib, name)(h, C.byref(b))

        assert call() == -4 and call(device=True) == -4 and untouched()       # NEO_MPC_ERR_NO_COSTMAP
        s.set_costmap(cells[0], UPDATE_RES, 1.0, 2.0)
        assert call() == -5 and call(device=True) == -5 and untouched()       # a single costmap: NEO_MPC_ERR_UNSUPPORTED
        s.set_costmap_pool(cells, UPDATE_RES, start)
        s.update_scan_layer_from_ranges(*params, ranges, poses, UPDATE_SCANNERS, **UPDATE_KW)   # what the refusals must leave alone
        held = window_state(s)
        assert (held[0] == 254).any() and (held[0] == 0).any()
        nan, inf = float("nan"), float("inf")
        shape_errors = [dict(reserved=1), dict(sources=0), dict(sources=5), dict(beams=0), dict(beams=4097), dict(scanners=None),
                        dict(ranges=None), dict(poses=None)]
        scanner_errors = [dict(flags=2), dict(flags=3), dict(reserved=1), dict(range_min=-0.1), dict(range_max=0.01)]
        for name in ("mount_x", "mount_y", "mount_yaw", "angle_min", "angle_increment", "range_min", "range_max"):
            scanner_errors += [{name: nan}, {name: inf}, {name: -inf}]
        update_errors = [dict(scan_flags=0), dict(scan_flags=4), dict(scan_flags=7), dict(unknown_value=1), dict(unknown_value=254),
                         dict(count=UPDATE_WINDOWS - 1), dict(count=UPDATE_WINDOWS + 1)]
        for name in ("obstacle_max_range", "obstacle_min_range", "raytrace_max_range", "raytrace_min_range",
                     "inscribed_radius", "inflation_radius", "cost_scaling_factor"):
            update_errors += [{name: -0.1}, {name: nan}, {name: inf}]
        for device in (False, True):
            for entry in ("update", "project"):
                errors = [dict(over) for over in shape_errors] + [dict(scanner_over=o) for o in scanner_errors]
                errors += [dict(over) for over in update_errors] if entry == "update" else [dict(points_out=None), dict(origins_out=None)]
                if not device:
                    errors.append(dict(poses=bad_poses.ctypes.data))          # the host variants look at the poses
                else:
                    errors.append(dict(points_out=dev[2].data_ptr() + 8))     # ... the device variants at the alignment
                for over in errors:
                    assert call(entry, device, **over) == -1, (entry, device, over)
                    assert lib.neo_mpc_last_error_code() == -1 and untouched() and same(window_state(s), held), (entry, device, over)
                assert call(entry, device, count=0) == 0 and untouched() and same(window_state(s), held)
            assert call("update", device, inflation_radius=66 * UPDATE_RES) == -5 and untouched()       # 66 cells
            assert same(window_state(s), held)
            for entry in ("update", "project"):
                fn = getattr(lib, "neo_mpc_update_scan_layer_from_ranges" if entry == "update" else "neo_mpc_project_laser")
                assert fn(h, None) == -1 and fn(None, C.byref(abi.NeoMpcLaserBatch())) == -1
        # the projection alone ignores the update's fields and the pool's count, and writes the out buffers
        assert call("project", True, scan_flags=0, unknown_value=9, inflation_radius=nan, count=UPDATE_WINDOWS - 1) == 0
        assert not untouched() and same(window_state(s), held)


# ------------------------------------------------------------------------------------------ 10: graph capture
@pytest.mark.gpu
def test_roll_scan_from_ranges_stamp_gate_solve_can_be_captured_in_a_hip_graph():
    """After one eager call -- it builds the tables and allocates -- roll -> update from ranges -> stamp -> gate -> solve is
    captured on one stream, a linear chain, and replayed twice with ranges and poses rewritten in between; layers, pool,
    gate costs and commands equal the same calls made directly on a second handle."""
    beams = 40
    stamp, scan = (0.45, 0.9, 3.0), (0.1, 0.3, 3.0)
    scanners = [scanner((0.3, 0.0, 0.0), -1.5, 3.0 / 39, 0.05, 5.0, ref.INF_IS_VALID), scanner((-0.3, 0.0, math.pi), -1.5, 3.0 / 39, 0.05, 5.0)]
    f = capture_fleet(120)
    count, sx, sy, res = f.count, f.sx, f.sy, f.res
    rng = np.random.default_rng(94)
    ticks = []
    for k in range(3):
        poses = np.concatenate([f.probs["cur_xy"] + rng.uniform(-0.4, 0.4, size=(count, 2)) * k, rng.uniform(-3, 3, size=(count, 1))], 1)
        ticks.append((poses, special_ranges(rng, (count, 2, beams), 0.05, 5.0, 1.8)))
    fp = gpu(np.asarray(RECT, dtype=np.float64))

    class LaserSide(Side):
        def __init__(self, fleet, tick):
            super().__init__(fleet, tick)
            self.ranges = gpu(tick[1])

        def set_inputs(self, tick):
            super().set_inputs(tick)
            self.ranges.copy_(gpu(tick[1]))

        def tick(self):
            self.s.roll_costmap_pool(sx, sy, res, self.origins, poses=self.poses)
            self.s.update_scan_layer_from_ranges(*scan, self.ranges, self.poses, scanners, obstacle_max_range=1.5,
                                                 raytrace_max_range=1.2, raytrace_min_range=0.1)
            self.s.stamp_fleet(*stamp, footprint=fp, poses=self.poses)
            self.s.footprint_gate_device(fp, self.costs, poses=self.poses, problems=self.b.problems)
            self.s.solve_device(self.b.problems, self.b.states, self.b.warm, self.b.commands, solution=self.b.solution)

        def result(self):
            common = super().result()
            layers, layer_origins = self.s.get_scan_layer()
            return common + (self.s.get_costmap_pool()[0].tobytes(), layers.tobytes(), layer_origins.tolist())

    with replay_against_direct(lambda: LaserSide(f, ticks[0]), ticks, changed=(4, 5)) as (_, a, _):   # pool and layers changed
        layers = np.frombuffer(a[5], dtype=np.uint8).reshape(count, sy, sx)
        assert (layers == 254).any() and (layers == 0).any()


# ------------------------------------------------------------------------------------------ 11: the closed loop
@pytest.mark.gpu
def test_closed_loop_with_laser_ranges_and_without():
    """64 robots on a free world map, each with a wall 0.3 m in front of its centre -- inside its 0.35 m outline -- that exists
    only in its front scanner's ranges: with `laser` the footprint gate finds the wall and the collision latch stops the
    fleet; without it nobody sees anything; laser=None is the loop as it was, bit for bit."""
    import torch
    from neo_mpc_planner2_amd import fleet as fleet_loop
    from neo_mpc_planner2_amd.solver import BatchSolver, DeviceBatch
    from oracle import mpc_oracle as orc
    count, size, res, ticks, beams = 64, 60, 0.05, 4, 61
    world = np.zeros((400, 400), dtype=np.uint8)
    grid = np.stack(np.meshgrid(np.arange(8), np.arange(8)), -1).reshape(-1, 2)
    xy = -7.0 + 2.0 * grid + 0.011
    probs, st, warm = standing_fleet(count, xy, xy + (5.0, 0.0))
    front = scanner((0.1, 0.0, 0.0), -1.2, 2.4 / (beams - 1), 0.05, 8.0)
    rear = scanner((-0.1, 0.0, math.pi), -1.2, 2.4 / (beams - 1), 0.05, 8.0, ref.INF_IS_VALID)
    angle = front["angle_min"] + np.arange(beams) * front["angle_increment"]
    wall = (0.2 / np.cos(angle)).astype(F32)                    # x = 0.1 + 0.2 in the base frame, 1 m wide: across the outline
    ranges = np.empty((count, 2, beams), dtype=F32)
    ranges[:, 0], ranges[:, 1] = wall, np.inf                   # behind: nothing, which clears
    d_ranges = gpu(ranges)
    params = (0.1, 0.3, 3.0)

    def laser(t, poses):
        return dict(zip(("inscribed_radius", "inflation_radius", "cost_scaling_factor"), params), ranges=d_ranges, poses=poses,
                    scanners=[front, rear])

    runs = {}
    with BatchSolver(orc.make_params()) as s:
        s.set_world_map(world, res, -10.0, -10.0)
        for how, kw in (("default", {}), ("none", dict(laser=None)), ("laser", dict(laser=laser))):
            flags = []
            d_orig = gpu(probs["cur_xy"] - size * res / 2 + 0.013)
            s.roll_costmap_pool(size, size, res, d_orig)
            s.reset_scan_layer()
            b = DeviceBatch(probs, st, warm, "cuda:0")
            out = fleet_loop.closed_loop(s, b, ticks, after_tick=lambda t, cm: flags.append(cm.copy()), footprint=RECT,
                                         rolling=(size, size, res, d_orig), **kw)
            torch.cuda.synchronize()
            runs[how] = (out, np.array(flags))
    assert runs["default"][1].tobytes() == runs["none"][1].tobytes()
    free, seen = runs["none"][0], runs["laser"][0]
    print("lethal fraction %s without, %s with; stopped fraction %s without, %s with" %
          (free["footprint_lethal_fraction"], seen["footprint_lethal_fraction"], free["stopped_fraction"], seen["stopped_fraction"]))
    assert max(free["footprint_lethal_fraction"]) == 0.0
    assert min(seen["footprint_lethal_fraction"]) > max(free["footprint_lethal_fraction"])
    assert seen["stopped_fraction"][-1] > free["stopped_fraction"][-1]
