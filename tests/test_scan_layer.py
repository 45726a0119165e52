"""The scan obstacle layer (K10): a persistent layer per rolling window, fed from sensor points -- rolled, cleared along the
rays, marked at their ends, combined into the window and inflated: roll -> scan -> stamp -> gate -> carrots -> solve.

nav2's layers cannot be built here, so the contract is the text in include/neo_mpc.h (neo_mpc_scan_batch) and its executable
form the transcription in tests/scan_layer_reference.py.  The contract's float64 is + - * /, one sqrt of an exact integer and
comparisons, each one correctly rounded operation on both sides, and the rest is integers: every comparison with the
transcription is exact equality of uint8 cells and float64 origins -- no tolerance, no dropped case."""
import collections
import ctypes as C
import functools

import numpy as np
import pytest

from neo_mpc_planner2_amd import abi
from tests import fleet_stamp_reference as stamp_ref
from tests import footprint_gate_reference as gate_ref
from tests import rolling_window_reference as roll_ref
from tests import scan_layer_reference as ref
from tests.c_probe import check_entry_points, check_layout, probe_header
from tests.fleet_kit import RECT, Side, capture_fleet, gpu, inflation_for, replay_against_direct, same, standing_fleet, window_state
from tests.world_scan_cases import distance_64_case

ENTRY_POINTS = ("neo_mpc_update_scan_layer", "neo_mpc_update_scan_layer_device", "neo_mpc_get_scan_layer",
                "neo_mpc_reset_scan_layer")
#: wider than one 64-cell tile, not square, no multiples of 64
SHAPES = {"96x70-5cm": (96, 70, 0.05), "40x40-10cm": (40, 40, 0.1), "130x67-2.5cm": (130, 67, 0.025)}
REACHES = (0, 3, 12, 64)
MAX_POINTS = (1, 64, 130)           # one lane, one full wave, two waves and a tail
WINDOWS = 5
#: shape x R, the three point counts dealt over them
CASES = [(shape, reach, MAX_POINTS[(a + b) % 3]) for a, shape in enumerate(sorted(SHAPES)) for b, reach in enumerate(REACHES)]


# ------------------------------------------------------------------------------------------ 1: the hand-worked map
def test_the_line_walk_on_a_hand_worked_map():
    M, m = 100, 0
    want = {
        (9, 7): [(5, 5), (6, 6), (7, 6), (8, 7), (9, 7)],              # octant 1: x major, up
        (7, 9): [(5, 5), (6, 6), (6, 7), (7, 8), (7, 9)],              # octant 2: y major
        (3, 9): [(5, 5), (4, 6), (4, 7), (3, 8), (3, 9)],              # octant 3
        (1, 7): [(5, 5), (4, 6), (3, 6), (2, 7), (1, 7)],              # octant 4
        (1, 3): [(5, 5), (4, 4), (3, 4), (2, 3), (1, 3)],              # octant 5
        (3, 1): [(5, 5), (4, 4), (4, 3), (3, 2), (3, 1)],              # octant 6
        (7, 1): [(5, 5), (6, 4), (6, 3), (7, 2), (7, 1)],              # octant 7
        (9, 3): [(5, 5), (6, 4), (7, 4), (8, 3), (9, 3)],              # octant 8
        (8, 5): [(5, 5), (6, 5), (7, 5), (8, 5)],                      # along +x
        (5, 2): [(5, 5), (5, 4), (5, 3), (5, 2)],                      # along -y
        (8, 8): [(5, 5), (6, 6), (7, 7), (8, 8)],                      # the tie: x is the major axis
        (5, 5): [(5, 5)],                                              # zero length
    }
    for (x1, y1), cells in want.items():
        assert ref.raytrace_cells(5, 5, x1, y1, M, m) == cells, (x1, y1)
    # cut by raytrace_max_range: dist = 10, M = 5: scale 0.5, n = min(5, (unsigned)(0.5 * 8)) = 4 steps along x
    assert ref.raytrace_cells(0, 0, 8, 6, 5, 0) == [(0, 0), (1, 1), (2, 2), (3, 2), (4, 3)]
    # dropped by raytrace_min_range: dist = 5 < m = 6
    assert ref.raytrace_cells(0, 0, 3, 4, 100, 6) == []
    # the start moved by m = 5 along a ray of dist = 10: (u0, v0) = (0 + 0.8 * 5, 0 + 0.6 * 5) = (4, 3)
    assert ref.raytrace_cells(0, 0, 8, 6, 100, 5) == [(4, 3), (5, 4), (6, 5), (7, 5), (8, 6)]
    # ... and on a map: a 3 x 8 layer at (1, 2), 0.5 m cells; one ray from cell (0, 1) to a point beyond the right edge
    layer = np.full((3, 8), 255, dtype=np.uint8)
    ref.clear_by_definition(layer, (1.0, 2.0), 0.5, [(7.25, 2.75)], (1.25, 2.75), 100.0, 0.0)
    assert layer.tolist() == [[255] * 8, [0] * 8, [255] * 8]           # clipped to ex - 0.001: the row's last cell
    ref.mark_by_definition(layer, (1.0, 2.0), 0.5, [(7.25, 2.75), (2.3, 3.4), (1.3, 2.8)], (1.25, 2.75), 10.0, 0.5)
    assert layer.tolist() == [[255] * 8, [0] * 8, [255, 255, 254] + [255] * 5]   # off the map, marked, nearer than min
    assert ref.cell_distance(1.0, 0.3) == 4 and ref.cell_distance(0.0, 0.3) == 0
    assert ref.world_to_map(0.99, 2.0, 1.0, 2.0, 0.5, 8, 3) is None and ref.world_to_map(5.0, 2.0, 1.0, 2.0, 0.5, 8, 3) is None
    assert ref.world_to_map(4.99, 3.49, 1.0, 2.0, 0.5, 8, 3) == (7, 2) and ref.world_to_map(float("nan"), 2.0, 1.0, 2.0, 0.5, 8, 3) is None
    assert ref.combine_into(np.array([[255, 255, 255, 10, 0, 253, 254]], dtype=np.uint8),
                            np.array([[255, 0, 254, 0, 254, 254, 0]], dtype=np.uint8)).tolist() == [[255, 0, 254, 10, 254, 254, 254]]
    old = np.array([[255, 255, 255, 255, 255, 255]], dtype=np.uint8)
    rolled = ref.roll_layer(np.array([[1, 2, 3, 4, 5, 6]], dtype=np.uint8), (0.0, 0.0), (1.0, 0.0), 0.5, 255)
    assert rolled.tolist() == [[3, 4, 5, 6, 255, 255]]                  # the window moved two cells to the right
    assert ref.roll_layer(old * 0, (0.0, 0.0), (3.0, 0.0), 0.5, 255).tolist() == old.tolist()   # ... six: beyond it
    assert ref.shift_of(1.25, 0.0, 0.5, 6) == 2 and ref.shift_of(1.75, 0.0, 0.5, 6) == 4          # ties to even


# ------------------------------------------------------------------------------------------ 2: record and entry points
def test_scan_batch_layout_and_entry_points(tmp_path):
    got = probe_header(tmp_path, ["neo_mpc_scan_batch"], ["MAX_SCAN_POINTS", "SCAN_CLEAR", "SCAN_MARK"], ENTRY_POINTS)
    check_layout(got, "neo_mpc_scan_batch", 104, struct=abi.NeoMpcScanBatch, dtype=abi.SCAN_BATCH_DTYPE)
    assert got["MAX_SCAN_POINTS"] == abi.MAX_SCAN_POINTS == 8192 and got["SCAN_CLEAR"] == abi.SCAN_CLEAR == 1 and got["SCAN_MARK"] == abi.SCAN_MARK == 2
    assert len(ENTRY_POINTS) == 4
    check_entry_points(ENTRY_POINTS)


# ------------------------------------------------------------------------------------------ the generator
def ranges_for(shape):
    sx, sy, res = SHAPES[shape]
    span = max(sx, sy) * res
    return dict(obstacle_max_range=0.45 * span, obstacle_min_range=3 * res, raytrace_max_range=0.4 * span,
                raytrace_min_range=2 * res)


@functools.lru_cache(maxsize=None)
def case(shape, max_points):
    """(cells [5, sy, sx], origins [5, 2], points [5, max_points, 2], point_counts [5], sensor_origins [5, 2]).  Window 0:
    the sensor near the middle and points far beyond every edge and corner; 1: the sensor off the map; 2: no points;
    3: at the origin of the frame, two points whose clipped image lies on the upper edge exactly; 4: points that are not
    finite, nearer than obstacle_min_range and beyond obstacle_max_range.  Everything else at random around the sensors,
    many of them outside the windows."""
    sx, sy, res = SHAPES[shape]
    rng = np.random.default_rng(1000 * sx + max_points)
    cells = rng.choice(np.array([0, 0, 0, 0, 60, 150, 253, 254, 255, 255, 255], dtype=np.uint8), size=(WINDOWS, sy, sx))
    origins = rng.uniform(-5.0, 5.0, size=(WINDOWS, 2))
    origins[3] = (0.0, 0.0)
    span = np.array([sx * res, sy * res])
    sensors = origins + span * rng.uniform(0.3, 0.7, size=(WINDOWS, 2))
    sensors[1] = origins[1] + span * (-0.2, 0.5)
    sensors[3] = (1.0, 1.0)
    angle = rng.uniform(0.0, 2 * np.pi, size=(WINDOWS, max_points))
    radius = rng.uniform(0.0, 1.2 * span.max(), size=(WINDOWS, max_points))
    points = sensors[:, None, :] + radius[..., None] * np.stack([np.cos(angle), np.sin(angle)], -1)
    counts = np.array([max_points, max_points, 0, max_points, max_points - max_points // 3], dtype=np.uint32)
    if max_points >= 8:
        for j, (dx, dy) in enumerate(((-3, 0.1), (3, -0.1), (0.1, -3), (-0.1, 3), (-3, -3), (3, 3), (-3, 3), (3, -3))):
            points[0, j] = sensors[0] + span * (dx, dy)
        ex, ey = 0.0 + sx * res, 0.0 + sy * res
        points[3, 0] = (2 * ex - 1.0, 2 * ey - 1.0)           # clipped at ex: t = 1/2, wy = ey exactly
        points[3, 1] = (-1.0, 2 * ey - 1.0)                   # clipped at ox: t = 1/2, wy = ey exactly
        points[4, 0] = (np.nan, sensors[4, 1])
        points[4, 1] = (sensors[4, 0], np.inf)
        points[4, 2] = sensors[4] + (res, 0.0)
        points[4, 3] = sensors[4] + (0.3 * span[0], 0.0)      # (in the window; beyond 0.45 x the longer side or not)
        points[1, 0] = sensors[1] + (0.3 * span[0], 0.0)      # in window 1, seen from outside it
    for a in (cells, origins, points, counts, sensors):
        a.setflags(write=False)
    return cells, origins, points, counts, sensors


@functools.lru_cache(maxsize=None)
def expected(shape, reach, max_points, by_definition=False):
    """The transcription on a case: (layers, pool, the branches taken -- by definition only)."""
    cells, origins, points, counts, sensors = case(shape, max_points)
    stats = collections.Counter() if by_definition else None
    model = ref.ScanLayers()
    pool = model.update(cells, origins, SHAPES[shape][2], *inflation_for(reach, SHAPES[shape][2]), points=points,
                        sensor_origins=sensors, point_counts=counts, by_definition=by_definition, stats=stats,
                        **ranges_for(shape))
    model.layers.setflags(write=False)
    pool.setflags(write=False)
    return model.layers, pool, stats


# three ticks on a world map: the poses, in cells relative to the first tick, and what the scan step is asked for
TICK_SHAPE = "96x70-5cm"
TICK_MOVES = (np.zeros((WINDOWS, 2)),
              np.array([(3.0, -2.7), (-2.7, 3.0), (0.0, 0.0), (140.0, 1.0), (3.0, -2.7)]),
              np.array([(3.0, -2.7), (-2.7, 3.0), (0.0, 0.0), (140.0, 1.0), (3.0, -2.7)]))
TICK_FLAGS = (ref.CLEAR | ref.MARK, 0, ref.CLEAR)
TICK_REACH = 12


@functools.lru_cache(maxsize=None)
def tick_world():
    world = np.random.default_rng(77).choice(np.array([0, 0, 0, 0, 90, 254, 255, 255], dtype=np.uint8), size=(400, 400))
    world.setflags(write=False)
    return world, 0.05, -10.0, -10.0


@functools.lru_cache(maxsize=None)
def tick_inputs():
    """Per tick: (poses [5, 3], points [5, 64, 2], sensor origins [5, 2]); and the windows' start origins."""
    sx, sy, res = SHAPES[TICK_SHAPE]
    rng = np.random.default_rng(78)
    home = rng.uniform(-4.0, 2.0, size=(WINDOWS, 2))
    start = home - ((sx - 0.5) * res / 2, (sy - 0.5) * res / 2) - 0.5 * res     # (the roll's quotient starts at one half)
    ticks = []
    first = None
    for move in TICK_MOVES:
        xy = home + move * res
        poses = np.concatenate([xy, np.zeros((WINDOWS, 1))], 1)
        if first is None:
            angle = rng.uniform(0.0, 2 * np.pi, size=(WINDOWS, 64))
            first = xy[:, None, :] + rng.uniform(0.3, 1.6, size=(WINDOWS, 64))[..., None] * np.stack([np.cos(angle), np.sin(angle)], -1)
            points = first
        else:
            points = xy[:, None, :] + 1.3 * (first - xy[:, None, :])         # beyond the first tick's marks, through them
        ticks.append((poses, points.copy(), xy.copy()))
    return tuple(ticks), start


@functools.lru_cache(maxsize=None)
def expected_ticks(by_definition=False):
    """Per tick: (window origins, layers, pool after the update, pool the roll left); and the branches."""
    sx, sy, res = SHAPES[TICK_SHAPE]
    world, wres, wox, woy = tick_world()
    ticks, origins = tick_inputs()
    stats = collections.Counter() if by_definition else None
    model = ref.ScanLayers()
    out = []
    for (poses, points, sensors), flags in zip(ticks, TICK_FLAGS):
        origins, rolled = roll_ref.roll(world, wres, wox, woy, origins, sx, sy, res, poses=poses, outside_value=255)
        pool = model.update(rolled, origins, res, *inflation_for(TICK_REACH, res), points=points, sensor_origins=sensors,
                            flags=flags, by_definition=by_definition, stats=stats, **ranges_for(TICK_SHAPE))
        out.append((origins.copy(), model.layers.copy(), pool, rolled))
    return out, stats


# ------------------------------------------------------------------------------------------ 3: the two transcriptions
def test_the_array_transcription_equals_the_definition():
    for shape, reach, max_points in CASES:
        a, b = expected(shape, reach, max_points), expected(shape, reach, max_points, True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (shape, reach, max_points)
    for a, b in zip(expected_ticks()[0], expected_ticks(True)[0]):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # ... and on rays alone, from anywhere to anywhere, every range
    rng = np.random.default_rng(5)
    for _ in range(40):
        sx, sy = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        res = float(rng.choice([0.05, 0.1, 0.025, 0.3]))
        origin = rng.uniform(-3, 3, size=2)
        span = np.array([sx, sy]) * res
        sensor = origin + span * rng.uniform(-0.1, 1.1, size=2)
        points = sensor + rng.uniform(-2, 2, size=(50, 2)) * span
        args = (origin, res, points, sensor, float(rng.uniform(0, 2) * span.max()), float(rng.uniform(0, 0.5) * span.max()))
        layers = [np.full((sy, sx), 255, dtype=np.uint8) for _ in range(2)]
        ref.clear(layers[0], *args)
        ref.clear_by_definition(layers[1], *args)
        assert np.array_equal(layers[0], layers[1])
        ref.mark(layers[0], *args)
        ref.mark_by_definition(layers[1], *args)
        assert np.array_equal(layers[0], layers[1])


# ------------------------------------------------------------------------------------------ 4: the generator has teeth
def test_the_cases_take_every_branch():
    stats = collections.Counter()
    for shape, reach, max_points in CASES:
        stats.update(expected(shape, reach, max_points, True)[2])
    ticks, tick_stats = expected_ticks(True)
    stats.update(tick_stats)
    print(dict(stats))
    for name in ("clip wx < ox", "clip wy < oy", "clip wx > ex", "clip wy > ey", "sensor origin off the map",
                 "marked from a sensor origin off the map", "clipped point off the map", "point not finite",
                 "mark dropped: >= max", "mark dropped: < min", "mark dropped: off the map", "marked",
                 "ray walked", "ray cut by raytrace_max_range", "ray dropped by raytrace_min_range",
                 "combine: v == 255", "combine: old == 255", "combine: old < v", "combine: old >= v",
                 "inflate: old == 255, cost >= 253", "inflate: old == 255, cost < 253",
                 "shift x +", "shift x -", "shift x 0", "shift y +", "shift y -", "shift y 0", "shift beyond the window", "reset"):
        assert stats[name] > 0, name
    # the ticks are what they say: windows 0 and 4 move by (+3, -2) cells, 1 by (-2, +3), 2 stays, 3 leaves; then nobody moves
    res = SHAPES[TICK_SHAPE][2]
    moved = np.rint((ticks[1][0] - ticks[0][0]) / res).astype(int).tolist()
    assert moved[0] == [3, -2] and moved[1] == [-2, 3] and moved[2] == [0, 0] and moved[3][0] > 96 and moved[4] == [3, -2]
    assert ticks[2][0].tolist() == ticks[1][0].tolist()
    # the layer came along: tick 2 (flags 0) holds tick 1's marks at their new cells, tick 3 cleared some of them
    assert not np.array_equal(ticks[1][1][0], ticks[0][1][0])                     # (not in place ...)
    assert np.array_equal(ticks[1][1][0][2:, :-3], ticks[0][1][0][:-2, 3:])       # new (i, l) = old (i + 3, l - 2)
    assert (ticks[1][1][3] == 255).all()
    marks = [int((t[1] == 254).sum()) for t in ticks]
    assert marks[0] > 0 and marks[2] < marks[1] <= marks[0]


# ------------------------------------------------------------------------------------------ 5: one update
@pytest.mark.gpu
@pytest.mark.parametrize("shape,reach,max_points", CASES, ids=["%s-R%d-%dpoints" % c for c in CASES])
def test_update_equals_the_transcription(shape, reach, max_points):
    from neo_mpc_planner2_amd.solver import BatchSolver
    sx, sy, res = SHAPES[shape]
    cells, origins, points, counts, sensors = case(shape, max_points)
    want_layers, want_pool, _ = expected(shape, reach, max_points)
    params, ranges = inflation_for(reach, res), ranges_for(shape)
    assert BatchSolver.inflation_costs(res, *params)[1] == reach
    with BatchSolver({}) as s:
        s.set_costmap_pool(cells, res, origins)
        d = (gpu(points), gpu(sensors), gpu(counts, np.int32))
        s.update_scan_layer(*params, points=d[0], sensor_origins=d[1], point_counts=d[2], **ranges)
        first = window_state(s)
        print("%s R=%d %d points: %d layer cells set, %d window cells change" %
              (shape, reach, max_points, int((want_layers != 255).sum()), int((want_pool != cells).sum())))
        assert np.array_equal(first[0], want_layers), int((first[0] != want_layers).sum())
        assert first[1].tolist() == origins.tolist() == first[3].tolist()
        assert np.array_equal(first[2], want_pool), int((first[2] != want_pool).sum())
        # idempotence: the same batch again, no roll in between
        s.update_scan_layer(*params, points=d[0], sensor_origins=d[1], point_counts=d[2], **ranges)
        assert same(window_state(s), first)
        # the host variant, from scratch: identical bytes
        s.set_costmap_pool(cells, res, origins)
        s.reset_scan_layer()
        s.update_scan_layer(*params, points=points, sensor_origins=sensors, point_counts=counts, **ranges)
        assert same(window_state(s), first)


@pytest.mark.gpu
def test_a_sensor_origin_that_is_not_finite_clears_nothing_on_the_device():
    from neo_mpc_planner2_amd.solver import BatchSolver
    shape, reach, max_points = "40x40-10cm", 3, 64
    sx, sy, res = SHAPES[shape]
    cells, origins, points, counts, sensors = case(shape, max_points)
    sensors = sensors.copy()
    sensors[0, 0] = np.nan
    big = np.full(WINDOWS, 1000, dtype=np.int32)                      # counts beyond max_points are clamped to it
    params, ranges = inflation_for(reach, res), ranges_for(shape)
    model = ref.ScanLayers()
    want_pool = model.update(cells, origins, res, *params, points=points, sensor_origins=sensors, **ranges)
    assert not (model.layers[0] == 0).any()
    with BatchSolver({}) as s:
        s.set_costmap_pool(cells, res, origins)
        s.update_scan_layer(*params, points=gpu(points), sensor_origins=gpu(sensors), point_counts=gpu(big), **ranges)
        got = window_state(s)
        assert np.array_equal(got[0], model.layers) and np.array_equal(got[2], want_pool)


# ------------------------------------------------------------------------------------------ 6: three ticks
@pytest.mark.gpu
def test_three_ticks_roll_the_layer_with_its_window():
    from neo_mpc_planner2_amd.solver import BatchSolver
    sx, sy, res = SHAPES[TICK_SHAPE]
    world, wres, wox, woy = tick_world()
    ticks, start = tick_inputs()
    want, _ = expected_ticks()
    params, ranges = inflation_for(TICK_REACH, res), ranges_for(TICK_SHAPE)
    with BatchSolver({}) as s:
        s.set_world_map(gpu(world), wres, wox, woy)
        d_origins = gpu(start)
        for k, ((poses, points, sensors), flags) in enumerate(zip(ticks, TICK_FLAGS)):
            s.roll_costmap_pool(sx, sy, res, d_origins, poses=gpu(poses))
            call = lambda: s.update_scan_layer(*params, points=gpu(points), sensor_origins=gpu(sensors), flags=flags, **ranges)
            call()
            got = window_state(s)
            assert got[3].tolist() == want[k][0].tolist() == got[1].tolist(), k
            assert np.array_equal(got[0], want[k][1]), (k, int((got[0] != want[k][1]).sum()))
            assert np.array_equal(got[2], want[k][2]), (k, int((got[2] != want[k][2]).sum()))
            call()                                                  # repeated: nothing changes
            assert same(window_state(s), got), k


# ------------------------------------------------------------------------------------------ 7: unknown_value
@pytest.mark.gpu
def test_unknown_value_0_frees_unknown_ground_and_a_change_resets_the_layer():
    from neo_mpc_planner2_amd.solver import BatchSolver
    shape, reach, max_points = "40x40-10cm", 3, 64
    sx, sy, res = SHAPES[shape]
    cells, origins, points, counts, sensors = case(shape, max_points)
    params, ranges = inflation_for(reach, res), ranges_for(shape)
    model = ref.ScanLayers()
    assert (cells == 255).any()
    with BatchSolver({}) as s:
        seen = {}
        for step, (unknown, with_points) in enumerate(((255, True), (0, False), (255, False))):
            s.set_costmap_pool(cells, res, origins)
            kw = dict(points=gpu(points), sensor_origins=gpu(sensors)) if with_points else dict(on_device=True)
            s.update_scan_layer(*params, unknown_value=unknown, **kw, **ranges)
            want = model.update(cells, origins, res, *params, unknown_value=unknown, **ranges,
                                **(dict(points=points, sensor_origins=sensors) if with_points else {}))
            got = window_state(s)
            assert np.array_equal(got[0], model.layers) and np.array_equal(got[2], want), step
            seen[step] = got
        assert (seen[0][0] == 254).any() and (seen[0][2] == 255).any()
        assert (seen[1][0] == 0).all() and not (seen[1][2] == 255).any()       # reset to 0: the marks are gone, nothing unknown
        assert (seen[2][0] == 255).all() and np.array_equal(seen[2][2], cells)  # reset to 255: the layer says nothing


# ------------------------------------------------------------------------------------------ 8: scan, then stamp
@pytest.mark.gpu
def test_scan_then_stamp_is_the_two_transcriptions_composed_and_the_order_matters():
    from neo_mpc_planner2_amd.solver import BatchSolver
    sx, sy, res = 96, 70, 0.05
    stamp = (0.45, 0.9, 3.0)
    scan = (0.1, 0.3, 3.0)
    cells = np.full((2, sy, sx), 255, dtype=np.uint8)                   # unknown ground
    origins = np.array([(0.0, 0.0), (0.4, 0.2)])
    poses = np.array([(1.0, 1.75, 0.0), (3.0, 1.75, 0.0)])              # two robots 2 m apart, in each other's window
    sensors = poses[:, :2].copy()
    angle = np.linspace(0.0, 2 * np.pi, 48, endpoint=False)
    points = sensors[:, None, :] + 2.2 * np.stack([np.cos(angle), np.sin(angle)], -1)[None]
    ranges = dict(obstacle_max_range=2.5, obstacle_min_range=0.0, raytrace_max_range=3.0, raytrace_min_range=0.0)
    with BatchSolver({}) as s:
        s.set_costmap_pool(cells, res, origins)
        _, polygons = s.footprint_gate(np.asarray(RECT), poses=poses, map_indices=np.arange(2, dtype=np.int32), want_polygons=True)
        scanned = ref.ScanLayers().update(cells, origins, res, *scan, points=points, sensor_origins=sensors, **ranges)
        want = stamp_ref.stamp_pool(scanned, origins, res, polygons, *stamp)
        s.update_scan_layer(*scan, points=points, sensor_origins=sensors, **ranges)
        s.stamp_fleet(*stamp, polygons=polygons)
        assert np.array_equal(s.get_costmap_pool()[0], want)
        # the other order: the rays free cells the stamp's ring had to leave at 255, and the ring is lost there
        s.set_costmap_pool(cells, res, origins)
        s.reset_scan_layer()
        s.stamp_fleet(*stamp, polygons=polygons)
        s.update_scan_layer(*scan, points=points, sensor_origins=sensors, **ranges)
        other = s.get_costmap_pool()[0]
        stamped_first = ref.ScanLayers().update(stamp_ref.stamp_pool(cells, origins, res, polygons, *stamp), origins, res, *scan,
                                                points=points, sensor_origins=sensors, **ranges)
        assert np.array_equal(other, stamped_first)
        lost = (want > 0) & (want < 253) & (other == 0)
        assert lost.any() and not np.array_equal(other, want)


# ------------------------------------------------------------------------------------------ 9: refusals
@pytest.mark.gpu
def test_refusals_leave_pool_and_layer_alone():
    from neo_mpc_planner2_amd.solver import BatchSolver
    shape, max_points = "40x40-10cm", 64
    sx, sy, res = SHAPES[shape]
    cells, origins, points, counts, sensors = case(shape, max_points)
    params, ranges = inflation_for(3, res), ranges_for(shape)
    points, sensors, counts = points.copy(), sensors.copy(), counts.copy()
    bad_counts, bad_sensors = counts.copy(), sensors.copy()
    bad_counts[4] = max_points + 1
    bad_sensors[2, 1] = np.inf
    with BatchSolver({}) as s:
        lib, h = s._lib, s._handle

        def call(device=False, **over):
            b = abi.NeoMpcScanBatch()
            b.count, b.points, b.point_counts, b.sensor_origins = WINDOWS, points.ctypes.data, counts.ctypes.data, sensors.ctypes.data
            b.max_points, b.flags, b.unknown_value = max_points, 3, 255
            b.inscribed_radius, b.inflation_radius, b.cost_scaling_factor = params
            for k, v in ranges.items():
                setattr(b, k, v)
            for k, v in over.items():
                setattr(b, k, v)
            if device:
                return lib.neo_mpc_update_scan_layer_device(h, C.byref(b), None)
            return lib.neo_mpc_update_scan_layer(h, C.byref(b))

        assert call() == -4 and call(device=True) == -4                     # NEO_MPC_ERR_NO_COSTMAP
        assert lib.neo_mpc_get_scan_layer(h, 0, 1, None, None) == -4        # ... and no layer yet
        s.set_costmap(cells[0], res, 1.0, 2.0)
        assert call() == -5 and call(device=True) == -5                     # a single costmap: NEO_MPC_ERR_UNSUPPORTED
        s.set_costmap_pool(cells, res, origins)
        assert call() == 0                                                  # the layer the refusals must leave alone
        held = window_state(s)
        assert (held[0] == 254).any() and (held[0] == 0).any()
        shape_errors = [dict(reserved=1), dict(flags=4), dict(flags=7), dict(unknown_value=1), dict(unknown_value=254),
                        dict(max_points=8193), dict(points=None), dict(sensor_origins=None), dict(count=4), dict(count=6)]
        for name in ("obstacle_max_range", "obstacle_min_range", "raytrace_max_range", "raytrace_min_range",
                     "inscribed_radius", "inflation_radius", "cost_scaling_factor"):
            shape_errors += [{name: -0.1}, {name: float("nan")}, {name: float("inf")}]
        values = [dict(point_counts=bad_counts.ctypes.data), dict(sensor_origins=bad_sensors.ctypes.data)]
        for over in shape_errors + values:                                  # the host variant looks at the values too
            assert call(**over) == -1, over
            assert lib.neo_mpc_last_error_code() == -1 and same(window_state(s), held), over
        for over in shape_errors:                                           # the device variant: the record's shape alone
            assert call(device=True, **over) == -1, over
            assert same(window_state(s), held), over
        assert lib.neo_mpc_update_scan_layer(h, None) == -1 and lib.neo_mpc_update_scan_layer_device(h, None, None) == -1
        assert lib.neo_mpc_update_scan_layer(None, C.byref(abi.NeoMpcScanBatch())) == -1
        assert lib.neo_mpc_reset_scan_layer(None) == -1 and lib.neo_mpc_get_scan_layer(None, 0, 1, None, None) == -1
        assert lib.neo_mpc_get_scan_layer(h, 3, 3, None, None) == -1
        for device in (False, True):
            assert call(device, inflation_radius=6.6) == -5                 # 66 cells at 10 cm
            assert same(window_state(s), held)
            assert call(device, count=0) == 0 and same(window_state(s), held)   # nothing to do
        assert call(flags=0, points=None, sensor_origins=None, point_counts=None) == 0    # flags 0 needs no pointers
        assert same(window_state(s), held)                                # ... and is the idempotent repeat here


# ------------------------------------------------------------------------------------------ 10: the tick sees the obstacle
@pytest.mark.gpu
def test_gate_and_solve_see_the_scanned_wall():
    """World all free.  A scanned wall crosses A's path half the solver's reach ahead of A's cell; B stands on the wall.
    roll -> scan -> gate -> solve: A's command says a wall is in reach, B's gate cost is 254 and its collision latch stops
    it; the same tick without the update does none of it."""
    import torch
    from neo_mpc_planner2_amd.solver import BatchSolver, DeviceBatch
    from oracle import mpc_oracle as orc
    size, res = 100, 0.05
    world = np.zeros((400, 400), dtype=np.uint8)
    params = (0.1, 0.3, 3.0)
    with BatchSolver(orc.make_params()) as s:
        s.set_world_map(world, res, -10.0, -10.0)
        a_xy = np.array([0.012, 0.017])
        start = np.array([a_xy - size * res / 2 + 0.013] * 2)
        s.roll_costmap_pool(size, size, res, start.copy(), poses=np.array([(a_xy[0], a_xy[1], 0.0)] * 2))
        half = s.kernel_info()["reach_cells"] // 2
        assert half >= 1
        o_a = roll_ref.move_origin(start[0], a_xy, size, size, res)
        a_i, a_l = int((a_xy[0] - o_a[0]) / res), int((a_xy[1] - o_a[1]) / res)
        wall_x = o_a[0] + (a_i + half + 0.5) * res                      # the centres of column a_i + half
        wall = np.array([(wall_x, o_a[1] + (a_l + j + 0.5) * res) for j in range(-12, 13)])
        poses = np.array([(a_xy[0], a_xy[1], 0.0), (wall_x, a_xy[1], 0.0)])
        points = np.stack([wall, wall])
        probs, st, warm = standing_fleet(2, poses[:, :2], poses[:, :2] + (5.0, 0.0), seed=5)
        base, d_poses = gpu(np.asarray(RECT, dtype=np.float64)), gpu(poses)
        out = {}
        for scan in (False, True):
            d_orig = gpu(start)
            b = DeviceBatch(probs, st, warm, "cuda:0")
            costs = torch.zeros(2, dtype=torch.float64, device="cuda:0")
            s.roll_costmap_pool(size, size, res, d_orig, poses=d_poses)
            if scan:
                s.update_scan_layer(*params, points=gpu(points), sensor_origins=gpu(poses[:, :2]))
            s.footprint_gate_device(base, costs, poses=d_poses, problems=b.problems)
            s.solve_device(b.problems, b.states, b.warm, b.commands)
            torch.cuda.synchronize()
            out[scan] = (b.commands_host().copy(), costs.cpu().numpy(), s.get_costmap_pool())
    cells, origins = out[True][2]
    assert not out[False][2][0].any() and origins.tolist() == out[False][2][1].tolist() and origins[0].tolist() == list(o_a)
    model = ref.ScanLayers()
    want = model.update(out[False][2][0], origins, res, *params, points=points, sensor_origins=poses[:, :2])
    assert np.array_equal(cells, want)
    assert (model.layers[0][a_l - 12:a_l + 13, a_i + half] == 254).all() and not (model.layers[0][:, :a_i + half] == 254).any()
    gate = gate_ref.gate(want, res, origins, poses, np.asarray(RECT), map_indices=np.arange(2))
    print("reach %d cells, gate costs %s, flags %s" % (2 * half, out[True][1].tolist(), out[True][0]["flags"].tolist()))
    assert out[True][1].tolist() == gate.tolist() and gate[1] == 254.0 and not out[False][1].any()
    assert out[True][0]["flags"][0] & abi.FLAG_WALL_IN_REACH and not out[False][0]["flags"][0] & abi.FLAG_WALL_IN_REACH
    assert out[True][0]["flags"][1] & abi.FLAG_STOPPED and not out[False][0]["flags"][1] & abi.FLAG_STOPPED
    assert not out[True][0]["vel"][1].any() and out[False][0]["vel"][1].any()


# ------------------------------------------------------------------------------------------ 11: graph capture
@pytest.mark.gpu
def test_roll_scan_stamp_gate_solve_can_be_captured_in_a_hip_graph():
    """After one eager call -- it builds the cost tables and allocates -- roll -> scan -> stamp -> gate -> solve is captured
    on one stream, a linear chain, and replayed with points and poses rewritten in between; layers, pool, gate costs and
    commands equal the same calls made directly on a second handle."""
    n_points = 40
    stamp, scan = (0.45, 0.9, 3.0), (0.1, 0.3, 3.0)
    f = capture_fleet(120)
    count, sx, sy, res = f.count, f.sx, f.sy, f.res
    rng = np.random.default_rng(94)
    ticks = []
    for k in range(3):
        poses = np.concatenate([f.probs["cur_xy"] + rng.uniform(-0.4, 0.4, size=(count, 2)) * k, rng.uniform(-3, 3, size=(count, 1))], 1)
        angle = rng.uniform(0, 2 * np.pi, size=(count, n_points))
        points = poses[:, None, :2] + rng.uniform(0.2, 1.6, size=(count, n_points))[..., None] * np.stack([np.cos(angle), np.sin(angle)], -1)
        ticks.append((poses, points))
    fp = gpu(np.asarray(RECT, dtype=np.float64))

    class ScanSide(Side):
        def __init__(self, fleet, tick):
            super().__init__(fleet, tick)
            self.points = gpu(tick[1])
            self.sensors = self.poses[:, :2].contiguous()

        def set_inputs(self, tick):
            super().set_inputs(tick)
            self.points.copy_(gpu(tick[1]))
            self.sensors.copy_(self.poses[:, :2])

        def tick(self):
            self.s.roll_costmap_pool(sx, sy, res, self.origins, poses=self.poses)
            self.s.update_scan_layer(*scan, points=self.points, sensor_origins=self.sensors, obstacle_max_range=1.5,
                                     raytrace_max_range=1.2, raytrace_min_range=0.1)
            self.s.stamp_fleet(*stamp, footprint=fp, poses=self.poses)
            self.s.footprint_gate_device(fp, self.costs, poses=self.poses, problems=self.b.problems)
            self.s.solve_device(self.b.problems, self.b.states, self.b.warm, self.b.commands, solution=self.b.solution)

        def result(self):
            common = super().result()
            layers, layer_origins = self.s.get_scan_layer()
            return common + (self.s.get_costmap_pool()[0].tobytes(), layers.tobytes(), layer_origins.tolist())

    with replay_against_direct(lambda: ScanSide(f, ticks[0]), ticks, changed=(4, 5)) as (_, a, _):   # pool and layers changed
        # ... and the layers are persistent ones: the last tick's hold marks no point of that tick explains
        layers = np.frombuffer(a[5], dtype=np.uint8).reshape(count, sy, sx)
        alone = ref.ScanLayers()
        raw_origins = np.array(a[3])
        alone.update(np.zeros((count, sy, sx), dtype=np.uint8), raw_origins, res, *scan, points=ticks[2][1],
                     sensor_origins=ticks[2][0][:, :2], obstacle_max_range=1.5, raytrace_max_range=1.2, raytrace_min_range=0.1)
        assert ((layers == 254) & (alone.layers != 254)).any()


# ------------------------------------------------------------------------------------------ 12: the closed loop
@pytest.mark.gpu
def test_closed_loop_with_a_scan_and_without():
    """A robot drives at a wall only its scanner sees (the world map is free): with `scan` the collision latch stops it short
    of the wall, without it the robot drives through; and scan=None is the loop as it was, bit for bit."""
    import torch
    from neo_mpc_planner2_amd import fleet as fleet_loop
    from neo_mpc_planner2_amd.solver import BatchSolver, DeviceBatch
    from oracle import mpc_oracle as orc
    size, res, ticks = 100, 0.05, 100
    world = np.zeros((400, 400), dtype=np.uint8)
    probs, st, warm = standing_fleet(2, ((-2.0, 0.011), (-2.0, 4.011)), ((6.0, 0.011), (6.0, 4.011)))
    wall_x = -1.2
    wall = np.array([[(wall_x, y0 + j * res / 2) for j in range(-40, 41)] for y0 in (0.011, 4.011)])
    d_wall = gpu(wall)
    params = (0.45, 0.9, 3.0)

    def scan(t, poses):
        if t % 3:                                # scans at a third of the tick rate: in between the layer is put back
            return dict(zip(("inscribed_radius", "inflation_radius", "cost_scaling_factor"), params), on_device=True)
        return dict(zip(("inscribed_radius", "inflation_radius", "cost_scaling_factor"), params), points=d_wall,
                    sensor_origins=poses[:, :2].contiguous())

    runs = {}
    with BatchSolver(orc.make_params()) as s:
        s.set_world_map(world, res, -10.0, -10.0)
        for how, kw in (("default", {}), ("none", dict(scan=None)), ("scan", dict(scan=scan))):
            seen, flags = [], []
            d_orig = gpu(probs["cur_xy"] - size * res / 2 + 0.013)
            s.roll_costmap_pool(size, size, res, d_orig)
            s.reset_scan_layer()
            b = DeviceBatch(probs, st, warm, "cuda:0")
            fleet_loop.closed_loop(s, b, ticks, before_tick=lambda t, pos: seen.append(pos.cpu().numpy().copy()),
                                   after_tick=lambda t, cm: flags.append(cm.copy()), footprint=RECT,
                                   rolling=(size, size, res, d_orig), **kw)
            torch.cuda.synchronize()
            runs[how] = (np.array(seen), np.array(flags))
    assert runs["default"][0].tobytes() == runs["none"][0].tobytes() and runs["default"][1].tobytes() == runs["none"][1].tobytes()
    free, stopped = runs["none"][0][:, 0, 0].max(), runs["scan"][0][:, 0, 0].max()
    print("furthest x: %.3f m without the scan, %.3f m with it (wall at %.1f)" % (free, stopped, wall_x))
    assert free > wall_x, "the control run: the robot did not reach the wall"
    assert stopped < wall_x - 0.45
    assert ((runs["scan"][1]["flags"] & abi.FLAG_STOPPED) != 0).any(axis=0).all()


# ------------------------------------------------------------------------------------------ 13: a seed exactly 64 cells away
def test_a_seed_exactly_64_cells_away_in_the_transcriptions():
    assert np.array_equal(distance_64_case()[1], distance_64_case()[6][0])    # unknown layer cells leave a free window alone


@pytest.mark.gpu
def test_a_seed_exactly_64_cells_away_on_the_gpu():
    from neo_mpc_planner2_amd.solver import BatchSolver
    world, want, params, points, sensor, layers, pool = distance_64_case()
    with BatchSolver({}) as s:
        for put in (np.array, gpu):                                       # the host and the device variants
            s.set_world_map(put(world), 0.0625, 0.0, 0.0)
            s.inflate_world_map(*params)
            assert np.array_equal(s.get_world_map()[0], want), put.__name__
            s.set_costmap_pool(world[None] * 0, 0.0625, np.zeros((1, 2)))
            s.update_scan_layer(*params, points=put(points), sensor_origins=put(sensor))
            got = window_state(s)
            assert np.array_equal(got[0], layers) and np.array_equal(got[2], pool), put.__name__
