"""The fleet's shared obstacle layer on the world map (K12): one layer on the world's lattice, fed from every robot's scan,
merged into a copy of the world map and inflated there once per update; the roll cuts the windows from the result:
world scan -> roll -> stamp -> gate -> carrots -> solve.

The contract is the text in include/neo_mpc.h (neo_mpc_fleet_clear, neo_mpc_update_world_scan_layer) and its executable form the
transcription in tests/world_scan_layer_reference.py, which composes the scan layer's transcription on the world's geometry and
adds the footprint-clearing rule.  The contract's float64 is + - * /, sqrt and comparisons, each one correctly rounded
operation on both sides, and the rest is integers: every comparison with the transcription is exact equality of uint8 cells
-- no tolerance, no dropped case.  (From ranges the transcription is fed with the points the device projected, as in
tests/test_laser_scan.py.)"""
import collections
import ctypes as C
import functools
import math

import numpy as np
import pytest

from neo_mpc_planner2_amd import abi
from tests import fleet_stamp_reference as stamp_ref
from tests import rolling_window_reference as roll_ref
from tests import scan_layer_reference as scan_ref
from tests import world_inflation_reference as world_ref
from tests import world_scan_layer_reference as ref
from tests.c_probe import check_entry_points, check_layout, probe_header
from tests.fleet_kit import (F32, RECT, Side, capture_fleet, gpu, inflation_for, pairs_fleet, rectangle, replay_against_direct,
                             rolled_pool, same, scanner, world_scan_callback, world_state)
from tests.world_scan_cases import UPDATE_FLAGS, WORLDS, case, distance_64_case, expected, ranges_for

ENTRY_POINTS = ("neo_mpc_update_world_scan_layer", "neo_mpc_update_world_scan_layer_device",
                "neo_mpc_update_world_scan_layer_from_ranges", "neo_mpc_update_world_scan_layer_from_ranges_device",
                "neo_mpc_get_world_scan_layer", "neo_mpc_reset_world_scan_layer")
REACHES = (0, 3, 12, 64)
ROBOTS = (1, 3, 7)
MAX_POINTS = (1, 64, 130)           # one lane, one full wave, two waves and a tail
#: world x R, with the robots, the point counts and the two unknown values dealt over them
CASES = [(w, reach, ROBOTS[(a + b) % 3], MAX_POINTS[(2 * a + b) % 3], (255, 0)[(a + b) % 2])
         for a, w in enumerate(sorted(WORLDS)) for b, reach in enumerate(REACHES)]


# ------------------------------------------------------------------------------------------ 1: the rule by hand
def test_padding_by_hand_adds_exactly_one_ring():
    """A 4 x 2-cell rectangle, (5, 7) .. (9, 9), on a 16 x 16 world of 1 m cells at the origin.  Its own cells: centres 5.5 ..
    8.5 by 7.5 and 8.5.  padding 0.75: every edge line moves out by 0.75, so the centres 4.5 and 9.5, 6.5 and 9.5 come in
    (0.5 <= 0.75) and 3.5, 10.5, 5.5, 10.5 stay out (1.5 > 0.75); the corners of an axis-aligned rectangle are square."""
    i, l = np.arange(16)[None, :], np.arange(16)[:, None]
    own = [(i_, l_) for l_ in (7, 8) for i_ in (5, 6, 7, 8)]
    ring = [(4, 6), (5, 6), (6, 6), (7, 6), (8, 6), (9, 6),
            (4, 7), (9, 7), (4, 8), (9, 8),
            (4, 9), (5, 9), (6, 9), (7, 9), (8, 9), (9, 9)]
    for clockwise in (False, True):
        poly = rectangle(5.0, 7.0, 9.0, 9.0, clockwise)
        got = ref.cleared(poly, 0.0, 0.0, 0.0, 1.0, i, l)
        assert sorted((int(a), int(b)) for b, a in np.argwhere(got)) == sorted(own)
        got = ref.cleared(poly, 0.75, 0.0, 0.0, 1.0, i, l)
        assert sorted((int(a), int(b)) for b, a in np.argwhere(got)) == sorted(own + ring)
        assert len(own + ring) == 24
        for (a, b), want in (((4, 6), True), ((3, 6), False), ((4, 5), False), ((9, 9), True), ((10, 9), False)):
            assert ref.cleared_cell(poly, 0.75, 0.0, 0.0, 1.0, a, b) is want


# ------------------------------------------------------------------------------------------ 2: the two forms, every branch
@functools.lru_cache(maxsize=None)
def rule_polygons():
    """On a 24 x 20 world of 0.25 m cells at (-1, 2): a rectangle, a triangle and a turned pentagon inside, one rectangle
    partly off the world, one wholly off it, one with a vertex that is not finite; each in both windings."""
    rng = np.random.default_rng(12)
    angle = np.sort(rng.uniform(0, 2 * np.pi, size=5))
    polys = [rectangle(0.1, 2.9, 1.3, 3.6), np.array([(1.0, 4.0), (3.2, 4.4), (1.7, 6.1)]),
             np.stack([2.6 + 0.9 * np.cos(angle), 4.2 + 0.7 * np.sin(angle)], 1),
             rectangle(-1.6, 1.4, -0.2, 2.7), rectangle(9.0, 9.0, 10.0, 10.0),
             np.array([(0.0, 3.0), (np.nan, 3.0), (1.0, 4.0)])]
    return polys + [p[::-1].copy() for p in polys]


def test_the_two_forms_of_the_clearing_rule_agree_and_take_every_branch():
    wox, woy, wres, sx, sy = -1.0, 2.0, 0.25, 24, 20
    i, l = np.arange(sx)[None, :], np.arange(sy)[:, None]
    stats = collections.Counter()
    for padding in (0.0, 0.2, 0.6):
        a, b = np.full((sy, sx), 255, dtype=np.uint8), np.full((sy, sx), 255, dtype=np.uint8)
        ref.clear_footprints(a, wox, woy, wres, rule_polygons(), padding)
        ref.clear_footprints_by_definition(b, wox, woy, wres, rule_polygons(), padding, stats)
        assert np.array_equal(a, b) and (a == 0).any() and (a == 255).any(), padding
    print(dict(stats))
    for name in ("clear: a vertex is not finite", "clear: a polygon reaches beyond the world",
                 "clear: every c_e >= -padding L_e", "clear: not every c_e >= -padding L_e",
                 "clear: every c_e <= padding L_e", "clear: not every c_e <= padding L_e", "clear: both arms"):
        assert stats[name] > 0, name
    # padding 0 is the fleet stamp's rule on every cell, for both windings
    for poly in rule_polygons():
        assert np.array_equal(ref.cleared(poly, 0.0, wox, woy, wres, i, l), stamp_ref.stamped(poly, wox, woy, wres, i, l))
    # the polygon that is partly off the world clears what is on it; the one wholly off it nothing
    assert ref.cleared(rule_polygons()[3], 0.0, wox, woy, wres, i, l).any()
    assert not ref.cleared(rule_polygons()[4], 0.6, wox, woy, wres, i, l).any()


# ------------------------------------------------------------------------------------------ 3: record and entry points
def test_fleet_clear_layout_and_entry_points(tmp_path):
    got = probe_header(tmp_path, ["neo_mpc_fleet_clear"], entry_points=ENTRY_POINTS)
    check_layout(got, "neo_mpc_fleet_clear", 64, struct=abi.NeoMpcFleetClear, dtype=abi.FLEET_CLEAR_DTYPE)
    assert len(ENTRY_POINTS) == 6
    check_entry_points(ENTRY_POINTS)


# ------------------------------------------------------------------------------------------ the generator has teeth
def test_the_array_transcription_equals_the_definition_on_a_case():
    case_ = ("40x40-10cm", 3, 3, 64, 255)
    for a, b in zip(expected(*case_)[0], expected(*case_, by_definition=True)[0]):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    stats = expected(*case_, by_definition=True)[1]
    for name in ("reset", "ray walked", "marked", "sensor origin off the map", "clear: every c_e >= -padding L_e",
                 "clear: a polygon reaches beyond the world", "combine: v == 255", "combine: old < v"):
        assert stats[name] > 0, name
    layers = [x[0] for x in expected(*case_)[0]]
    assert (layers[0] == 254).any() and np.array_equal(layers[0], layers[1])          # flags 0 keeps the layer
    assert (layers[2] == 254).sum() < (layers[0] == 254).sum()                        # rays alone erase marks


# ------------------------------------------------------------------------------------------ 4: equality with the transcription
@pytest.mark.gpu
@pytest.mark.parametrize("world,reach,robots,max_points,unknown", CASES,
                         ids=["%s-R%d-%drobots-%dpoints-unknown%d" % c for c in CASES])
def test_updates_equal_the_transcription(world, reach, robots, max_points, unknown):
    from neo_mpc_planner2_amd.solver import BatchSolver
    sx, sy, res = WORLDS[world]
    cells, wox, woy, updates, polygons = case(world, robots, max_points)
    want, _ = expected(world, reach, robots, max_points, unknown)
    params, ranges = inflation_for(reach, res), ranges_for(world)
    assert BatchSolver.inflation_costs(res, *params)[1] == reach
    with BatchSolver({}) as s:
        for put in (gpu, np.array):                                       # the device and the host variants
            s.set_world_map(put(cells), res, wox, woy)
            s.reset_world_scan_layer()
            for k, ((points, counts, sensors), flags) in enumerate(zip(updates, UPDATE_FLAGS)):
                kw = dict(flags=flags, clear=dict(polygons=put(polygons), padding=1.5 * res), unknown_value=unknown, **ranges)
                if points is not None:
                    kw.update(points=put(points), sensor_origins=put(sensors),
                              point_counts=gpu(counts, np.int32) if put is gpu else counts)
                elif put is gpu:
                    kw.update(on_device=True)
                s.update_world_scan_layer(*params, **kw)
                got = world_state(s)
                assert np.array_equal(got[0], want[k][0]), (put.__name__, k, int((got[0] != want[k][0]).sum()))
                assert np.array_equal(got[1], want[k][1]), (put.__name__, k, int((got[1] != want[k][1]).sum()))
                s.update_world_scan_layer(*params, **kw)                  # repeated with the same inputs: nothing changes
                assert same(world_state(s), got), (put.__name__, k)
            assert np.array_equal(s.get_world_map()[0], cells)            # the static map is what it was
        print("%s R=%d %d robots %d points: %d marks, %d free layer cells, %d world cells changed" %
              (world, reach, robots, max_points, int((want[0][0] == 254).sum()), int((want[0][0] == 0).sum()),
               int((want[0][1] != cells).sum())))


@pytest.mark.gpu
def test_a_seed_exactly_64_cells_away_on_this_path():
    """The 193 x 66 case of tests/test_scan_layer.py (world_scan_cases.distance_64_case): seeds at (64, 1) and (64, 65), R = 64,
    a world width of 193."""
    from neo_mpc_planner2_amd.solver import BatchSolver
    world, want, params, points, sensor, layers, pool = distance_64_case()
    model = ref.WorldScanLayer()
    live = model.update(world * 0, 0.0625, 0.0, 0.0, *params, points=points, sensor_origins=sensor)
    assert np.array_equal(model.layer, layers[0]) and np.array_equal(live, pool[0]) and np.array_equal(live, want)
    with BatchSolver({}) as s:
        for put in (np.array, gpu):
            s.set_world_map(put(world * 0), 0.0625, 0.0, 0.0)
            s.reset_world_scan_layer()
            s.update_world_scan_layer(*params, points=put(points), sensor_origins=put(sensor))
            got = world_state(s)
            assert np.array_equal(got[0], model.layer) and np.array_equal(got[1], live), put.__name__


# ------------------------------------------------------------------------------------------ 5: order across robots
TWO_KW = dict(obstacle_max_range=20.0, obstacle_min_range=0.0, raytrace_max_range=20.0, raytrace_min_range=0.0)
TWO_INFLATION = (0.0, 0.0, 1.0)                                 # R = 0: the layer's cells and nothing around them
#: the two beams of docs/NOTEBOOK.md A.19 as two robots: A at (16.5, 16.5) hits (20, 16), B at (12.5, 16.5) looks through it
#: into (24, 16); a 32 x 32 world of 1 m cells
TWO_SENSORS = np.array([(16.5, 16.5), (12.5, 16.5)])
TWO_POINTS = np.array([[(20.5, 16.5)], [(24.5, 16.5)]])


@pytest.mark.gpu
def test_a_mark_of_one_robot_survives_the_ray_of_another_in_the_same_update():
    from neo_mpc_planner2_amd.solver import BatchSolver
    world = np.zeros((32, 32), dtype=np.uint8)
    with BatchSolver({}) as s:
        for put in (gpu, np.array):
            s.set_world_map(put(world), 1.0, 0.0, 0.0)
            s.reset_world_scan_layer()
            s.update_world_scan_layer(*TWO_INFLATION, points=put(TWO_POINTS), sensor_origins=put(TWO_SENSORS), **TWO_KW)
            layer, live = world_state(s)
            row = layer[16]
            assert row[20] == 254 and row[24] == 254                              # both marks stand
            assert (row[21:24] == 0).all() and (row[12:20] == 0).all()            # B's ray: free between the marks and before them
            assert (np.delete(layer, 16, axis=0) == 255).all() and (row[:12] == 255).all() and (row[25:] == 255).all()
            assert live[16, 20] == 254 and live[16, 24] == 254 and (live == 254).sum() == 2
            # robot B's scan alone, one robot: its ray frees A's cell
            s.update_world_scan_layer(*TWO_INFLATION, points=put(TWO_POINTS[1:]), sensor_origins=put(TWO_SENSORS[1:]), **TWO_KW)
            layer, live = world_state(s)
            assert layer[16, 20] == 0 and layer[16, 24] == 254 and live[16, 20] == 0 and (live == 254).sum() == 1


# ------------------------------------------------------------------------------------------ 6: the capability
@pytest.mark.gpu
def test_what_robot_0_sees_reaches_robot_1s_window():
    """Two robots 1.5 m apart on a free world; a pallet between them exists only in robot 0's points.  World scan -> roll:
    robot 1's window shows the pallet and its ring and is the rolling-window transcription applied to the transcription's
    `live`.  The same inputs through the per-window layers (K10) leave robot 1's window without it."""
    from neo_mpc_planner2_amd.solver import BatchSolver
    res, size = 0.05, 60
    world = np.zeros((200, 200), dtype=np.uint8)
    params = (0.1, 0.3, 3.0)
    poses = np.array([(0.012, 0.017, 0.0), (1.512, 0.017, 0.0)])
    pallet = np.array([(0.7 + 0.05 * (j % 3), -0.1 + 0.05 * (j // 3)) for j in range(12)])
    points = np.stack([pallet, np.full((12, 2), np.nan)])
    start = poses[:, :2] - size * res / 2 + 0.013
    model = ref.WorldScanLayer()
    live = model.update(world, res, -5.0, -5.0, *params, points=points, sensor_origins=poses[:, :2])
    want_origins, want = roll_ref.roll(live, res, -5.0, -5.0, start, size, size, res, poses=poses, outside_value=255)
    assert (want[1] == 254).any() and ((want[1] > 0) & (want[1] < 254)).any()
    with BatchSolver({}) as s:
        s.set_world_map(gpu(world), res, -5.0, -5.0)
        s.update_world_scan_layer(*params, points=gpu(points), sensor_origins=gpu(poses[:, :2]))
        assert same(world_state(s), (model.layer, live))
        pool, origins = rolled_pool(s, size, size, res, start.copy(), poses)
        assert origins.tolist() == want_origins.tolist() and np.array_equal(pool, want)
    with BatchSolver({}) as s:                                            # a handle that never saw a world-scan update
        s.set_world_map(gpu(world), res, -5.0, -5.0)
        pool, origins = rolled_pool(s, size, size, res, start.copy(), poses)
        s.update_scan_layer(*params, points=points, sensor_origins=poses[:, :2])
        pool = s.get_costmap_pool()[0]
        assert (pool[0] == 254).any() and not pool[1].any()


# ------------------------------------------------------------------------------------------ 7: footprint clearing
@pytest.mark.gpu
def test_fleet_footprint_clearing_frees_the_hulls_and_nothing_beyond_the_padding():
    """Robot 0's scanner hits robot 1's rear edge -- a point ON the outline -- and something 1.5 cells plus the padding behind
    it.  Without the record robot 1's own gate reads 254 in its window; with it the hull's mark is gone from layer and live,
    the other mark stays, and the gate reads less.  A third robot whose pose is not finite clears nothing (device variant)."""
    from neo_mpc_planner2_amd.solver import BatchSolver
    res, size = 0.05, 60
    padding = math.sqrt(2.0) * res
    world = np.zeros((160, 160), dtype=np.uint8)
    params = (0.0, 0.05, 3.0)                                           # R = 1: a ring of one cell
    poses = np.array([(-1.2 + 0.012, 0.017, 0.0), (0.012, 0.017, 0.0), (np.nan, 0.5, 0.0)])
    rear = poses[1, 0] - 0.35
    hits = np.array([(rear, 0.017), (rear - padding - 1.5 * res, 0.017)])
    points = np.stack([hits, np.full((2, 2), np.nan), np.full((2, 2), np.nan)])
    sensors = np.array([poses[0, :2], poses[1, :2], poses[1, :2]])
    hull = scan_ref.world_to_map(*hits[0], -4.0, -4.0, res, 160, 160)
    other = scan_ref.world_to_map(*hits[1], -4.0, -4.0, res, 160, 160)
    start = np.round((poses[:2, :2] - size * res / 2) / res) * res      # the windows on the world's lattice: cell for cell
    fp = np.asarray(RECT, dtype=np.float64)
    with BatchSolver({}) as s:
        s.set_world_map(gpu(world), res, -4.0, -4.0)
        seen = {}
        for how in ("without", "footprint", "polygons", "host"):
            s.reset_world_scan_layer()
            if how == "without":
                s.update_world_scan_layer(*params, points=gpu(points), sensor_origins=gpu(sensors))
            elif how == "footprint":
                s.update_world_scan_layer(*params, points=gpu(points), sensor_origins=gpu(sensors),
                                          clear=dict(footprint=gpu(fp), poses=gpu(poses), padding=padding))
            elif how == "polygons":
                s.update_world_scan_layer(*params, points=gpu(points), sensor_origins=gpu(sensors),
                                          clear=dict(polygons=gpu(polygons), padding=padding))
            else:
                s.update_world_scan_layer(*params, points=points[:2], sensor_origins=sensors[:2],
                                          clear=dict(footprint=fp, poses=poses[:2], padding=padding))
            layer, live = world_state(s)
            pool, origins = rolled_pool(s, size, size, res, start.copy(), poses[:2])
            costs, polys = s.footprint_gate(fp, poses=poses[:2], map_indices=np.arange(2, dtype=np.int32), want_polygons=True)
            seen[how] = (layer, live, costs)
            if how == "without":
                polygons = np.concatenate([polys, np.full((1, 4, 2), np.nan)])       # what the device places the outlines at
                model = ref.WorldScanLayer()
                model.update(world, res, -4.0, -4.0, *params, points=points, sensor_origins=sensors)
                assert same((layer, live), (model.layer, model.live))
            else:
                model = ref.WorldScanLayer()
                model.update(world, res, -4.0, -4.0, *params, points=points, sensor_origins=sensors,
                             clear=dict(polygons=polygons, padding=padding))
                assert same((layer, live), (model.layer, model.live)), how
        layer, live, costs = seen["without"]
        assert layer[hull[1], hull[0]] == 254 and layer[other[1], other[0]] == 254 and costs[1] >= 254.0
        for how in ("footprint", "polygons", "host"):
            layer, live, costs = seen[how]
            assert layer[hull[1], hull[0]] == 0 and live[hull[1], hull[0]] == 0, how
            assert layer[other[1], other[0]] == 254 and live[other[1], other[0]] == 254, how
            assert costs[1] < 254.0 and (layer == 254).sum() == 1, how
        print("robot 1's gate: %.0f without the record, %.0f with it" % (seen["without"][2][1], seen["footprint"][2][1]))


# ------------------------------------------------------------------------------------------ 8: validity
@pytest.mark.gpu
def test_live_is_valid_from_an_update_to_the_next_change_of_the_world_map():
    from neo_mpc_planner2_amd.solver import BatchSolver
    world_name, reach = "96x70-5cm", 3
    wsx, wsy, res = WORLDS[world_name]
    cells, wox, woy, updates, _ = case(world_name, 3, 64)
    points, counts, sensors = updates[0]
    params, ranges = inflation_for(reach, res), ranges_for(world_name)
    size = 40
    poses = np.concatenate([sensors, np.zeros((3, 1))], 1)
    start = sensors - size * res / 2 + 0.013
    other = np.where(cells == 60, 254, np.where(cells == 150, 0, cells)).astype(np.uint8)   # other walls: seeds for K9 too

    def roll_of(source):
        return roll_ref.roll(source, res, wox, woy, start, size, size, res, poses=poses, outside_value=255)[1]

    with BatchSolver({}) as s:
        model = ref.WorldScanLayer()

        def rolled():
            return rolled_pool(s, size, size, res, start.copy(), poses)[0]

        s.set_world_map(cells, res, wox, woy)
        assert s._lib.neo_mpc_get_world_scan_layer(s._handle, None, None) == -4          # before the first update
        assert np.array_equal(rolled(), roll_of(cells))
        s.update_world_scan_layer(*params, points=points, sensor_origins=sensors, point_counts=counts, **ranges)
        live = model.update(cells, res, wox, woy, *params, points=points, sensor_origins=sensors, point_counts=counts, **ranges)
        assert not np.array_equal(live, cells) and np.array_equal(rolled(), roll_of(live))
        # the world map set again, same geometry: the roll reads the static map; the next flags-0 update puts the kept layer back
        s.set_world_map(other, res, wox, woy)
        assert np.array_equal(rolled(), roll_of(other))
        s.update_world_scan_layer(*params, **ranges)
        kept = model.layer.copy()
        live = model.update(other, res, wox, woy, *params, **ranges)
        assert np.array_equal(model.layer, kept) and same(world_state(s), (kept, live)) and np.array_equal(rolled(), roll_of(live))
        # an inflation of the world map: the same
        s.inflate_world_map(*params)
        inflated = world_ref.inflate_world(other, res, *params)
        assert np.array_equal(rolled(), roll_of(inflated))
        s.update_world_scan_layer(*params, **ranges)
        live = model.update(inflated, res, wox, woy, *params, **ranges)
        assert same(world_state(s), (kept, live)) and np.array_equal(rolled(), roll_of(live))
        # another origin: the layer is reset
        s.set_world_map(other, res, wox + res, woy)
        s.update_world_scan_layer(*params, **ranges)
        layer, live = world_state(s)
        assert (layer == 255).all() and np.array_equal(live, other)
        # ... and by the reset call, behind which there is no layer and the roll reads the static map
        s.update_world_scan_layer(*params, points=points, sensor_origins=sensors, point_counts=counts, **ranges)
        assert (world_state(s)[0] != 255).any()
        s.reset_world_scan_layer()
        assert s._lib.neo_mpc_get_world_scan_layer(s._handle, None, None) == -4
        assert np.array_equal(rolled(), roll_ref.roll(other, res, wox + res, woy, start, size, size, res, poses=poses)[1])
        s.update_world_scan_layer(*params, **ranges)
        assert (world_state(s)[0] == 255).all()
        # another unknown_value resets it too
        s.update_world_scan_layer(*params, points=points, sensor_origins=sensors, point_counts=counts, **ranges)
        s.update_world_scan_layer(*params, unknown_value=0, **ranges)
        assert (world_state(s)[0] == 0).all()


# ------------------------------------------------------------------------------------------ 9: refusals
@pytest.mark.gpu
def test_refusals_leave_layer_live_pool_and_validity_alone():
    from neo_mpc_planner2_amd.solver import BatchSolver
    world_name, robots, max_points = "40x40-10cm", 3, 64
    wsx, wsy, res = WORLDS[world_name]
    cells, wox, woy, updates, polygons = case(world_name, robots, max_points)
    points, counts, sensors = (a.copy() for a in updates[0])
    polygons = polygons.copy()
    params, ranges = inflation_for(3, res), ranges_for(world_name)
    bad_counts, bad_sensors, bad_polygons = counts.copy(), sensors.copy(), polygons.copy()
    bad_counts[2] = max_points + 1
    bad_sensors[2, 1] = np.inf
    bad_polygons[1, 2, 0] = np.nan
    fp = np.asarray(RECT, dtype=np.float64)
    poses = np.concatenate([sensors, np.zeros((robots, 1))], 1)
    bad_poses = poses.copy()
    bad_poses[0, 2] = np.nan
    size = 24
    start = sensors - size * res / 2 + 0.013
    scanners = abi.scanner_array(dict(mount_x=0.1, mount_y=0.0, mount_yaw=0.0, angle_min=-1.0, angle_increment=0.1,
                                      range_min=0.05, range_max=5.0))
    laser_ranges = np.full((robots, 1, 21), 1.0, dtype=F32)
    with BatchSolver({}) as s:
        lib, h = s._lib, s._handle

        def clear_record(**over):
            c = abi.NeoMpcFleetClear()
            c.count, c.polygons, c.footprint_points, c.padding = robots, polygons.ctypes.data, 4, 0.1
            for k, v in over.items():
                setattr(c, k, v)
            return c

        def call(device=False, clear=None, **over):
            b = abi.NeoMpcScanBatch()
            b.count, b.points, b.point_counts, b.sensor_origins = robots, points.ctypes.data, counts.ctypes.data, sensors.ctypes.data
            b.max_points, b.flags, b.unknown_value = max_points, 3, 255
            b.inscribed_radius, b.inflation_radius, b.cost_scaling_factor = params
            for k, v in ranges.items():
                setattr(b, k, v)
            for k, v in over.items():
                setattr(b, k, v)
            cp = C.byref(clear) if clear is not None else None
            if device:
                return lib.neo_mpc_update_world_scan_layer_device(h, C.byref(b), cp, None)
            return lib.neo_mpc_update_world_scan_layer(h, C.byref(b), cp)

        def laser_call(device=False, clear=None, **over):
            b = abi.NeoMpcLaserBatch()
            b.count, b.ranges, b.poses, b.scanners = robots, laser_ranges.ctypes.data, poses.ctypes.data, scanners.ctypes.data
            b.sources, b.beams, b.scan_flags, b.unknown_value = 1, 21, 3, 255
            b.inscribed_radius, b.inflation_radius, b.cost_scaling_factor = params
            for k, v in ranges.items():
                setattr(b, k, v)
            for k, v in over.items():
                setattr(b, k, v)
            cp = C.byref(clear) if clear is not None else None
            if device:
                return lib.neo_mpc_update_world_scan_layer_from_ranges_device(h, C.byref(b), cp, None)
            return lib.neo_mpc_update_world_scan_layer_from_ranges(h, C.byref(b), cp)

        assert call() == -4 and call(device=True) == -4 and laser_call() == -4 and laser_call(device=True) == -4   # no world map
        s.set_world_map(cells, res, wox, woy)
        assert lib.neo_mpc_get_world_scan_layer(h, None, None) == -4        # ... and no layer yet
        assert call(clear=clear_record()) == 0                              # the state the refusals must leave alone
        rolled_pool(s, size, size, res, start.copy(), poses)

        def state():
            return world_state(s) + (s.get_costmap_pool()[0],)

        held = state()
        assert (held[0] == 254).any() and (held[0] == 0).any() and not np.array_equal(held[1], cells)
        shape_errors = [dict(reserved=1), dict(flags=4), dict(flags=7), dict(unknown_value=1), dict(unknown_value=254),
                        dict(max_points=8193), dict(points=None), dict(sensor_origins=None), dict(count=65536)]
        for name in ("obstacle_max_range", "obstacle_min_range", "raytrace_max_range", "raytrace_min_range",
                     "inscribed_radius", "inflation_radius", "cost_scaling_factor"):
            shape_errors += [{name: -0.1}, {name: float("nan")}, {name: float("inf")}]
        clear_errors = [dict(reserved=1), dict(footprint_points=2), dict(footprint_points=17), dict(per_robot_footprints=2),
                        dict(padding=-0.01), dict(padding=float("nan")), dict(padding=float("inf")), dict(count=robots - 1),
                        dict(polygons=None), dict(polygons=None, footprint=fp.ctypes.data)]
        value_errors = [dict(point_counts=bad_counts.ctypes.data), dict(sensor_origins=bad_sensors.ctypes.data)]
        clear_values = [dict(polygons=bad_polygons.ctypes.data),
                        dict(polygons=None, footprint=fp.ctypes.data, poses=bad_poses.ctypes.data)]
        for device in (False, True):
            for over in shape_errors + ([] if device else value_errors):    # the host variant looks at the values too
                assert call(device, **over) == -1, (device, over)
                assert lib.neo_mpc_last_error_code() == -1 and same(state(), held), (device, over)
            for over in clear_errors + ([] if device else clear_values):
                assert call(device, clear=clear_record(**over)) == -1, (device, over)
                assert same(state(), held), (device, over)
            assert call(device, inflation_radius=6.6) == -5                 # 66 cells at 10 cm
            assert call(device, count=0) == 0 and same(state(), held)       # nothing to do
            # from ranges: K11's refusals, the world's, the clear record's
            for over in (dict(reserved=1), dict(sources=0), dict(sources=5), dict(beams=0), dict(scanners=None), dict(ranges=None),
                         dict(poses=None), dict(scan_flags=0), dict(scan_flags=4), dict(unknown_value=7),
                         dict(raytrace_max_range=-1.0), dict(inflation_radius=float("nan")), dict(count=65536)):
                assert laser_call(device, **over) == -1, (device, over)
            assert laser_call(device, clear=clear_record(padding=-1.0)) == -1 and laser_call(device, inflation_radius=6.6) == -5
            assert same(state(), held), device
        assert laser_call(poses=bad_poses.ctypes.data) == -1 and same(state(), held)
        assert lib.neo_mpc_update_world_scan_layer(h, None, None) == -1 and lib.neo_mpc_update_world_scan_layer_device(h, None, None, None) == -1
        assert lib.neo_mpc_update_world_scan_layer(None, C.byref(abi.NeoMpcScanBatch()), None) == -1
        assert lib.neo_mpc_update_world_scan_layer_from_ranges(h, None, None) == -1
        assert lib.neo_mpc_reset_world_scan_layer(None) == -1 and lib.neo_mpc_get_world_scan_layer(None, None, None) == -1
        # live is still valid: a roll cuts its windows from it
        pool = rolled_pool(s, size, size, res, start.copy(), poses)[0]
        assert np.array_equal(pool, roll_ref.roll(held[1], res, wox, woy, start, size, size, res, poses=poses)[1])
        assert call(flags=0, points=None, sensor_origins=None, point_counts=None, clear=clear_record()) == 0   # flags 0 needs no points
        assert same(world_state(s), held[:2])                                  # ... and is the idempotent repeat here


# ------------------------------------------------------------------------------------------ 10: from ranges
LASER_SCANNERS = [scanner((0.3, 0.1, 0.2), -1.6, 3.2 / 89, 0.05, 6.0, abi.LASER_INF_IS_VALID), scanner((-0.3, -0.05, 3.0), -1.6, 3.2 / 89, 0.05, 6.0)]
LASER_KW = dict(obstacle_max_range=2.0, obstacle_min_range=0.15, raytrace_max_range=2.4, raytrace_min_range=0.1)


@pytest.mark.gpu
def test_update_from_ranges_equals_projection_then_the_transcription():
    """Two scanners, three robots, two ticks: the transcription is fed with the points and origins the device projected
    (project_laser, read back), so layer and live are compared bit for bit wherever the points fall."""
    import torch
    from neo_mpc_planner2_amd.solver import BatchSolver
    world_name, reach = "96x70-5cm", 12
    wsx, wsy, res = WORLDS[world_name]
    cells, wox, woy, updates, _ = case(world_name, 3, 64)
    params = inflation_for(reach, res)
    rng = np.random.default_rng(1201)
    model = ref.WorldScanLayer()
    fp = np.asarray(RECT, dtype=np.float64) * 0.5
    with BatchSolver({}) as s:
        s.set_world_map(gpu(cells), res, wox, woy)
        s.set_costmap_pool(np.zeros((3, 8, 8), dtype=np.uint8), res, np.zeros((3, 2)))    # (a pool for the gate's polygons)
        for k in range(2):
            poses = np.concatenate([updates[0][2] + rng.uniform(-0.2, 0.2, size=(3, 2)), rng.uniform(-3.0, 3.0, size=(3, 1))], 1)
            ranges = rng.uniform(0.0, 3.5, size=(3, 2, 90)).astype(F32)
            ranges[:, :, 3:45:7] = np.array([np.nan, np.inf, -np.inf, 0.05, 6.0, 0.04], dtype=F32)
            d_poses, d_ranges = gpu(poses), gpu(ranges)
            points, sensors = s.project_laser(d_ranges, d_poses, LASER_SCANNERS)
            torch.cuda.synchronize()
            points, sensors = points.cpu().numpy(), sensors.cpu().numpy()
            polygons = s.footprint_gate(fp, poses=poses, map_indices=np.arange(3, dtype=np.int32), want_polygons=True)[1]
            clear = dict(polygons=polygons, padding=0.08)
            live = model.update(cells, res, wox, woy, *params, points=points, sensor_origins=sensors, clear=clear, **LASER_KW)
            s.update_world_scan_layer_from_ranges(*params, d_ranges, d_poses, LASER_SCANNERS,
                                                  clear=dict(footprint=gpu(fp), poses=d_poses, padding=0.08), **LASER_KW)
            got = world_state(s)
            print("tick %d: %d marks, %d free layer cells" % (k, int((model.layer == 254).sum()), int((model.layer == 0).sum())))
            assert (model.layer == 254).any() and (model.layer == 0).any()
            assert np.array_equal(got[0], model.layer), (k, int((got[0] != model.layer).sum()))
            assert np.array_equal(got[1], live), (k, int((got[1] != live).sum()))
        # the host variant, from scratch with the last tick's inputs on top of a reset: the projection handed out, the same bytes
        before = ref.WorldScanLayer()
        want = before.update(cells, res, wox, woy, *params, points=points, sensor_origins=sensors, clear=clear, **LASER_KW)
        s.reset_world_scan_layer()
        out_p, out_o = np.zeros((3, 2, 90, 2)), np.zeros((3, 2, 2))
        s.update_world_scan_layer_from_ranges(*params, ranges, poses, LASER_SCANNERS, points_out=out_p, origins_out=out_o,
                                              clear=dict(footprint=fp, poses=poses, padding=0.08), **LASER_KW)
        assert out_p.tobytes() == points.tobytes() and out_o.tobytes() == sensors.tobytes()
        assert same(world_state(s), (before.layer, want))


# ------------------------------------------------------------------------------------------ 11: both kinds of layer in one tick
@pytest.mark.gpu
def test_world_layer_and_window_layers_in_one_tick_compose():
    from neo_mpc_planner2_amd.solver import BatchSolver
    world_name, reach = "96x70-5cm", 3
    wsx, wsy, res = WORLDS[world_name]
    cells, wox, woy, updates, _ = case(world_name, 3, 64)
    points, counts, sensors = updates[0]
    beyond = updates[2][0]
    params, ranges = inflation_for(reach, res), ranges_for(world_name)
    size = 40
    poses = np.concatenate([sensors, np.zeros((3, 1))], 1)
    start = sensors - size * res / 2 + 0.013
    world_model, window_model = ref.WorldScanLayer(), scan_ref.ScanLayers()
    live = world_model.update(cells, res, wox, woy, *params, points=points, sensor_origins=sensors, point_counts=counts, **ranges)
    origins, rolled = roll_ref.roll(live, res, wox, woy, start, size, size, res, poses=poses, outside_value=255)
    want = window_model.update(rolled, origins, res, *params, points=beyond, sensor_origins=sensors, **ranges)
    with BatchSolver({}) as s:
        s.set_world_map(gpu(cells), res, wox, woy)
        s.update_world_scan_layer(*params, points=gpu(points), sensor_origins=gpu(sensors), point_counts=gpu(counts, np.int32), **ranges)
        s.roll_costmap_pool(size, size, res, gpu(start), poses=gpu(poses))
        s.update_scan_layer(*params, points=gpu(beyond), sensor_origins=gpu(sensors), **ranges)
        import torch
        torch.cuda.synchronize()
        assert np.array_equal(s.get_costmap_pool()[0], want)
        assert np.array_equal(s.get_scan_layer()[0], window_model.layers) and same(world_state(s), (world_model.layer, live))


# ------------------------------------------------------------------------------------------ 12: graph capture
@pytest.mark.gpu
def test_world_scan_roll_stamp_gate_solve_can_be_captured_in_a_hip_graph():
    """After one eager call -- it builds the tables and allocates -- world scan from ranges -> roll -> stamp -> gate -> solve
    is captured on one stream, a linear chain, and replayed twice with ranges and poses rewritten in between; layer, live,
    pool, gate costs and commands equal the same calls made directly on a second handle."""
    beams = 40
    stamp, scan = (0.45, 0.9, 3.0), (0.1, 0.3, 3.0)
    scanners = [scanner((0.3, 0.0, 0.0), -1.5, 3.0 / 39, 0.05, 5.0, abi.LASER_INF_IS_VALID), scanner((-0.3, 0.0, math.pi), -1.5, 3.0 / 39, 0.05, 5.0)]
    f = capture_fleet(120)
    count = f.count
    rng = np.random.default_rng(95)
    ticks = []
    for k in range(3):
        poses = np.concatenate([f.probs["cur_xy"] + rng.uniform(-0.4, 0.4, size=(count, 2)) * k, rng.uniform(-3, 3, size=(count, 1))], 1)
        ranges = rng.uniform(0.0, 1.8, size=(count, 2, beams)).astype(F32)
        ranges[:, :, 3:39:7] = np.array([np.nan, np.inf, -np.inf, 0.05, 5.0, 0.04], dtype=F32)
        ticks.append((poses, ranges))
    fp = gpu(np.asarray(RECT, dtype=np.float64))

    class WorldScanSide(Side):
        def __init__(self, fleet, tick):
            super().__init__(fleet, tick)
            self.ranges = gpu(tick[1])

        def set_inputs(self, tick):
            super().set_inputs(tick)
            self.ranges.copy_(gpu(tick[1]))

        def tick(self):
            self.s.update_world_scan_layer_from_ranges(*scan, self.ranges, self.poses, scanners, obstacle_max_range=1.5,
                                                       raytrace_max_range=1.2, raytrace_min_range=0.1,
                                                       clear=dict(footprint=fp, poses=self.poses, padding=0.1))
            self.s.roll_costmap_pool(f.sx, f.sy, f.res, self.origins, poses=self.poses)
            self.s.stamp_fleet(*stamp, footprint=fp, poses=self.poses)
            self.s.footprint_gate_device(fp, self.costs, poses=self.poses, problems=self.b.problems)
            self.s.solve_device(self.b.problems, self.b.states, self.b.warm, self.b.commands, solution=self.b.solution)

        def result(self):
            common = super().result()
            layer, live = self.s.get_world_scan_layer()
            return common + (self.s.get_costmap_pool()[0].tobytes(), layer.tobytes(), live.tobytes())

    # pool, layer and live changed
    with replay_against_direct(lambda: WorldScanSide(f, ticks[0]), ticks, changed=(4, 5, 6)) as (_, a, _):
        layer = np.frombuffer(a[5], dtype=np.uint8)
        live = np.frombuffer(a[6], dtype=np.uint8)
        assert (layer == 254).any() and (layer == 0).any() and live.tobytes() != f.world.tobytes()


# ------------------------------------------------------------------------------------------ 13: the closed loop
@pytest.mark.gpu
def test_closed_loop_a_wall_seen_by_half_the_fleet_stops_the_other_half():
    """64 robots in 32 pairs on a free world map: the even robot of a pair stands 1.5 m behind the odd one and its front
    scanner's ranges hold a wall 0.3 m in front of the ODD robot's centre -- inside that robot's 0.35 m outline; the odd
    robots' own ranges hold nothing.  With `world_scan` the odd robots' gates find the wall in their windows and the
    collision latch stops them; without it nobody sees anything; world_scan=None is the loop as it was, bit for bit."""
    import torch
    from neo_mpc_planner2_amd import fleet as fleet_loop
    from neo_mpc_planner2_amd.solver import BatchSolver, DeviceBatch
    from oracle import mpc_oracle as orc
    ticks = 4
    world = np.zeros((400, 400), dtype=np.uint8)
    p = pairs_fleet()
    count, size, res, probs, st, warm = p.count, p.size, p.res, p.probs, p.st, p.warm
    ranges = np.full((count, 1, p.beams), np.inf, dtype=F32)             # (no INF_IS_VALID: nothing, not even a clearing ray)
    ranges[0::2, 0] = (1.7 / np.cos(p.angle)).astype(F32)                # x = 0.1 + 1.7 in the even robot's base frame
    world_scan = world_scan_callback((0.1, 0.3, 3.0), gpu(ranges), p.front)

    runs = {}
    with BatchSolver(orc.make_params()) as s:
        s.set_world_map(world, res, -10.0, -10.0)
        for how, kw in (("default", {}), ("none", dict(world_scan=None)), ("world_scan", dict(world_scan=world_scan))):
            flags = []
            d_orig = gpu(p.origins)
            s.reset_world_scan_layer()
            s.roll_costmap_pool(size, size, res, d_orig)
            b = DeviceBatch(probs, st, warm, "cuda:0")
            fleet_loop.closed_loop(s, b, ticks, after_tick=lambda t, cm: flags.append(cm.copy()), footprint=RECT,
                                   rolling=(size, size, res, d_orig), **kw)
            torch.cuda.synchronize()
            runs[how] = np.array(flags)
    assert runs["default"].tobytes() == runs["none"].tobytes()
    stopped = {how: ((f["flags"] & abi.FLAG_STOPPED) != 0)[-1] for how, f in runs.items()}
    print("stopped fraction of the odd half: %.3f without, %.3f with; of the even half: %.3f, %.3f" %
          (stopped["none"][1::2].mean(), stopped["world_scan"][1::2].mean(), stopped["none"][0::2].mean(),
           stopped["world_scan"][0::2].mean()))
    assert stopped["world_scan"][1::2].mean() > stopped["none"][1::2].mean()
