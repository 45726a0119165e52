"""The plan check (K15): which of a fleet's global plans the live world map blocks.

nav2 cannot be built here, so the contract is the text in include/neo_mpc.h (neo_mpc_plan_check_batch) and its executable
form the plain-Python transcription in tests/plan_check_reference.py.  Every output is an integer: every comparison is an
exact equality of the result records.  CPU tests pin the transcription to records written out by hand and the record layout
to the header; GPU tests compare the kernel with the hand-written records, with the transcription, with K6 and with itself
(host against device variant, graph replay against direct calls).

In footprint mode a vertex that sits on a cell boundary to within rounding may land in either cell (device and libm sin /
cos differ in the last bits), so the random fleet asserts that no oriented vertex of any pose lies within 1e-6 cells of a
cell edge -- tests/test_footprint_gate.py's condition on the inputs (fixed seeds), not a tolerance; no robot is dropped.
Point mode needs no such condition: the plan poses are kept clear of the edges by construction."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from neo_mpc_planner2_amd import _lib, abi, synthetic
from tests import footprint_gate_reference as fref
from tests import plan_check_reference as ref
from tests import world_scan_layer_reference as wref
from tests.c_probe import check_entry_points, check_layout, probe_header
from tests.fleet_kit import F32, RECT, capture, eager_on_side_stream, gpu, pairs_fleet

R = ref.record
NAN, INF = math.nan, math.inf
TRIANGLE = ((0.4, 0.0), (-0.3, 0.3), (-0.3, -0.3))
GON16 = tuple((0.4 * math.cos(2 * math.pi * k / 16), 0.4 * math.sin(2 * math.pi * k / 16)) for k in range(16))
POLYGONS = {"rect": RECT, "triangle": TRIANGLE, "gon16": GON16}
MARGIN = 1e-6          # cells: the condition on the footprint-mode inputs


def records(rows):
    return np.array([tuple(r) for r in rows], dtype=abi.PLAN_CHECK_DTYPE)


def hand_map(marks, sx=16, sy=16):
    cells = np.zeros((sy, sx), dtype=np.uint8)
    for (x, y), v in marks.items():
        cells[y, x] = v
    return cells


def solver_on_world(cells, res, ox, oy):
    from neo_mpc_planner2_amd.solver import BatchSolver
    s = BatchSolver({})
    s.set_world_map(cells, res, ox, oy)
    return s


# ------------------------------------------------------------------------------------------ 1: hand-worked, point mode
# 16 x 16 cells, resolution 1, origin 0.  ROW: twelve poses on the centres of cells (2, 8) .. (13, 8), pose i on cell
# (i + 2, 8); the marked cell (8, 8) is pose 6.  EDGE: five poses on row 3 from cell 13 on, pose 3 the first beyond the map.
ROW = [(i + 2.5, 8.5, 0.0) for i in range(12)]
EDGE = [(13.5 + i, 3.5, 0.0) for i in range(5)]
MARK = (8, 8)
HAND_CASES = (
    # name, {(x, y): raw}, plans, robot poses or None, keywords, the records by hand
    ("252 under 253", {MARK: 252}, [ROW], None, dict(max_cost=253), [R(0, 12, 12, 0, 252)]),
    ("253 under 253", {MARK: 253}, [ROW], None, dict(max_cost=253), [R(0, 12, 6, 1, 253)]),
    ("254 under 253", {MARK: 254}, [ROW], None, dict(max_cost=253), [R(0, 12, 6, 1, 254)]),
    ("253 with unknown blocking", {MARK: 253}, [ROW], None, dict(max_cost=253, unknown_blocks=True), [R(0, 12, 6, 1, 253)]),
    ("254 with unknown blocking", {MARK: 254}, [ROW], None, dict(max_cost=253, unknown_blocks=True), [R(0, 12, 6, 1, 254)]),
    ("255 does not block", {MARK: 255}, [ROW], None, dict(max_cost=253, unknown_blocks=False), [R(0, 12, 12, 0, 0)]),
    ("255 blocks", {MARK: 255}, [ROW], None, dict(max_cost=253, unknown_blocks=True), [R(0, 12, 6, 1, 255)]),
    ("252 with unknown blocking", {MARK: 252}, [ROW], None, dict(max_cost=253, unknown_blocks=True), [R(0, 12, 12, 0, 252)]),
    ("255 is no maximum", {MARK: 255, (4, 8): 7}, [ROW], None, dict(max_cost=253), [R(0, 12, 12, 0, 7)]),
    ("max_cost 1: a 1 blocks", {MARK: 1}, [ROW], None, dict(max_cost=1), [R(0, 12, 6, 1, 1)]),
    ("max_cost 1: free", {}, [ROW], None, dict(max_cost=1), [R(0, 12, 12, 0, 0)]),
    ("max_cost 254: 253 passes", {MARK: 253}, [ROW], None, dict(max_cost=254), [R(0, 12, 12, 0, 253)]),
    ("max_cost 254: 254 blocks", {MARK: 254}, [ROW], None, dict(max_cost=254), [R(0, 12, 6, 1, 254)]),
    ("a blocked pose in front of begin is not seen", {MARK: 254}, [ROW], [(11.5, 8.5, 0.0)], dict(), [R(9, 12, 12, 0, 0)]),
    ("begin on the blocked pose", {MARK: 254}, [ROW], [(8.4, 8.6, 0.0)], dict(), [R(6, 12, 6, 1, 254)]),
    ("max_poses ends one pose before", {MARK: 254}, [ROW], None, dict(max_poses=6), [R(0, 6, 6, 0, 0)]),
    ("max_poses ends on the blocked pose", {MARK: 254}, [ROW], None, dict(max_poses=7), [R(0, 7, 6, 1, 254)]),
    ("max_poses from begin", {MARK: 254}, [ROW], [(5.5, 8.5, 0.0)], dict(max_poses=3), [R(3, 6, 6, 0, 0)]),
    ("max_poses beyond the end", {MARK: 100}, [ROW], [(5.5, 8.5, 0.0)], dict(max_poses=100), [R(3, 12, 12, 0, 100)]),
    ("an empty plan between two", {MARK: 254, (14, 3): 9}, [ROW, [], EDGE[:2]], None, dict(),
     [R(0, 12, 6, 1, 254), R(0, 0, 0, 2, 0), R(0, 2, 2, 0, 9)]),
    ("an empty plan between two, robot poses", {MARK: 254}, [ROW, [], ROW], [(2.5, 8.5, 0.0), (1.0, 1.0, 0.0), (10.5, 8.5, 0.0)],
     dict(), [R(0, 12, 6, 1, 254), R(0, 0, 0, 2, 0), R(8, 12, 12, 0, 0)]),
    ("off the map is 0", {(15, 3): 50}, [EDGE], None, dict(outside_value=0), [R(0, 5, 5, 0, 50)]),
    ("off the map is 254", {(15, 3): 50}, [EDGE], None, dict(outside_value=254), [R(0, 5, 3, 1, 254)]),
    ("off the map is 255, not blocking", {(15, 3): 50}, [EDGE], None, dict(outside_value=255), [R(0, 5, 5, 0, 50)]),
    ("off the map is 255, blocking", {(15, 3): 50}, [EDGE], None, dict(outside_value=255, unknown_blocks=True), [R(0, 5, 3, 1, 255)]),
    ("below the origin", {}, [[(0.5, 0.5, 0.0), (-0.5, 0.5, 0.0)], [(0.5, 0.5, 0.0), (0.5, -1e-9, 0.0)]], None,
     dict(outside_value=254), [R(0, 2, 1, 1, 254), R(0, 2, 1, 1, 254)]),
    ("a NaN and a +inf coordinate", {}, [[(2.5, 3.5, 0.0), (NAN, 3.5, 0.0), (4.5, 3.5, 0.0)],
                                         [(2.5, 3.5, 0.0), (3.5, 3.5, 0.0), (4.5, INF, 0.0)],
                                         [(2.5, 3.5, 0.0), (-INF, 3.5, 0.0)]], None, dict(outside_value=254),
     [R(0, 3, 1, 1, 254), R(0, 3, 2, 1, 254), R(0, 2, 1, 1, 254)]),
    ("exactly at the origin: on the map", {(0, 0): 254}, [[(0.0, 0.0, 0.0)]], None, dict(outside_value=0), [R(0, 1, 0, 1, 254)]),
    ("exactly at the far edge: off the map", {(15, 8): 254}, [[(16.0, 8.5, 0.0)], [(8.5, 16.0, 0.0)]], None, dict(outside_value=77),
     [R(0, 1, 1, 0, 77), R(0, 1, 1, 0, 77)]),
    ("just inside the far edge", {(15, 8): 254}, [[(np.nextafter(16.0, 0.0), 8.5, 0.0)]], None, dict(outside_value=77),
     [R(0, 1, 0, 1, 254)]),
    ("a first pose of NaN: begin is 0", {(4, 5): 30}, [[(NAN, NAN, 0.0), (3.5, 5.5, 0.0), (4.5, 5.5, 0.0)]], [(4.5, 5.5, 0.0)],
     dict(outside_value=0), [R(0, 3, 3, 0, 30)]),
    ("a first pose of NaN is off the map", {}, [[(NAN, NAN, 0.0), (3.5, 5.5, 0.0), (4.5, 5.5, 0.0)]], [(4.5, 5.5, 0.0)],
     dict(outside_value=254), [R(0, 3, 0, 1, 254)]),
    ("a later pose of NaN does not move begin", {}, [[(3.5, 5.5, 0.0), (NAN, NAN, 0.0), (4.5, 5.5, 0.0)]], [(4.6, 5.5, 0.0)],
     dict(outside_value=254), [R(2, 3, 3, 0, 0)]),
)


def hand_inputs(case):
    name, marks, plans, robots, kw, want = case
    poses, offsets = ref.assemble(plans)
    robots = None if robots is None else np.asarray(robots, dtype=np.float64)
    return name, hand_map(marks), poses, offsets, robots, kw, records(want)


def test_transcription_on_hand_worked_maps():
    for case in HAND_CASES:
        name, cells, poses, offsets, robots, kw, want = hand_inputs(case)
        got = ref.check_plans(cells, 1.0, 0.0, 0.0, poses, offsets, robot_poses=robots, **kw)
        assert got.tolist() == want.tolist(), name
    # footprint mode, by hand: tests/test_footprint_gate.py's square outline (cells 2 .. 10 of rows and columns 2 and 10) around
    # pose (6.5, 6.5), moved one cell to the right from pose to pose
    square = ((-4.0, -4.0), (4.0, -4.0), (4.0, 4.0), (-4.0, 4.0))
    plan = [(6.5 + i, 6.5, 0.0) for i in range(4)]            # right columns 10, 11, 12, 13
    poses, offsets = ref.assemble([plan])
    cells = hand_map({(12, 6): 254, (11, 5): 200, (7, 7): 254})   # (7, 7) lies inside every outline: never on one
    got = ref.check_plans(cells, 1.0, 0.0, 0.0, poses, offsets, footprint=square)
    assert got.tolist() == records([R(0, 4, 2, 1, 254)]).tolist()
    got = ref.check_plans(cells, 1.0, 0.0, 0.0, poses, offsets, footprint=square, max_poses=2)
    assert got.tolist() == records([R(0, 2, 2, 0, 200)]).tolist()
    got = ref.check_plans(cells, 1.0, 0.0, 0.0, poses, offsets, footprint=square, max_poses=2, max_cost=200)
    assert got.tolist() == records([R(0, 2, 1, 1, 200)]).tolist()
    # an outline that leaves the map costs 254 whatever outside_value says
    far = ref.assemble([[(6.5, 6.5, 0.0), (12.5, 6.5, 0.0)]])
    got = ref.check_plans(hand_map({}), 1.0, 0.0, 0.0, *far, footprint=square, outside_value=0)
    assert got.tolist() == records([R(0, 2, 1, 1, 254)]).tolist()


def test_plan_check_layout_and_entry_points(tmp_path):
    entry_points = ("neo_mpc_check_plans", "neo_mpc_check_plans_device")
    got = probe_header(tmp_path, ["neo_mpc_plan_check_batch", "neo_mpc_plan_check"], entry_points=entry_points)
    check_layout(got, "neo_mpc_plan_check_batch", 72, struct=abi.NeoMpcPlanCheckBatch)
    check_layout(got, "neo_mpc_plan_check", 24, struct=abi.NeoMpcPlanCheck, dtype=abi.PLAN_CHECK_DTYPE)
    result = abi.PLAN_CHECK_DTYPE.names
    assert len(result) == 6 and all(abi.PLAN_CHECK_DTYPE.fields[f][0].itemsize == 4 for f in result)
    check_entry_points(entry_points)


@pytest.mark.gpu
def test_hand_worked_point_mode():
    from neo_mpc_planner2_amd.solver import BatchSolver
    with BatchSolver({}) as s:
        for case in HAND_CASES:
            name, cells, poses, offsets, robots, kw, want = hand_inputs(case)
            s.set_world_map(cells, 1.0, 0.0, 0.0)
            got = s.check_plans(poses, offsets, robot_poses=robots, **kw)
            assert got.tolist() == want.tolist(), name


# ------------------------------------------------------------------------------------------ 2: wave boundaries
# One row of a 320-cell-wide map per plan, resolution 1, origin 0: pose k of plan c on the centre of cell (k, c).
LENGTHS = (1, 63, 64, 65, 128, 129, 257, 300)


def wave_cases():
    """[(length, robot's pose index or None, {index: raw}, max_poses, (begin, end, first_blocked, status, value))]"""
    out = []
    for n in LENGTHS:                                             # a single blocking pose
        for at in sorted(set(k for k in (0, 63, 64, 65, n - 1) if k < n)):
            out.append((n, None, {at: 254}, 0, (0, n, at, 1, 254)))
        out.append((n, None, {}, 0, (0, n, n, 0, 0)))
    for b in (1, 63, 64, 65):                                     # begin forced by the robot pose
        for n in (129, 300):
            out.append((n, b, {b - 1: 254, n - 1: 253}, 0, (b, n, n - 1, 1, 253)))     # (the pose in front of begin is not seen)
            out.append((n, b, {b - 1: 254, b: 253}, 0, (b, n, b, 1, 253)))
            out.append((n, b, {b - 1: 254, b + 63: 254, b + 64: 253}, 0, (b, n, b + 63, 1, 254)))   # last lane of begin's round
        # max_poses: one round exactly, and one pose more
        out.append((300, b, {b - 1: 254, b + 64: 253}, 64, (b, b + 64, b + 64, 0, 0)))
        out.append((300, b, {b + 64: 253}, 65, (b, b + 65, b + 64, 1, 253)))
    out.append((300, None, {10: 253, 40: 254}, 0, (0, 300, 10, 1, 253)))        # two in one round: the first wins
    out.append((300, None, {70: 254, 100: 253, 290: 254}, 0, (0, 300, 70, 1, 254)))
    out.append((300, None, {63: 253, 64: 254}, 0, (0, 300, 63, 1, 253)))        # ... in neighbouring rounds
    out.append((300, None, {200: 253, 10: 255, 299: 254}, 0, (0, 300, 200, 1, 253)))   # (255 does not block here)
    out.append((300, 130, {131: 254, 260: 253}, 0, (130, 300, 131, 1, 254)))
    for n in (65, 129, 257, 300):                                 # the maximum in the last partial round
        out.append((n, None, {3: 100, n - 1: 200, 20 % n: 255}, 0, (0, n, n, 0, 200)))
        out.append((n, None, {3: 100, (n - 1) // 64 * 64: 252}, 0, (0, n, n, 0, 252)))
    out.append((300, 70, {3: 252, 80: 100, 299: 101}, 0, (70, 300, 300, 0, 101)))
    out.append((300, 0, {3: 100, 250: 200}, 200, (0, 200, 200, 0, 100)))         # (a maximum beyond end is not seen)
    return out


@functools.lru_cache(maxsize=None)
def wave_batch():
    cases = wave_cases()
    cells = np.zeros((len(cases), 320), dtype=np.uint8)
    by_max_poses = {}
    for c, (n, b, marks, max_poses, want) in enumerate(cases):
        for k, v in marks.items():
            cells[c, k] = v
        plan = [(k + 0.5, c + 0.5, 0.0) for k in range(n)]
        robot = (0.5, c + 0.5, 0.0) if b is None else (b + 0.45, c + 0.55, 0.3)
        by_max_poses.setdefault(max_poses, []).append((plan, robot, want))
    return cells, by_max_poses


def test_wave_boundary_records_by_hand_equal_the_transcription():
    cells, groups = wave_batch()
    for max_poses, group in groups.items():
        poses, offsets = ref.assemble([g[0] for g in group])
        robots = np.array([g[1] for g in group])
        got = ref.check_plans(cells, 1.0, 0.0, 0.0, poses, offsets, robot_poses=robots, max_poses=max_poses)
        assert got.tolist() == records([R(*g[2]) for g in group]).tolist(), max_poses


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["point", "footprint"])
def test_wave_boundaries(mode):
    """Point mode, and footprint mode with an outline that stays inside its pose's cell: the outline's cost is the cell's."""
    cells, groups = wave_batch()
    speck = ((0.2, 0.0), (-0.1, 0.2), (-0.1, -0.2)) if mode == "footprint" else None
    with solver_on_world(cells, 1.0, 0.0, 0.0) as s:
        for max_poses, group in groups.items():
            poses, offsets = ref.assemble([g[0] for g in group])
            robots = np.array([g[1] for g in group])
            got = s.check_plans(poses, offsets, robot_poses=robots, footprint=speck, max_poses=max_poses)
            want = records([R(*g[2]) for g in group])
            bad = [i for i in range(len(want)) if got[i].tolist() != want[i].tolist()]
            assert not bad, (max_poses, bad[:5], got[bad[:5]].tolist(), want[bad[:5]].tolist())


# ------------------------------------------------------------------------------------------ 3: the random fleet
FLEET = 64
SETTINGS = ((253, False), (120, True))          # (max_cost, unknown_blocks)
#: a fixed seed for which the condition on inputs holds for every pose of every plan, with every polygon (smallest margins
#: 4.6e-6, 1.2e-5 and 5.4e-6 cells; seed 13 puts a vertex of the 16-gon 5.6e-7 cells from an edge, seed 15 one of the rectangle
#: 4.3e-7)
FLEET_SEEDS = {"point": 19, "rect": 19, "triangle": 19, "gon16": 19}


@functools.lru_cache(maxsize=None)
def random_world():
    """make_costmap(200) with a few rectangular patches of NO_INFORMATION (255) written in."""
    cells, res, ox, oy = synthetic.make_costmap(200, seed=5)
    cells = cells.copy()
    rng = np.random.default_rng(19)
    for _ in range(6):
        x, y = rng.integers(0, 180, size=2)
        w, h = rng.integers(4, 16, size=2)
        cells[y:y + h, x:x + w] = 255
    cells.setflags(write=False)
    return cells, res, ox, oy


@functools.lru_cache(maxsize=None)
def random_fleet(seed):
    """64 ragged random-walk plans of 0 .. 300 poses, 5 cm a step, over the world and a little beyond it; every coordinate is
    kept at least 0.05 cells from a cell edge by construction; a robot pose near a random pose of each plan."""
    cells, res, ox, oy = random_world()
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 301, size=FLEET)
    lens[:3] = (0, 1, 300)
    plans, robots = [], np.zeros((FLEET, 3))
    for i, n in enumerate(lens):
        heading = rng.uniform(-math.pi, math.pi) + np.cumsum(rng.normal(0.0, 0.12, size=n))
        xy = rng.uniform(-4.5, 4.5, size=2) + 0.03 * np.cumsum(np.stack([np.cos(heading), np.sin(heading)], 1), axis=0)
        q = (xy - (ox, oy)) / res
        q = np.floor(q) + np.clip(q - np.floor(q), 0.05, 0.95)          # away from the cell edges
        plans.append(np.concatenate([(ox, oy) + q * res, heading[:, None]], 1))
        robots[i] = (0.0, 0.0, 0.0) if n == 0 else np.append(plans[-1][rng.integers(0, n), :2] + rng.normal(0.0, 0.04, size=2), 0.0)
    poses, offsets = ref.assemble(plans)
    for a in (poses, offsets, robots):
        a.setflags(write=False)
    return poses, offsets, robots


@functools.lru_cache(maxsize=None)
def random_case(mode, max_cost, unknown_blocks):
    """(poses, offsets, robots, footprint, the transcription's records); computed once, shared, never written."""
    cells, res, ox, oy = random_world()
    poses, offsets, robots = random_fleet(FLEET_SEEDS[mode])
    footprint = None if mode == "point" else np.asarray(POLYGONS[mode], dtype=np.float64)
    if footprint is None:
        q = (poses[:, :2] - (ox, oy)) / res
        assert np.abs(q - np.round(q)).min() > 0.04
    else:
        assert fref.vertex_margin(res, (ox, oy), poses, footprint) > MARGIN
    want = ref.check_plans(cells, res, ox, oy, poses, offsets, robot_poses=robots, footprint=footprint, max_cost=max_cost,
                           unknown_blocks=unknown_blocks, outside_value=255)
    want.setflags(write=False)
    return poses, offsets, robots, footprint, want


@pytest.mark.gpu
@pytest.mark.parametrize("max_cost,unknown_blocks", SETTINGS)
@pytest.mark.parametrize("mode", ["point", "rect", "triangle", "gon16"])
def test_random_fleet_matches_transcription(mode, max_cost, unknown_blocks):
    poses, offsets, robots, footprint, want = random_case(mode, max_cost, unknown_blocks)
    with solver_on_world(*random_world()) as s:
        got = s.check_plans(poses, offsets, robot_poses=robots, footprint=footprint, max_cost=max_cost,
                            unknown_blocks=unknown_blocks, outside_value=255)
    bad = [i for i in range(FLEET) if got[i].tolist() != want[i].tolist()]
    assert not bad, (bad[:5], got[bad[:5]].tolist(), want[bad[:5]].tolist())
    # the inputs exercise the check: empty, valid and blocked plans, begins and blocked poses beyond the first round
    st = want["status"]
    print(mode, max_cost, "status counts", np.bincount(st, minlength=3).tolist(), "begin >= 64:", int((want["begin"] >= 64).sum()),
          "blocked beyond begin's round:", int(((st == 1) & (want["first_blocked"] >= want["begin"] + 64)).sum()))
    assert (st == 2).sum() >= 1 and (st == 0).sum() >= 5 and (st == 1).sum() >= 5
    assert (want["begin"] >= 64).sum() >= 5 and ((st == 1) & (want["first_blocked"] > want["begin"])).sum() >= 3
    assert ((st == 0) & (want["value"] > 0)).sum() >= 3 and ((st == 1) & (want["first_blocked"] >= want["begin"] + 64)).sum() >= 3


# ------------------------------------------------------------------------------------------ 4: the live map
@pytest.mark.gpu
def test_the_check_reads_the_live_map():
    """A 32 x 32 world of 1 m cells.  The plan runs along row 16, pose i on cell (i + 4, 16).  A scan marks cell (20, 16) --
    pose 16 --, inflated with an inscribed radius of two cells."""
    world = np.zeros((32, 32), dtype=np.uint8)
    plan = [(i + 4.5, 16.5, 0.0) for i in range(24)]
    poses, offsets = ref.assemble([plan])
    inflation = (2.0, 3.0, 1.0)
    far = dict(obstacle_max_range=20.0, obstacle_min_range=0.0, raytrace_max_range=20.0, raytrace_min_range=0.0)
    sensor, hit, miss = np.array([(16.5, 12.5)]), np.array([[(20.5, 16.5)]]), np.array([[(26.5, 4.5)]])
    model = wref.WorldScanLayer()
    live = model.update(world, 1.0, 0.0, 0.0, *inflation, points=hit, sensor_origins=sensor, **far)
    assert live[16, 20] == 254 and live[16, 18] == 253 and live[16, 19] == 253 and 0 < live[16, 17] < 253
    with solver_on_world(world, 1.0, 0.0, 0.0) as s:
        valid = records([R(0, 24, 24, 0, 0)]).tolist()
        assert s.check_plans(poses, offsets).tolist() == valid
        s.update_world_scan_layer(*inflation, points=hit, sensor_origins=sensor, **far)
        for max_cost in (253, 254, 100):
            got = s.check_plans(poses, offsets, max_cost=max_cost)
            assert got.tolist() == ref.check_plans(live, 1.0, 0.0, 0.0, poses, offsets, max_cost=max_cost).tolist(), max_cost
        # the inscribed ring blocks two cells earlier under nav2's rule; under 254 only the cell itself does
        assert s.check_plans(poses, offsets, max_cost=253).tolist() == records([R(0, 24, 14, 1, 253)]).tolist()
        assert s.check_plans(poses, offsets, max_cost=254).tolist() == records([R(0, 24, 16, 1, 254)]).tolist()
        assert s.check_plans(poses, offsets, max_cost=254, max_poses=16).tolist() == records([R(0, 16, 16, 0, 253)]).tolist()
        # footprint mode reads the same map
        got = s.check_plans(poses, offsets, footprint=RECT, max_cost=254)
        assert got.tolist() == ref.check_plans(live, 1.0, 0.0, 0.0, poses, offsets, footprint=RECT, max_cost=254).tolist()
        assert got["status"][0] == 1
        # a reset alone: the roll, and the check, read the world map again
        s.reset_world_scan_layer()
        assert s.check_plans(poses, offsets).tolist() == valid
        # ... and a fresh update without the mark leaves the plan valid
        s.update_world_scan_layer(*inflation, points=miss, sensor_origins=sensor, **far)
        fresh = wref.WorldScanLayer().update(world, 1.0, 0.0, 0.0, *inflation, points=miss, sensor_origins=sensor, **far)
        assert (fresh[16] == 0).all()
        assert s.check_plans(poses, offsets).tolist() == valid
        # another world map: the composition is no longer current, the check reads the new copy
        other = world.copy()
        other[16, 9] = 254
        s.set_world_map(other, 1.0, 0.0, 0.0)
        assert s.check_plans(poses, offsets).tolist() == records([R(0, 24, 5, 1, 254)]).tolist()
        s.set_world_map(gpu(world), 1.0, 0.0, 0.0)                      # ... set on the device as well
        assert s.check_plans(poses, offsets).tolist() == valid


# ------------------------------------------------------------------------------------------ 5: footprint mode against K6
@pytest.mark.gpu
def test_footprint_mode_equals_the_footprint_gate_pose_by_pose():
    """Plan k of the batch is the plan cut off behind pose k, its robot stands on pose k and max_poses is 1: the check looks at
    pose k alone.  With max_cost 1 and unknown blocking, `value` is that pose's outline cost whatever it is -- K6's cost at
    the same pose on a costmap holding the same cells."""
    from neo_mpc_planner2_amd.solver import BatchSolver
    cells, res, ox, oy = random_world()
    n = 150
    t = np.arange(n)
    plan = np.stack([-4.9 + 0.067 * t, 3.0 * np.sin(t / 17.0) - 0.5, np.cos(t / 17.0) * 1.2 + 0.01 * t], 1)   # x grows: no pose twice
    poses, offsets = ref.assemble([plan[:k + 1] for k in range(n)])
    with BatchSolver({}) as s:
        s.set_costmap(cells, res, ox, oy)
        s.set_world_map(cells, res, ox, oy)
        for name in sorted(POLYGONS):
            costs = s.footprint_gate(POLYGONS[name], poses=plan)
            got = s.check_plans(poses, offsets, robot_poses=plan, footprint=POLYGONS[name], max_cost=1, unknown_blocks=True,
                                max_poses=1)
            assert got["begin"].tolist() == t.tolist() and got["end"].tolist() == (t + 1).tolist(), name
            assert got["value"].tolist() == costs.astype(np.int64).tolist(), name
            assert got["status"].tolist() == (costs > 0).astype(int).tolist(), name
            assert len(set(costs.tolist())) >= 5 and (costs == 254).any() and (costs == 0).any(), name


# ------------------------------------------------------------------------------------------ 6: host and device variant
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["point", "gon16"])
def test_host_variant_equals_device_variant(mode):
    import torch
    max_cost, unknown_blocks = SETTINGS[1]
    poses, offsets, robots, footprint, want = random_case(mode, max_cost, unknown_blocks)
    with solver_on_world(*random_world()) as s:
        host = s.check_plans(poses, offsets, robot_poses=robots, footprint=footprint, max_cost=max_cost,
                             unknown_blocks=unknown_blocks)
        d_results = torch.full((FLEET * 24,), 0xA5, dtype=torch.uint8, device="cuda:0")
        s.check_plans_device(gpu(poses), gpu(offsets.astype(np.int32)), d_results, robot_poses=gpu(robots),
                             footprint=None if footprint is None else gpu(footprint), max_cost=max_cost,
                             unknown_blocks=unknown_blocks)
        torch.cuda.synchronize()
        assert d_results.cpu().numpy().tobytes() == host.tobytes() == want.tobytes()
        # without robot poses every check starts at pose 0, on both variants
        host0 = s.check_plans(poses, offsets, footprint=footprint, max_cost=max_cost, unknown_blocks=unknown_blocks)
        s.check_plans_device(gpu(poses), gpu(offsets.astype(np.int32)), d_results,
                             footprint=None if footprint is None else gpu(footprint), max_cost=max_cost,
                             unknown_blocks=unknown_blocks)
        torch.cuda.synchronize()
        assert d_results.cpu().numpy().tobytes() == host0.tobytes() and (host0["begin"] == 0).all()


# ------------------------------------------------------------------------------------------ 7: refusals
@pytest.mark.gpu
def test_refusals():
    from neo_mpc_planner2_amd.solver import BatchSolver
    poses, offsets = ref.assemble([ROW, ROW[:3]])
    results = np.zeros(2, dtype=abi.PLAN_CHECK_DTYPE)
    fp = np.asarray(RECT, dtype=np.float64)

    def batch(**kw):
        b = abi.NeoMpcPlanCheckBatch()
        b.count, b.plan_poses, b.plan_offsets, b.results = 2, poses.ctypes.data, offsets.ctypes.data, results.ctypes.data
        b.max_cost, b.outside_value = 253, 255
        for k, v in kw.items():
            setattr(b, k, v)
        return b

    with BatchSolver({}) as s:
        lib, h = s._lib, s._handle
        both = (lambda b: lib.neo_mpc_check_plans(h, C.byref(b)), lambda b: lib.neo_mpc_check_plans_device(h, C.byref(b), None))
        for call in both:
            assert call(batch()) == -4                                  # NEO_MPC_ERR_NO_COSTMAP: no world map yet
        s.set_costmap(np.zeros((16, 16), dtype=np.uint8), 1.0, 0.0, 0.0)
        for call in both:
            assert call(batch()) == -4                                  # (a costmap is no world map)
        s.set_world_map(np.zeros((16, 16), dtype=np.uint8), 1.0, 0.0, 0.0)
        shapes = (dict(plan_poses=None), dict(plan_offsets=None), dict(results=None), dict(max_cost=0), dict(max_cost=255),
                  dict(unknown_blocks=2), dict(outside_value=256), dict(reserved=1),
                  dict(footprint=None, footprint_points=4), dict(footprint=fp.ctypes.data, footprint_points=0),
                  dict(footprint=fp.ctypes.data, footprint_points=2), dict(footprint=fp.ctypes.data, footprint_points=17),
                  dict(count=1 << 31))
        for kw in shapes:
            for call in both:
                assert call(batch(**kw)) == -1, kw                      # NEO_MPC_ERR_INVALID_ARGUMENT
        assert lib.neo_mpc_check_plans(h, None) == -1 and lib.neo_mpc_check_plans_device(h, None, None) == -1
        assert lib.neo_mpc_check_plans(None, C.byref(batch())) == -1 and lib.neo_mpc_check_plans_device(None, C.byref(batch()), None) == -1
        # values: the host variant alone looks at them
        down = np.array([0, 12, 3], dtype=np.uint32)
        with pytest.raises(_lib.NeoMpcError) as e:
            s.check_plans(poses, down)
        assert e.value.code == -1 and "plan_offsets" in str(e.value)
        bad_fp = fp.copy()
        bad_fp[2, 1] = np.nan
        with pytest.raises(_lib.NeoMpcError) as e:
            s.check_plans(poses, offsets, footprint=bad_fp)
        assert e.value.code == -1 and "not finite" in str(e.value)
        # count == 0 is OK on both and launches nothing; the record's other pointers may then be null
        empty = batch(count=0, plan_poses=None, plan_offsets=None, results=None)
        for call in both:
            assert call(empty) == 0
        assert s.check_plans(np.zeros((0, 3)), np.zeros(1, dtype=np.uint32)).shape == (0,)
        assert s.check_plans(poses, offsets).tolist() == records([R(0, 12, 12, 0, 0), R(0, 3, 3, 0, 0)]).tolist()


# ------------------------------------------------------------------------------------------ 8: graph capture
@pytest.mark.gpu
def test_world_scan_check_roll_can_be_captured_in_a_hip_graph():
    """fleet_kit.pairs_fleet on a free 400 x 400 world: the even robot of a pair sees, through its front scanner, a wall across
    the pair's lane; every robot's plan runs straight ahead along that lane.  world scan from ranges -> check -> roll on one
    stream, captured after one eager tick and replayed twice with new ranges and new plans in the same buffers: the records
    equal those of the same ticks made directly on a second handle, and the blocked set changes from tick to tick."""
    import torch
    from neo_mpc_planner2_amd.solver import BatchSolver
    p = pairs_fleet()
    count, size, res = p.count, p.size, p.res
    world = np.zeros((400, 400), dtype=np.uint8)
    inflation = (0.1, 0.3, 3.0)
    robot_poses = np.concatenate([p.xy, np.zeros((count, 1))], 1)
    length = 48                                                     # poses, 5 cm apart: 2.4 m ahead
    offsets = (length * np.arange(count + 1)).astype(np.int32)

    def tick_inputs(k):
        ranges = np.full((count, 1, p.beams), np.inf, dtype=F32)
        seen = np.arange(0, count, 2)[(np.arange(count // 2) + k) % 3 != 0]     # two pairs in three see a wall
        ranges[seen, 0] = ((0.6 + 0.3 * k) / np.cos(p.angle)).astype(F32)      # ... 0.7, 1.0, 1.3 m in front of the seer
        plans = np.zeros((count, length, 3))
        plans[:, :, 0] = p.xy[:, None, 0] + 0.05 * np.arange(length) + 0.01 * k
        plans[:, :, 1] = p.xy[:, None, 1] + (0.6 * (k == 2)) * (np.arange(count)[:, None] % 4 == 0)   # tick 2: every 4th plan swerves
        return ranges, plans.reshape(-1, 3)

    ticks = [tick_inputs(k) for k in range(3)]

    class CheckSide:
        def __init__(self):
            self.s = BatchSolver({})
            self.s.set_world_map(gpu(world), res, -10.0, -10.0)
            self.ranges, self.plans = gpu(ticks[0][0]), gpu(ticks[0][1])
            self.offsets, self.poses, self.origins = gpu(offsets), gpu(robot_poses), gpu(p.origins)
            self.results = torch.zeros(count * 24, dtype=torch.uint8, device="cuda:0")

        def set_inputs(self, tick):
            self.ranges.copy_(gpu(tick[0]))
            self.plans.copy_(gpu(tick[1]))

        def tick(self):
            self.s.update_world_scan_layer_from_ranges(*inflation, self.ranges, self.poses, [p.front])
            self.s.check_plans_device(self.plans, self.offsets, self.results, robot_poses=self.poses)
            self.s.roll_costmap_pool(size, size, res, self.origins, poses=self.poses)

        def result(self):
            torch.cuda.synchronize()
            return self.results.cpu().numpy().view(abi.PLAN_CHECK_DTYPE).copy()

    direct, graphed = CheckSide(), CheckSide()
    try:
        side = eager_on_side_stream(graphed.tick)
        direct.tick()
        seen = [direct.result()]
        assert graphed.result().tobytes() == seen[0].tobytes()
        g = capture(graphed.tick, side)
        for k in (1, 2):
            for x in (direct, graphed):
                x.set_inputs(ticks[k])
            torch.cuda.synchronize()
            g.replay()
            direct.tick()
            seen.append(direct.result())
            assert graphed.result().tobytes() == seen[k].tobytes(), k
            # ... and the transcription on the map the update composed
            live = direct.s.get_world_scan_layer()[1]
            want = ref.check_plans(live, res, -10.0, -10.0, ticks[k][1], offsets, robot_poses=robot_poses)
            assert seen[k].tolist() == want.tolist(), k
            assert graphed.s.get_costmap_pool()[0].tobytes() == direct.s.get_costmap_pool()[0].tobytes(), k
        blocked = [set(np.nonzero(r["status"] == 1)[0].tolist()) for r in seen]
        print("blocked plans per tick:", [len(b) for b in blocked])
        assert all(blocked) and blocked[0] != blocked[1] and blocked[1] != blocked[2] and blocked[0] != blocked[2]
        assert all((r["status"] == 0).any() for r in seen)
    finally:
        direct.s.close()
        graphed.s.close()
