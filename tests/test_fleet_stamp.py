"""The fleet stamp (K8): the other robots' outlines written into each robot's rolling window, inflation ring included --
roll -> stamp -> gate -> carrots -> solve.

nav2's layers cannot be built here, so the contract is the text in include/neo_mpc.h (neo_mpc_stamp_batch) and its
executable form the transcription in tests/fleet_stamp_reference.py.  The float64 part of the contract is + - * / alone
and rounds identically on both sides, the rest is integers, so every comparison with the transcription is exact equality of
uint8 cells: no tolerance, no dropped case.  On the GPU the polygons handed to the transcription are the ones the footprint
gate (K6) wrote for the same inputs -- the contract says the stamp uses those bit for bit -- so the last bit of a sine
cannot move a cell."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from neo_mpc_planner2_amd import _lib, abi, synthetic
from tests import fleet_stamp_reference as ref
from tests import footprint_gate_reference as gate_ref
from tests import rolling_window_reference as roll_ref
from tests.c_probe import check_entry_points, check_layout, probe_header
from tests.fleet_kit import RECT, Side, capture_fleet, gpu, replay_against_direct, standing_fleet

ENTRY_POINTS = ("neo_mpc_stamp_fleet", "neo_mpc_stamp_fleet_device", "neo_mpc_inflation_costs")
WRES, WOX, WOY, WSIZE = synthetic.RESOLUTION, -1.5, -1.5, 300         # the world: 15 m around a 12 m yard
PARAMS = (0.45, 0.9, 3.0)           # inscribed_radius, inflation_radius, cost_scaling_factor
STAMPS_ONLY = (0.3, 0.0, 1.0)       # R = 0: no ring
SIZES = {"13x11": (13, 11), "36x20": (36, 20), "200x200": (200, 200)}
RESOLUTIONS = {"5cm": 0.05, "2.5cm": 0.025}
BIG = ((1.0, 0.8), (-1.0, 0.8), (-1.0, -0.8), (1.0, -0.8))            # 80 x 64 cells at 2.5 cm: more than one 64 x 64 tile
TRIANGLE = ((0.4, 0.0), (-0.3, 0.3), (-0.3, -0.3))
GON16 = tuple((0.4 * math.cos(2 * math.pi * k / 16), 0.4 * math.sin(2 * math.pi * k / 16)) for k in range(16))
COUNT = 70                          # the search for robots in reach crosses a 64-lane batch


# ------------------------------------------------------------------------------------------ 1: the hand-worked map
def test_transcription_on_a_hand_worked_map():
    table, reach = ref.inflation_costs(0.5, 0.5, 1.0, 2.0)
    assert reach == 2 and table.tolist() == [254, 253, 166, 121, 92]
    square = [(1.25, 1.25), (3.25, 1.25), (3.25, 3.25), (1.25, 3.25)]       # its edges run through cell centres
    own = [(4.6, 0.1), (5.9, 0.1), (5.9, 1.4), (4.6, 1.4)]                  # robot 0 itself, inside its own window
    #      i = 0    1    2    3    4    5    6    7    8   9  10  11
    want = [[0,   0,  92,  92,  92,  92,  92,   0,   0,  0,  0,  0],       # l = 0
            [0, 166, 253, 253, 253, 253, 253, 166,   0,  0,  0,  0],
            [92, 253, 254, 254, 254, 254, 254, 253, 92,  0,  0,  0],
            [92, 253, 254, 254, 254, 254, 254, 253, 92,  0,  0,  0],
            [92, 253, 254, 254, 254, 254, 254, 253, 92,  0,  0,  0],
            [92, 253, 254, 254, 254, 254, 254, 253, 92,  0,  0,  0],
            [92, 253, 254, 254, 254, 254, 254, 253, 92,  0,  0,  0],
            [0, 166, 253, 253, 253, 253, 253, 166,   0,  0,  0,  0],
            [0,   0,  92,  92,  92,  92,  92,   0,   0,  0,  0,  0],
            [0,   0,   0,   0,   0,   0,   0,   0,   0,  0,  0,  0]]       # l = 9
    cells = np.zeros((2, 10, 12), dtype=np.uint8)
    origins = np.array([(0.0, 0.0), (100.0, 100.0)])
    nan = [(1.25, 1.25), (3.25, float("nan")), (3.25, 3.25), (1.25, 3.25)]
    for polygon in (square, square[::-1]):                                  # both windings
        got = ref.stamp_pool(cells, origins, 0.5, [own, polygon], 0.5, 1.0, 2.0)
        assert got[0].tolist() == want                                      # robot 0's own polygon is not stamped
        assert not got[1].any()                                             # window 1 is far from both
        assert ref.stamp_window_by_definition(cells[0], origins[0], 0.5, [polygon], table, reach).tolist() == want
    assert not ref.stamp_pool(cells, origins, 0.5, [own, nan], 0.5, 1.0, 2.0).any()
    # the combination: unknown cells take the lethal and the inscribed value only; others the maximum
    old = np.array([[255, 255, 255, 255, 200, 200, 100, 0]], dtype=np.uint8)
    dist2 = np.array([[0, 1, 2, 9, 2, 0, 2, 9]])
    assert ref.combine(old, dist2, table, reach).tolist() == [[254, 253, 255, 255, 200, 254, 166, 0]]


def test_the_fast_transcription_equals_the_definition():
    """stamp_window (bounding boxes, row-wise minimum) against stamp_window_by_definition (every cell, every pair) on
    windows cut by their neighbours in every way: robots inside, astride the edges, just outside, at both resolutions."""
    rng = np.random.default_rng(5)
    checked = 0
    for res, params in ((0.05, PARAMS), (0.025, (0.2, 0.3, 5.0)), (0.05, STAMPS_ONLY)):
        table, reach = ref.inflation_costs(res, *params)
        for size_x, size_y in ((13, 11), (36, 20)):
            cells = rng.integers(0, 256, size=(size_y, size_x)).astype(np.uint8)
            origin = rng.uniform(-3, 3, size=2)
            span = np.array([size_x, size_y]) * res
            polygons = []
            for base in (RECT, RECT[::-1], TRIANGLE, GON16, BIG):
                pose = list(origin + rng.uniform(-0.5, 1.5, size=2) * span) + [rng.uniform(-3, 3)]
                polygons.append(gate_ref.oriented(pose, base))
            for chosen in (polygons[:3], polygons[2:4], polygons[4:]):
                fast, _ = ref.stamp_window(cells, origin, res, chosen, table, reach)
                assert np.array_equal(fast, ref.stamp_window_by_definition(cells, origin, res, chosen, table, reach))
                checked += int((fast != cells).any())
    assert checked >= 12


# ------------------------------------------------------------------------------------------ 2: record and entry points
def test_stamp_batch_layout_and_entry_points(tmp_path):
    got = probe_header(tmp_path, ["neo_mpc_stamp_batch"], ["MAX_INFLATION_CELLS"], ENTRY_POINTS)
    check_layout(got, "neo_mpc_stamp_batch", 80, struct=abi.NeoMpcStampBatch)
    assert got["MAX_INFLATION_CELLS"] == abi.MAX_INFLATION_CELLS == 64 and len(ENTRY_POINTS) == 3
    check_entry_points(ENTRY_POINTS)


# ------------------------------------------------------------------------------------------ 3: the cost table
def test_inflation_costs_against_the_formula():
    from neo_mpc_planner2_amd.solver import BatchSolver
    rng = np.random.default_rng(41)
    near_integer = 0
    reaches = set()
    for _ in range(300):
        res = float(rng.choice([0.025, 0.0375, 0.05, 0.1]))
        inflation = float(rng.uniform(0.0, 64 * res))
        inscribed = float(rng.uniform(0.0, inflation))
        # (252 * factor stays above 1e-3: a cost that has decayed to within 1e-9 of the integer 0 would count as "near an
        # integer" below although no last bit can move its truncation)
        scaling = float(rng.uniform(0.5, min(10.0, 12.0 / max(inflation, 1e-9))))
        got, reach = BatchSolver.inflation_costs(res, inscribed, inflation, scaling)
        want, want_reach = ref.inflation_costs(res, inscribed, inflation, scaling)
        assert reach == want_reach == math.ceil(inflation / res) <= 64 and len(got) == reach * reach + 1
        assert got[0] == 254 and (np.diff(got.astype(np.int32)) <= 0).all()
        for n in range(1, len(got)):
            dist = math.sqrt(n) * res
            if dist <= inscribed:
                assert got[n] == 253, (res, inscribed, inflation, scaling, n)
                continue
            value = 252 * math.exp(-scaling * (dist - inscribed))
            if abs(value - round(value)) < 1e-9:          # libm's last bit may decide the truncation here
                near_integer += 1
                assert abs(int(got[n]) - int(want[n])) <= 1
            else:
                assert got[n] == want[n], (res, inscribed, inflation, scaling, n)
        reaches.add(reach)
    assert near_integer == 0
    assert len(reaches) >= 30 and max(reaches) >= 60
    lib = _lib.load()
    buf = np.zeros(8, dtype=np.uint8)
    cells = C.c_uint32(7)
    assert lib.neo_mpc_inflation_costs(0.05, 0.45, 3.3, 3.0, None, 0, C.byref(cells)) == -5       # 66 cells
    assert lib.neo_mpc_inflation_costs(0.05, 0.45, 0.9, 3.0, C.c_void_p(buf.ctypes.data), 8, None) == -1   # too small
    for bad in ((0.0, 0.45, 0.9, 3.0), (0.05, -0.1, 0.9, 3.0), (0.05, 0.45, float("nan"), 3.0), (0.05, 0.45, 0.9, float("inf"))):
        assert lib.neo_mpc_inflation_costs(*bad, None, 0, C.byref(cells)) == -1, bad
    assert not buf.any()
    assert BatchSolver.inflation_costs(0.05, 0.3, 0.0, 1.0)[0].tolist() == [254]


# ------------------------------------------------------------------------------------------ the fleet of tests 4 - 6
def pad16(polygon):
    polygon = list(polygon)
    return polygon + [polygon[-1]] * (16 - len(polygon))       # (a repeated vertex: an edge of length zero, c_e = 0)


@functools.lru_cache(maxsize=None)
def random_world():
    world = np.random.default_rng(61).integers(0, 256, size=(WSIZE, WSIZE)).astype(np.uint8)
    world.setflags(write=False)
    return world


@functools.lru_cache(maxsize=None)
def fleet(size, resolution):
    """(poses [70, 3], footprints [70, 16, 2] base frame, start origins [70, 2]) for windows of `size` at `resolution`: 60
    robots at random in the 12 m yard, two at one pose, a pair 0.3 m apart, one astride each edge of window 0 and one over
    its corner, one 1000 m away; odd robots wound clockwise; a 2.0 x 1.6 m robot, a triangle and two 16-gons among them."""
    size_x, size_y = SIZES[size]
    res = RESOLUTIONS[resolution]
    rng = np.random.default_rng(67)
    poses = np.concatenate([rng.uniform(0.0, 12.0, size=(COUNT, 2)), rng.uniform(-math.pi, math.pi, size=(COUNT, 1))], 1)
    poses[0, :2] = (6.013, 5.987)
    hx, hy = size_x * res / 2, size_y * res / 2
    poses[61] = poses[60]
    poses[63, :2] = poses[62, :2] + (0.3, 0.0)
    for j, (dx, dy) in zip(range(64, 69), ((-hx, 0.0), (hx, 0.0), (0.0, -hy), (0.0, hy), (hx, hy))):
        poses[j, :2] = poses[0, :2] + (dx, dy)
    poses[69, :2] = (1000.0, 1000.0)
    shapes = {5: BIG, 6: TRIANGLE, 7: GON16, 8: GON16, 66: TRIANGLE}
    footprints = np.array([pad16(shapes.get(j, RECT)[::-1] if j % 2 else shapes.get(j, RECT)) for j in range(COUNT)])
    start = poses[:, :2] - (hx, hy) + 0.013
    for a in (poses, footprints, start):
        a.setflags(write=False)
    return poses, footprints, start


@functools.lru_cache(maxsize=None)
def cpu_case():
    """The 36 x 20 windows at 5 cm wholly on the CPU: rolled by the rolling-window transcription, polygons oriented in
    Python.  (origins, cells before, polygons, cells after, squared distances)."""
    poses, footprints, start = fleet("36x20", "5cm")
    origins, old = roll_ref.roll(random_world(), WRES, WOX, WOY, start, 36, 20, 0.05, poses=poses, outside_value=255)
    polygons = np.array([gate_ref.oriented(poses[j], footprints[j]) for j in range(COUNT)])
    new, dist2 = ref.stamp_pool(old, origins, 0.05, polygons, *PARAMS, want_dist2=True)
    for a in (origins, old, polygons, new, dist2):
        a.setflags(write=False)
    return origins, old, polygons, new, dist2


# ------------------------------------------------------------------------------------------ 4: the fixture has teeth
def test_the_fleet_takes_every_branch_of_the_combination():
    origins, old, polygons, new, dist2 = cpu_case()
    table, reach = ref.inflation_costs(0.05, *PARAMS)
    assert reach == 18
    hit = dist2 <= reach * reach
    c = np.where(hit, table[np.where(hit, dist2, 0)], 0).astype(np.int32)
    o = old.astype(np.int32)
    branches = {"unknown, lethal or inscribed": (o == 255) & (c >= 253), "unknown, ring": (o == 255) & (c > 0) & (c < 253),
                "old wins": (o > c) & (c > 0) & (o != 255), "new wins": (o < c)}
    for name, where in branches.items():
        assert where.any(), name
    assert (new[branches["unknown, ring"]] == 255).all() and (new[branches["new wins"]] == c[branches["new wins"]]).all()
    assert (new[69] == old[69]).all() and (old[69] == 255).all()          # the robot 1000 m away: nobody in reach
    assert (new[0] != old[0]).any() and (new[60] == 254).any()            # ... and the others have neighbours
    # permuting the robots (windows with them) permutes the pool: the rule does not depend on their order
    perm = np.random.default_rng(71).permutation(COUNT)
    assert np.array_equal(ref.stamp_pool(old[perm], origins[perm], 0.05, polygons[perm], *PARAMS), new[perm])


# ------------------------------------------------------------------------------------------ shared GPU helpers
def solver_with_world(params=None, world=None, geometry=(WRES, WOX, WOY)):
    from neo_mpc_planner2_amd.solver import BatchSolver
    s = BatchSolver(params or {})
    s.set_world_map(random_world() if world is None else world, *geometry)
    return s


def rolled(s, size, resolution):
    """Rolls the fleet's windows (host call) and returns (origins, cells, K6's polygons for the fleet)."""
    poses, footprints, start = fleet(size, resolution)
    size_x, size_y = SIZES[size]
    origins = start.copy()
    s.roll_costmap_pool(size_x, size_y, RESOLUTIONS[resolution], origins, poses=poses)
    cells, back = s.get_costmap_pool()
    assert back.tolist() == origins.tolist()
    _, polygons = s.footprint_gate(footprints, poses=poses, map_indices=np.arange(COUNT, dtype=np.int32), want_polygons=True)
    return origins, cells, polygons


def refill(s, size, resolution, origins):
    """The windows as the roll left them: filled again where they are."""
    s.roll_costmap_pool(*SIZES[size], RESOLUTIONS[resolution], origins.copy())


# ------------------------------------------------------------------------------------------ 5: the stamp
#: every window size at both resolutions with the ring (R = 18 and 36), and the ring-less parameters (R = 0) on one geometry
STAMP_CASES = [(size, resolution, PARAMS) for size in sorted(SIZES) for resolution in sorted(RESOLUTIONS)] + \
              [("36x20", "5cm", STAMPS_ONLY)]


@pytest.mark.gpu
@pytest.mark.parametrize("size,resolution,params", STAMP_CASES,
                         ids=["%s-%s-%s" % (a, b, "ring" if c is PARAMS else "stamps-only") for a, b, c in STAMP_CASES])
def test_stamp_equals_the_transcription(size, resolution, params):
    poses, footprints, _ = fleet(size, resolution)
    res = RESOLUTIONS[resolution]
    with solver_with_world() as s:
        origins, old, polygons = rolled(s, size, resolution)
        want = ref.stamp_pool(old, origins, res, polygons, *params)
        assert (want != old).any() and (want[69] == old[69]).all()
        touched = int((want != old).sum())
        print("%s %s R=%d: %d cells change" % (size, resolution, ref.inflation_costs(res, *params)[1], touched))
        reversed_polygons = np.ascontiguousarray(polygons[:, ::-1])     # the other winding of every robot
        variants = (("host polygons", lambda: s.stamp_fleet(*params, polygons=polygons)),
                    ("host polygons, other winding", lambda: s.stamp_fleet(*params, polygons=reversed_polygons)),
                    ("host footprint + poses", lambda: s.stamp_fleet(*params, footprint=footprints, poses=poses)),
                    ("device polygons", lambda: s.stamp_fleet(*params, polygons=gpu(polygons))),
                    ("device footprint + poses", lambda: s.stamp_fleet(*params, footprint=gpu(footprints), poses=gpu(poses))))
        for k, (name, call) in enumerate(variants):
            if k:
                refill(s, size, resolution, origins)
            call()
            got, back = s.get_costmap_pool()
            assert back.tolist() == origins.tolist(), name
            assert np.array_equal(got, want), (name, size, resolution, int((got != want).sum()))
        # stamps are not undone and stamping twice changes nothing more
        s.stamp_fleet(*params, polygons=polygons)
        assert np.array_equal(s.get_costmap_pool()[0], want)


@pytest.mark.gpu
def test_stamp_with_a_shared_footprint_and_with_problems():
    """One footprint for all (per_robot_footprints 0, four points) and poses taken from the request records (cur_xy, the yaw
    of cur_q), host and device: the polygons are K6's for the same inputs."""
    import torch
    size, resolution = "36x20", "5cm"
    poses, _, start = fleet(size, resolution)
    probs = synthetic.make_problems(COUNT, 200, seed=3)
    probs["cur_xy"] = poses[:, :2]
    probs["cur_q"] = synthetic.yaw_quat(poses[:, 2])
    probs["map_index"] = np.arange(COUNT, dtype=np.int32)
    base = np.asarray(RECT, dtype=np.float64)
    dev = "cuda:0"
    with solver_with_world() as s:
        origins, old, _ = rolled(s, size, resolution)
        _, by_pose = s.footprint_gate(base, poses=poses, map_indices=probs["map_index"], want_polygons=True)
        _, by_request = s.footprint_gate(base, problems=probs.copy(), want_polygons=True)
        d_probs = torch.from_numpy(probs.view(np.uint8).reshape(COUNT, -1)).to(dev)
        for polygons, calls in ((by_pose, (lambda: s.stamp_fleet(*PARAMS, footprint=base, poses=poses),
                                           lambda: s.stamp_fleet(*PARAMS, footprint=torch.from_numpy(base).to(dev),
                                                                 poses=torch.from_numpy(poses.copy()).to(dev)))),
                                (by_request, (lambda: s.stamp_fleet(*PARAMS, footprint=base, problems=probs),
                                              lambda: s.stamp_fleet(*PARAMS, footprint=torch.from_numpy(base).to(dev),
                                                                    problems=d_probs)))):
            want = ref.stamp_pool(old, origins, 0.05, polygons, *PARAMS)
            assert (want != old).any()
            for call in calls:
                refill(s, size, resolution, origins)
                call()
                assert np.array_equal(s.get_costmap_pool()[0], want)


@pytest.mark.gpu
def test_a_fleet_of_one_leaves_the_pool_as_it_was():
    cells = np.random.default_rng(73).integers(0, 256, size=(1, 20, 36)).astype(np.uint8)
    with solver_with_world() as s:
        s.set_costmap_pool(cells, 0.05, np.array([(1.0, 2.0)]))
        s.stamp_fleet(*PARAMS, footprint=np.asarray(RECT), poses=np.array([(1.9, 2.5, 0.3)]))   # in the middle of its window
        assert np.array_equal(s.get_costmap_pool()[0], cells)


# ------------------------------------------------------------------------------------------ 6: order independence
@pytest.mark.gpu
def test_permuting_the_robots_permutes_the_pool():
    size, resolution = "36x20", "5cm"
    poses, footprints, start = fleet(size, resolution)
    perm = np.random.default_rng(71).permutation(COUNT)
    pools = []
    with solver_with_world() as s:
        for order in (np.arange(COUNT), perm):
            origins = start[order].copy()
            s.roll_costmap_pool(36, 20, 0.05, origins, poses=poses[order].copy())
            s.stamp_fleet(*PARAMS, footprint=footprints[order].copy(), poses=poses[order].copy())
            pools.append(s.get_costmap_pool())
    assert pools[1][1].tolist() == pools[0][1][perm].tolist()
    assert np.array_equal(pools[1][0], pools[0][0][perm])
    assert not np.array_equal(pools[1][0], pools[0][0])


# ------------------------------------------------------------------------------------------ 7: the border is intact
@pytest.mark.gpu
def test_a_solve_and_a_gate_cannot_tell_a_stamped_pool_from_an_ingested_one():
    """Geometry and requests of the rolled-against-ingested test of the rolling windows (eight windows of 160 x 160 cells,
    768 requests spread over them); here the windows are rolled AND stamped -- a polygon next to the centre of every window
    -- against the transcription's cells passed through neo_mpc_set_costmap_pool_device: commands, states, warm starts
    and gate costs are bit-identical, so the stamp wrote cells only: border and pitch padding are still lethal."""
    import torch
    from neo_mpc_planner2_amd.solver import BatchSolver, DeviceBatch
    from oracle import mpc_oracle as orc
    m, size, count = 8, 160, 768
    rng = np.random.default_rng(81)
    world, res, wox, woy = synthetic.make_costmap(600, seed=90)
    offsets = rng.uniform(-10.0, 10.0, size=(m, 2))
    probs = synthetic.make_problems(count, size, seed=82)
    idx = rng.integers(0, m, size=count).astype(np.int32)
    probs["map_index"] = idx
    probs["cur_xy"] += offsets[idx]
    probs["goal_xyz"][:, :2] += offsets[idx]
    st, warm = synthetic.make_states(probs, 3)
    start = offsets - 4.3
    # "robot" k stands next to the centre of window k + 1: every window holds one stamped neighbour, none its own
    robots = np.concatenate([np.roll(offsets, -1, axis=0) + (1.1, 0.6), rng.uniform(-3, 3, size=(m, 1))], 1)
    polygons = np.array([gate_ref.oriented(p, RECT) for p in robots])
    fp = gpu(np.asarray(RECT, dtype=np.float64))
    results = []
    with BatchSolver(orc.make_params()) as s:
        s.set_world_map(gpu(world), res, wox, woy)
        d_orig = gpu(start)
        s.roll_costmap_pool(size, size, res, d_orig, poses=gpu(np.concatenate([offsets, np.zeros((m, 1))], 1)))
        torch.cuda.synchronize()
        raw, want_o = s.get_costmap_pool()
        stamped = ref.stamp_pool(raw, want_o, res, polygons, *PARAMS)
        assert all((stamped[k] == 254).sum() > (raw[k] == 254).sum() for k in range(m))
    for how in ("stamped", "ingested"):
        with BatchSolver(orc.make_params()) as s:
            if how == "stamped":
                s.set_world_map(gpu(world), res, wox, woy)
                d_orig = gpu(start)
                s.roll_costmap_pool(size, size, res, d_orig, poses=gpu(np.concatenate([offsets, np.zeros((m, 1))], 1)))
                s.stamp_fleet(*PARAMS, polygons=gpu(polygons))
            else:
                d_orig = gpu(want_o)
                s.set_costmap_pool(gpu(stamped), res, d_orig)
            b = DeviceBatch(probs, st, warm, "cuda:0")
            costs = torch.zeros(count, dtype=torch.float64, device="cuda:0")
            s.footprint_gate_device(fp, costs, problems=b.problems)
            s.solve_device(b.problems, b.states, b.warm, b.commands, solution=b.solution)
            torch.cuda.synchronize()
            cells, back = s.get_costmap_pool()
            results.append((b.commands_host().copy(), b.states_host().copy(), b.warm.cpu().numpy(), costs.cpu().numpy(),
                            cells, back, s.kernel_info()))
    a, b = results
    assert a[5].tolist() == want_o.tolist() == b[5].tolist() and np.array_equal(a[4], stamped) and np.array_equal(b[4], stamped)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    assert a[3].tobytes() == b[3].tobytes() and a[6] == b[6]
    assert (a[3] >= 254).any() and (a[3] == 0).any()


# ------------------------------------------------------------------------------------------ 8: the tick sees the neighbour
@pytest.mark.gpu
def test_the_tick_sees_the_neighbour():
    """World all free; A at the centre of its window, B ahead of it with its nearest stamped cell half the solver's reach
    from A's cell, C beside B with its outline through B's inscribed ring only.  roll -> stamp -> gate -> solve: A's
    command says a wall is in reach (it does not without the stamp) and the gate costs are the transcription's."""
    import torch
    from neo_mpc_planner2_amd.solver import BatchSolver, DeviceBatch
    from oracle import mpc_oracle as orc
    size, res = 100, 0.05
    world = np.zeros((400, 400), dtype=np.uint8)
    dev = "cuda:0"
    with BatchSolver(orc.make_params()) as s:
        s.set_world_map(world, res, -10.0, -10.0)
        a_xy = np.array([0.012, 0.017])
        start = np.array([a_xy - size * res / 2 + 0.013] * 3)
        s.roll_costmap_pool(size, size, res, start.copy(), poses=np.array([(a_xy[0], a_xy[1], 0.0)] * 3))
        reach = s.kernel_info()["reach_cells"]
        half = reach // 2
        assert half >= 1
        # A's cell and its centre on A's lattice; B's rear edge a quarter cell short of the centre of column a_i + half
        o_a = roll_ref.move_origin(start[0], a_xy, size, size, res)
        a_i, a_l = int((a_xy[0] - o_a[0]) / res), int((a_xy[1] - o_a[1]) / res)
        rear = o_a[0] + (a_i + half + 0.5) * res - res / 4
        b_xy = np.array([rear + 0.35, a_xy[1]])
        c_xy = b_xy + (0.0, 0.25 + 0.2 + 0.25)              # 0.2 m between the outlines: inside the 0.45 m inscribed ring
        poses = np.array([(a_xy[0], a_xy[1], 0.0), (b_xy[0], b_xy[1], 0.0), (c_xy[0], c_xy[1], 0.0)])
        probs, st, warm = standing_fleet(3, poses[:, :2], poses[:, :2] + (5.0, 0.0), seed=5)
        base = torch.from_numpy(np.asarray(RECT, dtype=np.float64)).to(dev)
        d_poses = torch.from_numpy(poses).to(dev)
        out = {}
        for stamp in (False, True):
            d_orig = torch.from_numpy(start.copy()).to(dev)
            b = DeviceBatch(probs, st, warm, dev)
            costs = torch.zeros(3, dtype=torch.float64, device=dev)
            s.roll_costmap_pool(size, size, res, d_orig, poses=d_poses)
            if stamp:
                s.stamp_fleet(*PARAMS, footprint=base, poses=d_poses)
            s.footprint_gate_device(base, costs, poses=d_poses, problems=b.problems)
            s.solve_device(b.problems, b.states, b.warm, b.commands)
            torch.cuda.synchronize()
            out[stamp] = (b.commands_host().copy(), costs.cpu().numpy(), s.get_costmap_pool())
    cells, origins = out[True][2]
    assert not out[False][2][0].any() and origins.tolist() == out[False][2][1].tolist()
    polygons = np.array([gate_ref.oriented(p, RECT) for p in poses])        # (yaw 0: exact on both sides)
    want, dist2 = ref.stamp_pool(out[False][2][0], origins, res, polygons, *PARAMS, want_dist2=True)
    assert np.array_equal(cells, want)
    assert origins[0].tolist() == list(o_a) and dist2[0][a_l, a_i] == half * half     # B is where the test says it is
    assert out[True][0]["flags"][0] & abi.FLAG_WALL_IN_REACH and not out[False][0]["flags"][0] & abi.FLAG_WALL_IN_REACH
    gate = gate_ref.gate(want, res, origins, poses, np.asarray(RECT), map_indices=np.arange(3))
    print("reach %d cells, gate costs %s" % (reach, out[True][1].tolist()))
    assert out[True][1].tolist() == gate.tolist() and not out[False][1].any()
    assert gate[2] == 253.0                                  # C: through B's inscribed ring, on no lethal cell


# ------------------------------------------------------------------------------------------ 9: refusals
@pytest.mark.gpu
def test_refusals_leave_the_pool_alone():
    from neo_mpc_planner2_amd.solver import BatchSolver
    held = np.random.default_rng(37).integers(0, 256, size=(2, 20, 36)).astype(np.uint8)
    held_origins = np.array([(1.0, 2.0), (1.5, 2.2)])
    poses = np.array([(1.9, 2.5, 0.3), (2.4, 2.7, -1.0)])
    base = np.asarray(RECT, dtype=np.float64)
    polygons = np.array([gate_ref.oriented(p, RECT) for p in poses])
    probs = synthetic.make_problems(2, 200, seed=1)
    nan_pose, nan_base, nan_polygons, nan_probs = poses.copy(), base.copy(), polygons.copy(), probs.copy()
    nan_pose[1, 2] = np.nan
    nan_base[2, 0] = np.inf
    nan_polygons[0, 3, 1] = np.nan
    nan_probs["cur_q"][1, 3] = np.nan
    with BatchSolver({}) as s:
        lib, h = s._lib, s._handle

        def call(device=False, **over):
            b = abi.NeoMpcStampBatch()
            b.count, b.footprint, b.footprint_points, b.poses = 2, base.ctypes.data, 4, poses.ctypes.data
            b.inscribed_radius, b.inflation_radius, b.cost_scaling_factor = PARAMS
            for k, v in over.items():
                setattr(b, k, v)
            if device:
                return lib.neo_mpc_stamp_fleet_device(h, C.byref(b), None)
            return lib.neo_mpc_stamp_fleet(h, C.byref(b))

        assert call() == -4 and call(device=True) == -4                     # NEO_MPC_ERR_NO_COSTMAP
        s.set_costmap(held[0], 0.05, 1.0, 2.0)
        assert call() == -5 and call(device=True) == -5                     # a single costmap: NEO_MPC_ERR_UNSUPPORTED
        assert np.array_equal(s.get_costmap_pool()[0][0], held[0])
        s.set_costmap_pool(held, 0.05, held_origins)

        def pool_is_untouched():
            got, back = s.get_costmap_pool()
            return np.array_equal(got, held) and back.tolist() == held_origins.tolist()

        shape = [dict(reserved=1), dict(footprint_points=2), dict(footprint_points=17), dict(per_robot_footprints=2),
                 dict(footprint=None), dict(poses=None), dict(count=3), dict(count=1)]
        for name in ("inscribed_radius", "inflation_radius", "cost_scaling_factor"):
            shape += [{name: -0.1}, {name: float("nan")}, {name: float("inf")}]
        values = [dict(poses=nan_pose.ctypes.data), dict(footprint=nan_base.ctypes.data),
                  dict(polygons=nan_polygons.ctypes.data), dict(poses=None, problems=nan_probs.ctypes.data)]
        for over in shape + values:                                         # the host variant looks at the values too
            assert pool_is_untouched()
            assert call(**over) == -1, over
            assert lib.neo_mpc_last_error_code() == -1 and pool_is_untouched()
        for over in shape:                                                  # the device variant: the record's shape alone
            assert call(device=True, **over) == -1, over
            assert pool_is_untouched()
        assert lib.neo_mpc_stamp_fleet(h, None) == -1 and lib.neo_mpc_stamp_fleet_device(h, None, None) == -1
        assert lib.neo_mpc_stamp_fleet(None, C.byref(abi.NeoMpcStampBatch())) == -1
        for device in (False, True):
            assert call(device, inflation_radius=3.3) == -5                 # 66 cells at 5 cm
            assert pool_is_untouched()
            assert call(device, count=0) == 0 and pool_is_untouched()       # nothing to do
        assert call(polygons=polygons.ctypes.data, footprint=None, poses=None) == 0      # polygons alone are enough
        assert not pool_is_untouched()


# ------------------------------------------------------------------------------------------ 10: graph capture
@pytest.mark.gpu
def test_roll_stamp_gate_solve_can_be_captured_in_a_hip_graph():
    """After one eager call -- it builds the cost table and allocates -- roll -> stamp -> gate -> solve is captured on one
    stream, a linear chain, and replayed with the poses rewritten in between; pool, gate costs and commands equal the
    same calls made directly on a second handle."""
    import torch
    f = capture_fleet(120)                                        # 64 robots within 4 m x 4 m: windows full of neighbours
    rng = np.random.default_rng(93)
    ticks = [(np.concatenate([f.probs["cur_xy"] + rng.uniform(-0.4, 0.4, size=(f.count, 2)) * k,
                              rng.uniform(-3, 3, size=(f.count, 1))], 1),) for k in range(3)]
    fp = gpu(np.asarray(RECT, dtype=np.float64))

    class StampSide(Side):
        def tick(self):
            self.s.roll_costmap_pool(f.sx, f.sy, f.res, self.origins, poses=self.poses)
            self.s.stamp_fleet(*PARAMS, footprint=fp, poses=self.poses)
            self.s.footprint_gate_device(fp, self.costs, poses=self.poses, problems=self.b.problems)
            self.s.solve_device(self.b.problems, self.b.states, self.b.warm, self.b.commands, solution=self.b.solution)

        def result(self):
            return super().result() + (self.s.get_costmap_pool()[0].tobytes(),)

    with replay_against_direct(lambda: StampSide(f, ticks[0]), ticks, changed=(4,)) as (direct, a, _):   # the pool changed
        # ... and the pool is the stamped one: the transcription on the rolled windows, K6's polygons
        s = direct.s
        s.roll_costmap_pool(f.sx, f.sy, f.res, direct.origins, poses=direct.poses)
        torch.cuda.synchronize()
        raw, origins = s.get_costmap_pool()
        _, polygons = s.footprint_gate(np.asarray(RECT), poses=ticks[2][0], map_indices=f.probs["map_index"], want_polygons=True)
        want = ref.stamp_pool(raw, origins, f.res, polygons, *PARAMS)
        assert np.frombuffer(a[4], dtype=np.uint8).tolist() == want.reshape(-1).tolist() and (want != raw).any()


# ------------------------------------------------------------------------------------------ 11: the closed loop
@pytest.mark.gpu
def test_closed_loop_two_robots_head_on():
    """Two robots drive at each other from 4 m on an all-free world.  Without the stamp they drive through each other
    (the control run: centres within 0.35 m -- otherwise the inputs are wrong).  With it the collision latch trips when
    a rollout stage enters a cell >= 253, and those reach 0.45 m (the inscribed radius) beyond the other robot's outline:
    the centres never come closer than 0.45 m and both robots report NEO_MPC_FLAG_STOPPED at some tick."""
    import torch
    from neo_mpc_planner2_amd import fleet as fleet_loop
    from neo_mpc_planner2_amd.solver import BatchSolver, DeviceBatch
    from oracle import mpc_oracle as orc
    size, res, ticks = 100, 0.05, 150
    world = np.zeros((400, 400), dtype=np.uint8)
    probs, st, warm = standing_fleet(2, ((-2.0, 0.011), (2.0, 0.011)), ((6.0, 0.011), (-6.0, 0.011)), yaw=np.array([0.0, math.pi]))
    runs = {}
    with BatchSolver(orc.make_params()) as s:
        s.set_world_map(world, res, -10.0, -10.0)
        for stamp in (None, PARAMS):
            seen, flags = [], []
            d_orig = torch.from_numpy(probs["cur_xy"] - size * res / 2 + 0.013).to("cuda:0")
            s.roll_costmap_pool(size, size, res, d_orig)             # (the handle has a pool before the loop's first tick)
            b = DeviceBatch(probs, st, warm, "cuda:0")
            fleet_loop.closed_loop(s, b, ticks, before_tick=lambda t, pos: seen.append(pos.cpu().numpy().copy()),
                                   after_tick=lambda t, cm: flags.append(cm["flags"].copy()), footprint=RECT,
                                   rolling=(size, size, res, d_orig), stamp=stamp)
            torch.cuda.synchronize()
            distance = np.array([np.hypot(*(p[0] - p[1])) for p in seen])
            runs[stamp] = (distance, np.array(flags))
    print("closest approach: %.3f m without the stamp, %.3f m with it" % (runs[None][0].min(), runs[PARAMS][0].min()))
    assert runs[None][0].min() <= 0.35, "the control run: the robots did not meet"
    distance, flags = runs[PARAMS]
    assert distance.min() >= 0.45
    assert ((flags & abi.FLAG_STOPPED) != 0).any(axis=0).all()
