"""The footprint gate (K6): `footprintCostAtPose` of src/NeoMpcPlanner.cpp:218-219 for a fleet, on the device map(s).

nav2 cannot be built here, so the contract is the text in include/neo_mpc.h and its executable form is the pure-Python
transcription in tests/footprint_gate_reference.py (iterative LineIterator walk, sequential fold).  CPU tests pin the
transcription on hand-worked maps, the closed form of the line walk against the iterative one, and the record layout;
GPU tests compare the kernel with the transcription by exact equality.

A vertex that sits on a cell boundary to within rounding may land in either cell (device and libm sin / cos differ in the
last bits), so the tests on random poses assert that no vertex of any robot lies within 1e-6 cells of a cell edge -- a
condition on the inputs (fixed seeds), not a tolerance; no robot is dropped."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from neo_mpc_planner2_amd import _lib, abi, synthetic
from tests import footprint_gate_reference as ref
from tests.c_probe import check_entry_points, check_layout, probe_header
from tests.fleet_kit import RECT, gpu

RES = synthetic.RESOLUTION
TRIANGLE = ((0.4, 0.0), (-0.3, 0.3), (-0.3, -0.3))
GON16 = tuple((0.4 * math.cos(2 * math.pi * k / 16), 0.4 * math.sin(2 * math.pi * k / 16)) for k in range(16))
POLYGONS = {"rect": RECT, "triangle": TRIANGLE, "gon16": GON16}
MARGIN = 1e-6          # cells: the condition on inputs


# ------------------------------------------------------------------------------------------ hand-worked cases
# 16 x 16 cells, resolution 1, origin 0, pose (0, 0, 0): the oriented polygon IS the base polygon, every cell is certain.
# The square's edges: e0 row y = 2 (x 2..10), e1 column x = 10 (y 2..10), e2 row y = 10 (x 10..2), closing e3 column x = 2.
SQUARE = ((2.5, 2.5), (10.5, 2.5), (10.5, 10.5), (2.5, 10.5))
HAND_CASES = (
    # name, {(x, y): raw value}, polygon, expected cost
    ("unknown edge before a lethal edge", {(5, 2): 255, (10, 6): 254}, SQUARE, 255),            # edges cost [255, 254, 0, 0]
    ("lethal edge before an unknown edge", {(5, 2): 253, (10, 6): 254, (6, 10): 255}, SQUARE, 254),   # [253, 254, 255, 0]
    ("unknown and lethal on one edge", {(4, 2): 255, (7, 2): 254}, SQUARE, 254),                # that edge costs 254
    ("vertex off the map after an unknown edge", {(5, 2): 255},
     ((2.5, 2.5), (10.5, 2.5), (10.5, 20.5), (2.5, 10.5)), 254),
    ("first vertex off the map", {}, ((-1.5, 2.5), (10.5, 2.5), (10.5, 10.5), (2.5, 10.5)), 254),
    ("all free", {}, SQUARE, 0),
    ("all vertices in one cell", {(3, 3): 100, (4, 3): 200, (3, 4): 200}, ((3.2, 3.2), (3.7, 3.2), (3.7, 3.7), (3.2, 3.7)), 100),
    ("closing edge alone carries the maximum", {(5, 2): 100, (2, 6): 200}, SQUARE, 200),
    ("closing edge alone is unknown", {(5, 2): 100, (2, 6): 255}, SQUARE, 255),
    ("closing edge alone is lethal", {(5, 2): 100, (2, 6): 254}, SQUARE, 254),
)


def hand_map(marks):
    cells = np.zeros((16, 16), dtype=np.uint8)
    for (x, y), v in marks.items():
        cells[y, x] = v
    return cells


def test_transcription_on_hand_worked_maps():
    for name, marks, poly, want in HAND_CASES:
        got = ref.gate(hand_map(marks), 1.0, (0.0, 0.0), [(0.0, 0.0, 0.0)], poly)
        assert got[0] == want, name
    # the walk itself, by hand: a shallow line steps in y at its middle, a steep one in x
    assert ref.line_cells(0, 0, 4, 1) == [(0, 0), (1, 0), (2, 1), (3, 1), (4, 1)]
    assert ref.line_cells(3, 5, 2, 1) == [(3, 5), (3, 4), (2, 3), (2, 2), (2, 1)]
    assert ref.line_cells(7, 7, 7, 7) == [(7, 7)]


def test_closed_form_equals_the_iterative_walk_exhaustively():
    n = 12
    for x0 in range(n):
        for y0 in range(n):
            for x1 in range(n):
                for y1 in range(n):
                    it = ref.line_cells(x0, y0, x1, y1)
                    assert ref.closed_form_cells(x0, y0, x1, y1) == it
                    assert it[0] == (x0, y0) and it[-1] == (x1, y1)


def test_footprint_batch_layout_and_entry_points(tmp_path):
    entry_points = ("neo_mpc_footprint_gate", "neo_mpc_footprint_gate_device")
    got = probe_header(tmp_path, ["neo_mpc_footprint_batch"], entry_points=entry_points)
    check_layout(got, "neo_mpc_footprint_batch", 64, struct=abi.NeoMpcFootprintBatch)
    check_entry_points(entry_points)


# ------------------------------------------------------------------------------------------ shared GPU inputs
@functools.lru_cache(maxsize=None)
def random_map():
    """make_costmap(200) with a few rectangular patches of NO_INFORMATION (255) written in."""
    cells, res, ox, oy = synthetic.make_costmap(200, seed=3)
    cells = cells.copy()
    rng = np.random.default_rng(17)
    for _ in range(8):
        x, y = rng.integers(0, 180, size=2)
        w, h = rng.integers(4, 20, size=2)
        cells[y:y + h, x:x + w] = 255
    cells.setflags(write=False)
    return cells, res, ox, oy


def random_poses(count, seed, size=200):
    """Positions over the whole map extent plus 0.5 m beyond it (some outlines leave the map), any yaw."""
    rng = np.random.default_rng(seed)
    half = size * RES / 2.0 + 0.5
    return np.concatenate([rng.uniform(-half, half, size=(count, 2)), rng.uniform(-math.pi, math.pi, size=(count, 1))], 1)


#: fixed seeds for which the condition on inputs holds (seed 41 puts a vertex of the 16-gon 1.6e-7 cells from an edge)
CASE_SEEDS = {"rect": 41, "triangle": 41, "gon16": 45}


@functools.lru_cache(maxsize=None)
def random_case(name, count=512):
    """(poses, transcription's costs) of test 4 for one polygon; computed once, shared, never written."""
    cells, res, ox, oy = random_map()
    poses = random_poses(count, CASE_SEEDS[name])
    assert ref.vertex_margin(res, (ox, oy), poses, POLYGONS[name]) > MARGIN
    want = ref.gate(cells, res, (ox, oy), poses, POLYGONS[name])
    poses.setflags(write=False)
    want.setflags(write=False)
    return poses, want


def solver_on(cmap, params=None):
    from neo_mpc_planner2_amd.solver import BatchSolver
    s = BatchSolver(params or {})
    s.set_costmap(*cmap)
    return s


# ------------------------------------------------------------------------------------------ GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(POLYGONS))
def test_gate_matches_transcription_on_random_poses(name):
    poses, want = random_case(name)
    with solver_on(random_map()) as s:
        got = s.footprint_gate(POLYGONS[name], poses=poses)
    assert got.tolist() == want.tolist()
    # the inputs exercise the gate: outlines off the map, on lethal cells, on unknown cells, on inflated and on free ones
    assert (want == 254).sum() >= 20 and (want == 255).sum() >= 5 and (want == 0).sum() >= 5
    assert ((want > 0) & (want < 253)).sum() >= 20


@pytest.mark.gpu
def test_long_and_degenerate_edges():
    """A 5.2 m x 0.1 m rectangle: edges of more than 64 cells, so a lane takes more than one cell of the outline; a 1 cm
    square: all vertices in one or two cells (edges of a single cell, dx = dy = 0)."""
    cells, res, ox, oy = random_map()
    long_rect = ((2.6, 0.05), (-2.6, 0.05), (-2.6, -0.05), (2.6, -0.05))
    tiny = ((0.005, 0.005), (-0.005, 0.005), (-0.005, -0.005), (0.005, -0.005))
    with solver_on(random_map()) as s:
        for poly, seed in ((long_rect, 52), (tiny, 53)):
            poses = random_poses(64, seed)
            poses[:, :2] *= 0.8 if poly is long_rect else 1.0       # (keep most of the long outlines on the map)
            assert ref.vertex_margin(res, (ox, oy), poses, poly) > MARGIN
            want = ref.gate(cells, res, (ox, oy), poses, poly)
            got = s.footprint_gate(poly, poses=poses)
            assert got.tolist() == want.tolist()
            assert len(set(want.tolist())) >= 4
    # the long rectangle at yaw 0 has edges of 105 cells
    pts = ref.oriented((0.01, 0.01, 0.0), long_rect)
    a = ref.world_to_map(*pts[0], 200, 200, res, ox, oy)
    b = ref.world_to_map(*pts[1], 200, 200, res, ox, oy)
    assert len(ref.line_cells(*a, *b)) > 64


@pytest.mark.gpu
def test_order_cases_through_the_kernel():
    got = {}
    for name, marks, poly, want in HAND_CASES:
        with solver_on((hand_map(marks), 1.0, 0.0, 0.0)) as s:
            got[name] = s.footprint_gate(poly, poses=[(0.0, 0.0, 0.0)])[0]
        assert got[name] == want, name
    assert [got[c[0]] for c in HAND_CASES[:6]] == [255, 254, 254, 254, 254, 0]


def pool_inputs(count=256, maps=8, size=64, seed=7):
    rng = np.random.default_rng(seed)
    cells = np.stack([synthetic.make_costmap(size, seed=100 + k, n_discs=3)[0] for k in range(maps)])
    for k in range(maps):
        cells[k, 5 * k:5 * k + 6, 40:50] = 255           # distinct contents, unknown patches
    origins = rng.uniform(-20.0, 20.0, size=(maps, 2))
    idx = rng.integers(0, maps, size=count).astype(np.int32)
    ext = size * RES
    poses = np.concatenate([origins[idx] + rng.uniform(-0.3, ext + 0.3, size=(count, 2)),
                            rng.uniform(-math.pi, math.pi, size=(count, 1))], 1)
    return cells, origins, idx, poses


@pytest.mark.gpu
def test_pool_map_indices_problem_indices_and_rewritten_origins():
    import torch
    from neo_mpc_planner2_amd.solver import BatchSolver
    cells, origins, idx, poses = pool_inputs()
    assert ref.vertex_margin(RES, origins, poses, RECT, idx) > MARGIN
    want = ref.gate(cells, RES, origins, poses, RECT, idx)
    assert len(set(idx.tolist())) == 8 and (want == 255).any() and (want == 254).any() and (want < 254).any()
    probs = synthetic.make_problems(len(poses), 64, seed=1)
    probs["map_index"] = idx
    with BatchSolver({}) as s:
        s.set_costmap_pool(cells, RES, origins)
        assert s.footprint_gate(RECT, poses=poses, map_indices=idx).tolist() == want.tolist()
        # map_indices NULL: problems[i].map_index
        assert s.footprint_gate(RECT, poses=poses, problems=probs).tolist() == want.tolist()
        # an explicit index array wins over the records'
        probs2 = probs.copy()
        probs2["map_index"] = 0
        assert s.footprint_gate(RECT, poses=poses, problems=probs2, map_indices=idx).tolist() == want.tolist()
    # device pool: the origins live in the caller's tensor and may be rewritten between two gate calls
    shift = np.array([0.26, -0.31])
    assert ref.vertex_margin(RES, origins + shift, poses, RECT, idx) > MARGIN
    want2 = ref.gate(cells, RES, origins + shift, poses, RECT, idx)
    assert want2.tolist() != want.tolist()
    dev = "cuda:0"
    with BatchSolver({}) as s:
        d_origins = gpu(origins)
        s.set_costmap_pool(gpu(cells), RES, d_origins)
        d_fp, d_poses, d_idx = gpu(np.asarray(RECT, dtype=np.float64)), gpu(poses), gpu(idx)
        c1, c2 = torch.zeros(len(poses), dtype=torch.float64, device=dev), torch.zeros(len(poses), dtype=torch.float64, device=dev)
        s.footprint_gate_device(d_fp, c1, poses=d_poses, map_indices=d_idx)
        d_origins += gpu(shift)
        s.footprint_gate_device(d_fp, c2, poses=d_poses, map_indices=d_idx)
        torch.cuda.synchronize()
        assert c1.cpu().numpy().tolist() == want.tolist() and c2.cpu().numpy().tolist() == want2.tolist()


@pytest.mark.gpu
def test_per_robot_polygons():
    cells, res, ox, oy = random_map()
    poses, want = random_case("rect")
    rng = np.random.default_rng(5)
    # rows that differ: every robot its own rectangle
    half = rng.uniform(0.1, 0.6, size=(len(poses), 2))
    sign = np.array([(1, 1), (-1, 1), (-1, -1), (1, -1)], dtype=np.float64)
    own = half[:, None, :] * sign[None, :, :]
    assert ref.vertex_margin(res, (ox, oy), poses, own) > MARGIN
    want_own = ref.gate(cells, res, (ox, oy), poses, own)
    with solver_on(random_map()) as s:
        same = s.footprint_gate(np.broadcast_to(np.asarray(RECT), (len(poses), 4, 2)).copy(), poses=poses)
        assert same.tolist() == want.tolist() == s.footprint_gate(RECT, poses=poses).tolist()
        assert s.footprint_gate(own, poses=poses).tolist() == want_own.tolist()
    assert want_own.tolist() != want.tolist()


@pytest.mark.gpu
def test_oriented_polygons_and_problem_records():
    poses, want = random_case("rect")
    probs = synthetic.make_problems(len(poses), 200, seed=9)
    probs["cur_xy"] = poses[:, :2]
    probs["cur_q"] = synthetic.yaw_quat(poses[:, 2])
    probs["footprint_cost"] = 0.5
    before = probs.copy()
    # the pose comes from the records (poses NULL): cur_xy and the yaw of cur_q
    yaw = np.arctan2(2 * probs["cur_q"][:, 3] * probs["cur_q"][:, 2], 1 - 2 * probs["cur_q"][:, 2] ** 2)
    rec_poses = np.concatenate([probs["cur_xy"], yaw[:, None]], 1)
    cells, res, ox, oy = random_map()
    assert ref.vertex_margin(res, (ox, oy), rec_poses, RECT) > MARGIN
    want_rec = ref.gate(cells, res, (ox, oy), rec_poses, RECT)
    with solver_on(random_map()) as s:
        costs, polys = s.footprint_gate(RECT, problems=probs, want_polygons=True)
    assert costs.tolist() == want_rec.tolist()
    world = np.array([synthetic.footprint_world(row) for row in before])
    assert np.abs(polys - world).max() <= 1e-12
    assert (probs["footprint_cost"] == np.where(costs >= 254, 1.0, 0.0)).all() and (costs >= 254).any() and (costs < 254).any()
    after = probs.copy()
    after["footprint_cost"] = before["footprint_cost"]
    assert after.tobytes() == before.tobytes()            # nothing else in the records was touched


def chain_inputs(count=256):
    """Robots on the test-4 map with a plan each, passing by the robot."""
    poses = random_poses(count, seed=63)
    plan_poses, offsets, robots = synthetic.make_plans(count, seed=12, min_len=16, max_len=120)
    for i in range(count):
        plan_poses[offsets[i]:offsets[i + 1], :2] += poses[i, :2] - robots[i, :2]
    poses[:, 2] = robots[:, 2]
    probs = synthetic.make_problems(count, 200, seed=13)
    probs["cur_xy"] = poses[:, :2]
    probs["cur_q"] = synthetic.yaw_quat(poses[:, 2])
    return poses, plan_poses, offsets, probs


@pytest.mark.gpu
def test_gate_carrots_solve_chain_on_the_device():
    """K6 -> K4 -> K1 with no host copy between the steps, against the same chain fed from the host with the
    transcription's costs and synthetic.footprint_world polygons: bitwise the same commands, states and warm starts."""
    import torch
    from neo_mpc_planner2_amd.solver import DeviceBatch
    from oracle import mpc_oracle as orc
    count = 256
    cells, res, ox, oy = random_map()
    poses, plan_poses, offsets, probs = chain_inputs(count)
    yaw = np.arctan2(2 * probs["cur_q"][:, 3] * probs["cur_q"][:, 2], 1 - 2 * probs["cur_q"][:, 2] ** 2)
    rec_poses = np.concatenate([probs["cur_xy"], yaw[:, None]], 1)
    assert ref.vertex_margin(res, (ox, oy), rec_poses, RECT) > MARGIN
    want = ref.gate(cells, res, (ox, oy), rec_poses, RECT)
    assert (want == 255).any() and (want == 254).any() and ((want > 200) & (want < 254)).any()
    world = np.array([synthetic.footprint_world(row) for row in probs])
    st, warm = synthetic.make_states(probs, 3)
    slow = np.ones(count, dtype=np.int32)
    lp = abi.NeoMpcLookaheadParams(0.4, 0.8, 0.3, 1e9)
    dev = "cuda:0"
    results = []
    with solver_on(random_map(), orc.make_params()) as s:
        d_plans, d_off, d_rob = gpu(plan_poses), gpu(offsets.view(np.int32)), gpu(poses)
        for chain in ("device", "host-fed"):
            db = DeviceBatch(probs, st, warm, dev)
            d_slow = gpu(slow)
            d_car = torch.zeros((count, abi.CARROT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
            if chain == "device":
                d_costs = torch.zeros(count, dtype=torch.float64, device=dev)
                d_polys = torch.zeros((count, 4, 2), dtype=torch.float64, device=dev)
                s.footprint_gate_device(gpu(np.asarray(RECT, dtype=np.float64)), d_costs, problems=db.problems,
                                        footprints_out=d_polys)
            else:
                d_costs, d_polys = gpu(want), gpu(world)
            s.select_carrots_device(lp, d_plans, d_off, d_rob, d_slow, d_car, d_costs, problems=db.problems)
            s.solve_device(db.problems, db.states, db.warm, db.commands, footprints=d_polys)
            torch.cuda.synchronize()
            results.append((db.commands_host().copy(), db.states_host().copy(), db.warm.cpu().numpy(),
                            d_car.cpu().numpy().view(abi.CARROT_DTYPE).reshape(-1), d_costs.cpu().numpy(), d_slow.cpu().numpy()))
    (cm, sta, wa, car, costs, sl), (cm2, sta2, wa2, car2, _, sl2) = results
    assert costs.tolist() == want.tolist()
    thrown = want == 255
    assert (car["status"][thrown] == 3).all() and (car["status"][~thrown] == 0).all()
    assert (cm["flags"][thrown] == abi.FLAG_SKIPPED).all() and ((cm["flags"][~thrown] & abi.FLAG_SKIPPED) == 0).all()
    assert cm.tobytes() == cm2.tobytes() and sta.tobytes() == sta2.tobytes() and wa.tobytes() == wa2.tobytes()
    assert car.tobytes() == car2.tobytes() and sl.tolist() == sl2.tolist()
    assert ((cm["flags"] & abi.FLAG_STOPPED) != 0).any()      # the py:343 latch saw lethal outlines


@pytest.mark.gpu
def test_gates_are_ordered_against_costmap_ingests():
    """set_costmap(A), gate, set_costmap(B), gate, back to back on a stream of the caller's: each gate sees its own map."""
    import torch
    cells, res, ox, oy = random_map()
    other = np.ascontiguousarray(cells[::-1, ::-1])
    poses, want_a = random_case("rect")
    want_b = ref.gate(other, res, (ox, oy), poses, RECT)
    assert want_a.tolist() != want_b.tolist()
    dev = "cuda:0"
    from neo_mpc_planner2_amd.solver import BatchSolver
    with BatchSolver({}) as s:
        d_fp, d_poses = gpu(np.asarray(RECT, dtype=np.float64)), gpu(poses)
        ca, cb = torch.zeros(len(poses), dtype=torch.float64, device=dev), torch.zeros(len(poses), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            s.set_costmap(cells, res, ox, oy)
            s.footprint_gate_device(d_fp, ca, poses=d_poses)
            s.set_costmap(other, res, ox, oy)
            s.footprint_gate_device(d_fp, cb, poses=d_poses)
        torch.cuda.synchronize()
    assert ca.cpu().numpy().tolist() == want_a.tolist() and cb.cpu().numpy().tolist() == want_b.tolist()


@pytest.mark.gpu
def test_refusals():
    from neo_mpc_planner2_amd.solver import BatchSolver
    poses = np.array([(0.0, 0.0, 0.0), (1.0, 1.0, 0.5)])
    with BatchSolver({}) as s:
        with pytest.raises(_lib.NeoMpcError) as e:        # before any costmap
            s.footprint_gate(RECT, poses=poses)
        assert e.value.code == -4                         # NEO_MPC_ERR_NO_COSTMAP
        s.set_costmap(*random_map())
        for bad in (RECT[:2], GON16 + ((0.0, 0.0),)):     # 2 and 17 points
            with pytest.raises(_lib.NeoMpcError) as e:
                s.footprint_gate(bad, poses=poses)
            assert e.value.code == -1 and "footprint_points" in str(e.value)
        nan_pose = poses.copy()
        nan_pose[1, 2] = np.nan
        with pytest.raises(_lib.NeoMpcError) as e:
            s.footprint_gate(RECT, poses=nan_pose)
        assert e.value.code == -1 and "not finite" in str(e.value)
        b = abi.NeoMpcFootprintBatch()                    # null required pointers
        b.count, b.footprint_points = 2, 4
        assert s._lib.neo_mpc_footprint_gate(s._handle, C.byref(b)) == -1
        assert s._lib.neo_mpc_footprint_gate_device(s._handle, C.byref(b), None) == -1
        assert s.footprint_gate(RECT, poses=np.zeros((0, 3))).shape == (0,)     # count = 0: OK, nothing launched
        cells, origins, idx, pool_poses = pool_inputs(count=8)
        s.set_costmap_pool(cells, RES, origins)
        for wrong in (8, -1):
            bad_idx = idx.copy()
            bad_idx[3] = wrong
            with pytest.raises(_lib.NeoMpcError) as e:
                s.footprint_gate(RECT, poses=pool_poses, map_indices=bad_idx)
            assert e.value.code == -1 and "map index" in str(e.value)
        assert s.footprint_gate(RECT, poses=pool_poses, map_indices=idx).shape == (8,)


@pytest.mark.gpu
def test_closed_loop_with_the_gate():
    """fleet.closed_loop(footprint=RECT_FOOTPRINT): robots whose outline lies on a lethal cell are stopped on tick 0 by the
    py:343 latch; footprint=None is the loop every caller had -- bitwise."""
    from neo_mpc_planner2_amd import fleet
    from neo_mpc_planner2_amd.solver import DeviceBatch
    from oracle import mpc_oracle as orc
    cfg, cmap, probs, st, warm = synthetic.make_workload("C2", seed=0, batch=256)
    cells, res, ox, oy = cmap
    ys, xs = np.nonzero(cells == 254)
    placed = np.arange(0, 256, 16)
    for k, i in enumerate(placed):       # vertex 0 of the outline at the centre of a lethal cell, yaw 0
        j = (k * 997) % len(xs)
        centre = np.array([ox + (xs[j] + 0.5) * res, oy + (ys[j] + 0.5) * res])
        probs["cur_xy"][i] = centre - np.asarray(RECT[0])
        probs["cur_q"][i] = (0.0, 0.0, 0.0, 1.0)
    runs = {}
    with solver_on(cmap, orc.make_params()) as s:
        for tag, kw in (("plain", {}), ("none", dict(footprint=None)), ("gate", dict(footprint=RECT))):
            ticks = []
            db = DeviceBatch(probs, st, warm, "cuda:0")
            out = fleet.closed_loop(s, db, 5, after_tick=lambda t, cm: ticks.append(cm.copy()), **kw)
            runs[tag] = (ticks, out)
    assert len(runs["gate"][0]) == 5
    for a, b in zip(runs["plain"][0], runs["none"][0]):
        assert a.tobytes() == b.tobytes()
    assert "footprint_lethal_fraction" not in runs["none"][1] and len(runs["gate"][1]["footprint_lethal_fraction"]) == 5
    first = runs["gate"][0][0]
    assert ((first["flags"][placed] & abi.FLAG_STOPPED) != 0).all() and (first["vel"][placed] == 0.0).all()
    assert runs["gate"][1]["footprint_lethal_fraction"][0] >= len(placed) / 256.0
