"""The rolling windows (K7): a fleet's local costmaps cut from one world map on the device -- roll -> gate -> carrots -> solve.

nav2 cannot be built here, so the contract is the text in include/neo_mpc.h (neo_mpc_window_batch) and its executable form
the per-cell transcription in tests/rolling_window_reference.py.  Only + - * / on float64 are involved and they round
identically on both sides, so every comparison with the transcription is exact equality of uint8 cells and float64
origins: no tolerance, no dropped case, no condition on the inputs."""
import ctypes as C
import functools

import numpy as np
import pytest

from neo_mpc_planner2_amd import _lib, abi, synthetic
from tests import rolling_window_reference as ref
from tests.c_probe import check_entry_points, check_layout, probe_header
from tests.fleet_kit import RECT, Side, capture_fleet, gpu, replay_against_direct

WRES = synthetic.RESOLUTION
WOX, WOY = -1.0, -1.5
ENTRY_POINTS = ("neo_mpc_set_world_map", "neo_mpc_set_world_map_device", "neo_mpc_roll_costmap_pool",
                "neo_mpc_roll_costmap_pool_device", "neo_mpc_get_costmap_pool")


# ------------------------------------------------------------------------------------------ 1: the hand-worked map
def test_transcription_on_a_hand_worked_map():
    world = np.array([[10 * my + mx for mx in range(8)] for my in range(6)], dtype=np.uint8)
    o = (0.0, 0.0)

    def step(pose):
        origins, cells = ref.roll(world, 1.0, -2.0, -1.0, [o], 5, 4, 1.0, poses=[pose], outside_value=255)
        return tuple(origins[0]), cells[0].tolist()

    run = lambda a: list(range(a, a + 5))
    blank = [255] * 5
    o, cells = step((2.25, 1.75))
    assert o == (0.0, 0.0) and cells == [run(12), run(22), run(32), run(42)]
    o, cells = step((2.9, 1.75))          # a sub-cell move does not roll
    assert o == (0.0, 0.0) and cells == [run(12), run(22), run(32), run(42)]
    o, cells = step((3.3, 1.75))
    assert o == (1.0, 0.0) and cells == [run(13), run(23), run(33), run(43)]
    o, cells = step((0.1, -2.0))          # shifts (-3, -3): -3.75 truncates toward zero
    assert o == (-2.0, -3.0) and cells == [blank, blank, run(0), run(10)]
    o, cells = step((0.1, -2.9))
    assert o == (-2.0, -4.0) and cells == [blank, blank, blank, run(0)]
    o, cells = step((7.0, 5.0))
    assert o == (4.0, 3.0) and cells == [[46, 47, 255, 255, 255], [56, 57, 255, 255, 255], blank, blank]
    # the conversion's guard: a quotient that is not finite, or beyond 2^31, moves nothing
    assert ref.move_axis(float("nan"), 1.0, 5, 1.0) == 1.0 and ref.move_axis(1e12, 1.0, 5, 1.0) == 1.0
    # worldToMap refuses below the origin (no truncation into cell 0) and from the far edge on
    assert ref.world_cell(-2.5, -2.0, 1.0, 8) is None and ref.world_cell(-1.5, -2.0, 1.0, 8) == 0
    assert ref.world_cell(5.999, -2.0, 1.0, 8) == 7 and ref.world_cell(6.0, -2.0, 1.0, 8) is None


# ------------------------------------------------------------------------------------------ 2: record and entry points
def test_window_batch_layout_and_entry_points(tmp_path):
    got = probe_header(tmp_path, ["neo_mpc_window_batch"], entry_points=ENTRY_POINTS)
    check_layout(got, "neo_mpc_window_batch", 56, struct=abi.NeoMpcWindowBatch)
    assert len(ENTRY_POINTS) == 5
    check_entry_points(ENTRY_POINTS)


# ------------------------------------------------------------------------------------------ shared GPU inputs
@functools.lru_cache(maxsize=None)
def random_world():
    """50 x 70 random cells over every value 0 .. 255, origin (-1.0, -1.5)."""
    world = np.random.default_rng(23).integers(0, 256, size=(70, 50)).astype(np.uint8)
    world.setflags(write=False)
    return world


#: window resolution and where the window lattice sits: "half" = res = wres, half a cell off the world's lattice -- where a
#: fused ox + (i + 0.5) * res lands in another world cell; the others carry an offset that is no multiple of anything
RESOLUTIONS = {"equal": WRES, "finer": WRES / 2, "coarser": 2 * WRES, "half": WRES}
SIZES = {"13x11": (13, 11), "36x20": (36, 20), "200x200": (200, 200)}


def placements(size_x, size_y, res, case):
    """Window origins: over each of the four world edges, over a corner, wholly outside, inside (wholly, where the window
    fits).  The 200 x 200 windows (whose last eight columns share a 16-byte chunk with the pitch padding) come in three:
    the world flush in their top right corner -- world cells in that chunk --, over the world's corner, and outside."""
    w, h, wx, wy = size_x * res, size_y * res, 50 * WRES, 70 * WRES
    if case == "half":
        snap = lambda v, o: o + (round((v - o) / WRES) + 0.5) * WRES
    else:
        snap = lambda v, o: v + 0.0137
    cx, cy = WOX + wx / 2 - w / 2, WOY + wy / 2 - h / 2
    at = {"left": (WOX - w / 2, cy), "right": (WOX + wx - w / 2, cy), "bottom": (cx, WOY - h / 2),
          "top": (cx, WOY + wy - h / 2), "corner": (WOX + wx - w / 2, WOY + wy - h / 2),
          "outside": (WOX + wx + 1.0, WOY - h - 1.0), "inside": (cx, cy)}
    if size_x == 200:
        at["flush"] = (WOX + wx - w, WOY + wy - h)
    names = ("flush", "corner", "outside") if size_x == 200 else tuple(at)
    return names, np.array([(snap(at[n][0], WOX), snap(at[n][1], WOY)) for n in names])


@functools.lru_cache(maxsize=None)
def fill_case(size, case):
    """(names, origins, transcription's cells with -1 for an outside cell) of test 3; computed once, never written."""
    size_x, size_y = SIZES[size]
    res = RESOLUTIONS[case]
    names, origins = placements(size_x, size_y, res, case)
    want = np.stack([ref.fill_window(random_world(), WRES, WOX, WOY, o, size_x, size_y, res, -1, dtype=np.int16)
                     for o in origins])
    origins.setflags(write=False)
    want.setflags(write=False)
    return names, origins, want


def solver_with_world(params=None, world=None):
    from neo_mpc_planner2_amd.solver import BatchSolver
    s = BatchSolver(params or {})
    s.set_world_map(random_world() if world is None else world, WRES, WOX, WOY)
    return s


# ------------------------------------------------------------------------------------------ 3: the fill
@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(RESOLUTIONS))
@pytest.mark.parametrize("size", sorted(SIZES))
def test_fill_equals_the_transcription(size, case):
    size_x, size_y = SIZES[size]
    names, origins, want = fill_case(size, case)
    outside = want < 0
    per_window = dict(zip(names, outside.reshape(len(names), -1).mean(axis=1)))
    # the placements are what they say: cut by the world's edge, wholly outside, wholly inside where the window fits
    assert per_window["outside"] == 1.0 and 0.0 < per_window["corner"] < 1.0
    if size_x * RESOLUTIONS[case] < 50 * WRES and size_y * RESOLUTIONS[case] < 70 * WRES:
        assert per_window["inside"] == 0.0
        assert all(0.0 < per_window[n] < 1.0 for n in names if n not in ("inside", "outside"))
    with solver_with_world() as s:
        for value in (0, 7, 255):
            o = origins.copy()
            s.roll_costmap_pool(size_x, size_y, RESOLUTIONS[case], o, outside_value=value)
            cells, back = s.get_costmap_pool()
            assert o.tolist() == origins.tolist() == back.tolist()          # no pose: the windows stay
            assert cells.dtype == np.uint8 and cells.shape == want.shape
            assert np.array_equal(cells, np.where(outside, value, want).astype(np.uint8)), (size, case, value)


def test_the_half_cell_case_is_the_contraction_case():
    """What test 3's "half" placements are for: with res = wres and the window lattice half a cell off the world's, every
    cell centre sits on a world cell's edge, and o + (i + 0.5) * res evaluated as ONE fused operation lands in another world
    cell than the contract's two roundings for a good share of the columns and rows (exact rational arithmetic stands in
    for the fma)."""
    from fractions import Fraction
    for size in ("36x20", "200x200"):
        _, origins, _ = fill_case(size, "half")
        inside = differ = 0
        for ox, oy in origins:
            for o, n, wo, ws in ((float(ox), SIZES[size][0], WOX, 50), (float(oy), SIZES[size][1], WOY, 70)):
                for i in range(n):
                    two = o + (i + 0.5) * WRES
                    fused = float(Fraction(o) + Fraction(i + 0.5) * Fraction(WRES))      # one rounding
                    a, b = ref.world_cell(two, wo, WRES, ws), ref.world_cell(fused, wo, WRES, ws)
                    inside += a is not None
                    differ += a != b
        assert differ >= 0.05 * inside and inside >= 200, (size, differ, inside)


# ------------------------------------------------------------------------------------------ 4: origins as state
#: per-tick moves of the robots in cells (x, y): +-0.4 cell, +-1.6 cells, a jump of 30 cells, back across zero
MOVES = ((0.4, -0.4), (-0.4, 0.4), (1.6, -1.6), (-1.6, 1.6), (30.0, -30.0), (-47.3, 52.9))
SX4, SY4 = 36, 20


@functools.lru_cache(maxsize=None)
def state_case():
    """Eight windows, six ticks: (start origins, poses per tick, the transcription's origins and cells per tick)."""
    rng = np.random.default_rng(29)
    start = np.stack([rng.uniform(-1.6, 0.4, size=8), rng.uniform(-1.9, 1.0, size=8)], 1)
    centre = start + np.array([(SX4 - 0.5) * WRES / 2, (SY4 - 0.5) * WRES / 2]) + rng.uniform(-0.02, 0.02, size=(8, 2))
    sign = np.where(np.arange(8)[:, None] % 2 == 0, 1.0, -1.0)
    poses, origins, cells = [], [], []
    o, p = start, centre
    for move in MOVES:
        p = p + sign * np.array(move) * WRES
        o, c = ref.roll(random_world(), WRES, WOX, WOY, o, SX4, SY4, WRES, poses=p, outside_value=9)
        poses.append(np.concatenate([p, rng.uniform(-3, 3, size=(8, 1))], 1))
        origins.append(o)
        cells.append(c)
    for a in poses + origins + cells:
        a.setflags(write=False)
    moved = np.array(origins) - np.array([start] + origins[:-1])
    assert (moved[0] == 0).all() or (moved[1] == 0).all()         # a sub-cell move leaves origins alone
    assert (np.abs(moved[4]) > 1.0).all() and (np.array(origins[-1]) * np.array(origins[-2]) < 0).any()
    return start, poses, origins, cells


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["host", "device", "host-problems", "device-problems"])
def test_origins_are_state(variant):
    import torch
    start, poses, want_o, want_c = state_case()
    dev = "cuda:0"
    with solver_with_world() as s:
        o = start.copy() if variant.startswith("host") else torch.from_numpy(start.copy()).to(dev)
        for t in range(len(MOVES)):
            kw = {}
            if variant.endswith("problems"):
                probs = synthetic.make_problems(8, 200, seed=t)
                probs["cur_xy"] = poses[t][:, :2]
                kw["problems"] = probs if variant.startswith("host") else \
                    torch.from_numpy(probs.view(np.uint8).reshape(8, -1)).to(dev)
            else:
                kw["poses"] = poses[t].copy() if variant.startswith("host") else torch.from_numpy(poses[t].copy()).to(dev)
            s.roll_costmap_pool(SX4, SY4, WRES, o, outside_value=9, **kw)
            cells, back = s.get_costmap_pool()
            now = o if variant.startswith("host") else o.cpu().numpy()
            assert now.tolist() == want_o[t].tolist() == back.tolist(), (variant, t)
            assert np.array_equal(cells, want_c[t]), (variant, t)
        # the world map changed, no pose: origins stay, the cells are the new world's
        other = np.ascontiguousarray(random_world()[::-1, ::-1])
        s.set_world_map(other if variant.startswith("host") else torch.from_numpy(other).to(dev), WRES, WOX, WOY)
        s.roll_costmap_pool(SX4, SY4, WRES, o, outside_value=9)
        cells, back = s.get_costmap_pool()
        _, want = ref.roll(other, WRES, WOX, WOY, want_o[-1], SX4, SY4, WRES, outside_value=9)
        assert back.tolist() == want_o[-1].tolist() and np.array_equal(cells, want)
        assert not np.array_equal(cells, want_c[-1])


# ------------------------------------------------------------------------------------------ 5: a solve cannot tell
@pytest.mark.gpu
def test_a_solve_and_a_gate_cannot_tell_a_rolled_pool_from_an_ingested_one():
    """Geometry and requests of test_costmap_pool_each_instance_reads_its_own_map (eight windows of 160 x 160 cells, 768
    requests spread over them), the windows cut from one 600 x 600 world: against the transcription's raw windows passed
    through neo_mpc_set_costmap_pool_device with the rolled origins, commands, states, warm starts and gate costs are
    bit-identical -- border, pitch, pool_count and the derived constants are those of an ingested pool."""
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
    start = offsets - 4.3                                   # anywhere: the roll moves the windows to their centres
    want_o, raw = ref.roll(world, res, wox, woy, start, size, size, res, poses=offsets, outside_value=255)
    fp = gpu(np.asarray(RECT, dtype=np.float64))
    results = []
    for how in ("rolled", "ingested"):
        with BatchSolver(orc.make_params()) as s:
            if how == "rolled":
                s.set_world_map(gpu(world), res, wox, woy)
                d_orig = gpu(start)
                s.roll_costmap_pool(size, size, res, d_orig, poses=gpu(np.concatenate([offsets, np.zeros((m, 1))], 1)))
            else:
                d_orig = gpu(want_o)
                s.set_costmap_pool(gpu(raw), res, d_orig)
            b = DeviceBatch(probs, st, warm, "cuda:0")
            costs = torch.zeros(count, dtype=torch.float64, device="cuda:0")
            s.footprint_gate_device(fp, costs, problems=b.problems)
            s.solve_device(b.problems, b.states, b.warm, b.commands, solution=b.solution)
            torch.cuda.synchronize()
            cells, back = s.get_costmap_pool()
            results.append((b.commands_host().copy(), b.states_host().copy(), b.warm.cpu().numpy(), costs.cpu().numpy(),
                            cells, back, s.kernel_info()))
    a, b = results
    assert a[5].tolist() == want_o.tolist() == b[5].tolist() and np.array_equal(a[4], raw) and np.array_equal(b[4], raw)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    assert a[3].tobytes() == b[3].tobytes() and a[6] == b[6]
    # the inputs exercise it: gates on lethal and on free cells, searches next to walls and in the open
    assert (a[3] >= 254).any() and (a[3] == 0).any()
    assert ((a[0]["flags"] & abi.FLAG_WALL_IN_REACH) != 0).any() and ((a[0]["flags"] & abi.FLAG_WALL_IN_REACH) == 0).any()


# ------------------------------------------------------------------------------------------ 6: read-back
@pytest.mark.gpu
def test_get_costmap_pool_round_trips_set_costmap_pool_and_set_costmap():
    import torch
    from neo_mpc_planner2_amd.solver import BatchSolver
    rng = np.random.default_rng(31)
    with BatchSolver({}) as s:
        with pytest.raises(_lib.NeoMpcError) as e:
            s._map_shape = (1, 4, 4)
            s.get_costmap_pool()
        assert e.value.code == -4                          # NEO_MPC_ERR_NO_COSTMAP
        for shape in ((5, 11, 13), (3, 20, 36), (2, 200, 200)):
            cells = rng.integers(0, 256, size=shape).astype(np.uint8)
            origins = rng.uniform(-9, 9, size=(shape[0], 2))
            for device in (False, True):
                if device:
                    d_o = torch.from_numpy(origins).to("cuda:0")
                    s.set_costmap_pool(torch.from_numpy(cells).to("cuda:0"), 0.05, d_o)
                else:
                    s.set_costmap_pool(cells, 0.05, origins)
                got, back = s.get_costmap_pool()
                assert np.array_equal(got, cells) and back.tolist() == origins.tolist()
                got, back = s.get_costmap_pool(1, shape[0] - 1)
                assert np.array_equal(got, cells[1:]) and back.tolist() == origins[1:].tolist()
            with pytest.raises(_lib.NeoMpcError) as e:
                s.get_costmap_pool(1, shape[0])
            assert e.value.code == -1
        single = rng.integers(0, 256, size=(37, 53)).astype(np.uint8)
        s.set_costmap(single, 0.05, -1.25, 2.5)
        got, back = s.get_costmap_pool()
        assert np.array_equal(got[0], single) and back.tolist() == [[-1.25, 2.5]]


# ------------------------------------------------------------------------------------------ 7: refusals
@pytest.mark.gpu
def test_refusals_leave_the_costmap_alone():
    from neo_mpc_planner2_amd.solver import BatchSolver
    origins = np.array([(0.0, 0.0), (0.5, -0.5)])
    poses = np.array([(0.1, 0.2, 0.0), (0.3, 0.4, 1.0)])
    held = np.random.default_rng(37).integers(0, 256, size=(2, 9, 12)).astype(np.uint8)
    held_origins = np.array([(1.0, 2.0), (3.0, 4.0)])
    with BatchSolver({}) as s:
        s.set_costmap_pool(held, 0.05, held_origins)
        with pytest.raises(_lib.NeoMpcError) as e:        # before any world map
            s.roll_costmap_pool(13, 11, WRES, origins.copy(), poses=poses)
        assert e.value.code == -4                         # NEO_MPC_ERR_NO_COSTMAP
        for bad in (dict(size_x=0), dict(size_y=0), dict(resolution=0.0), dict(resolution=-0.05)):   # world geometry
            kw = dict(size_x=50, size_y=70, resolution=WRES)
            kw.update(bad)
            w = np.zeros((max(kw["size_y"], 1), max(kw["size_x"], 1)), dtype=np.uint8)
            assert s._lib.neo_mpc_set_world_map(s._handle, C.c_void_p(w.ctypes.data), kw["size_x"], kw["size_y"],
                                                kw["resolution"], WOX, WOY) == -1
        assert s._lib.neo_mpc_set_world_map(s._handle, None, 50, 70, WRES, WOX, WOY) == -1
        s.set_world_map(random_world(), WRES, WOX, WOY)

        def call(device=False, **over):
            o = origins.copy()
            b = abi.NeoMpcWindowBatch()
            b.count, b.size_x, b.size_y, b.resolution = 2, 13, 11, WRES
            b.poses, b.origins, b.outside_value = poses.ctypes.data, o.ctypes.data, 255
            for k, v in over.items():
                setattr(b, k, v)
            if device:
                return s._lib.neo_mpc_roll_costmap_pool_device(s._handle, C.byref(b), None)
            return s._lib.neo_mpc_roll_costmap_pool(s._handle, C.byref(b))

        nan_pose, inf_origin = poses.copy(), origins.copy()
        nan_pose[1, 0] = np.nan
        inf_origin[0, 1] = np.inf
        probs = synthetic.make_problems(2, 200, seed=1)
        probs["cur_xy"][0, 1] = np.nan
        refused = (dict(origins=None), dict(count=65536), dict(size_x=0), dict(size_y=0), dict(resolution=0.0),
                   dict(resolution=-0.05), dict(resolution=float("nan")), dict(resolution=float("inf")),
                   dict(outside_value=256), dict(reserved=1), dict(poses=nan_pose.ctypes.data),
                   dict(origins=inf_origin.ctypes.data), dict(poses=None, problems=probs.ctypes.data))
        for over in refused:
            assert call(**over) == -1, over
            assert s._lib.neo_mpc_last_error_code() == -1
        for over in refused[:10]:                         # the device variant checks the record's shape alone
            assert call(device=True, **over) == -1, over
        assert call(count=0) == 0 and call(device=True, count=0) == 0      # nothing to do: OK, nothing launched
        got, back = s.get_costmap_pool()                  # every refused call left the handle's costmap as it was
        assert np.array_equal(got, held) and back.tolist() == held_origins.tolist()
        assert call() == 0
        assert s._lib.neo_mpc_get_costmap_pool(s._handle, 0, 3, None, None) == -1


# ------------------------------------------------------------------------------------------ 8: graph capture
@pytest.mark.gpu
def test_roll_gate_solve_can_be_captured_in_a_hip_graph():
    """A roll with the geometry, count and origins of the previous one allocates nothing and does not synchronise: after one
    warm-up call, roll -> gate -> solve is captured on one stream and replayed with the poses rewritten in between; the
    replays equal the same calls made directly (on a second handle: same world, same inputs)."""
    f = capture_fleet(260)
    rng = np.random.default_rng(93)
    ticks = [(np.concatenate([f.probs["cur_xy"] + rng.uniform(-0.4, 0.4, size=(f.count, 2)) * k, np.zeros((f.count, 1))], 1),)
             for k in range(3)]
    fp = gpu(np.asarray(RECT, dtype=np.float64))

    class RollSide(Side):
        def tick(self):
            self.s.roll_costmap_pool(f.sx, f.sy, f.res, self.origins, poses=self.poses)
            self.s.footprint_gate_device(fp, self.costs, poses=self.poses, problems=self.b.problems)
            self.s.solve_device(self.b.problems, self.b.states, self.b.warm, self.b.commands, solution=self.b.solution)

    with replay_against_direct(lambda: RollSide(f, ticks[0]), ticks, changed=(3,)) as (direct, a, _):     # the windows moved
        want_o = f.start
        for poses, in ticks:                                     # the warm-up call, then the two replays
            want_o, _ = ref.roll(f.world, f.res, f.wox, f.woy, want_o, f.sx, f.sy, f.res, poses=poses, fill=False)
        assert a[3] == want_o.tolist()
        _, want_c = ref.roll(f.world, f.res, f.wox, f.woy, want_o, f.sx, f.sy, f.res)
        assert np.array_equal(direct.s.get_costmap_pool()[0], want_c)


# ------------------------------------------------------------------------------------------ 9: the closed loop
@pytest.mark.gpu
def test_closed_loop_rolls_the_windows_with_the_robots():
    """fleet.closed_loop(rolling=...): ten ticks of 64 robots through one fixed world, window i following robot i; the final
    windows are the transcription's, run tick by tick at the loop's own poses."""
    import torch
    from neo_mpc_planner2_amd import fleet
    from neo_mpc_planner2_amd.solver import BatchSolver, DeviceBatch
    from oracle import mpc_oracle as orc
    count, sx, sy, ticks = 64, 48, 44, 10
    world, res, wox, woy = synthetic.make_costmap(300, seed=95)
    probs = synthetic.make_problems(count, 300, seed=96)
    probs["map_index"] = np.arange(count, dtype=np.int32)
    st, warm = synthetic.make_states(probs, 3)
    start = probs["cur_xy"] - np.array([sx * res / 2, sy * res / 2]) + 0.013
    seen = []
    with BatchSolver(orc.make_params()) as s:
        s.set_world_map(world, res, wox, woy)
        d_orig = torch.from_numpy(start.copy()).to("cuda:0")
        b = DeviceBatch(probs, st, warm, "cuda:0")
        out = fleet.closed_loop(s, b, ticks, before_tick=lambda t, pos: seen.append(pos.cpu().numpy().copy()),
                                rolling=(sx, sy, res, d_orig))
        torch.cuda.synchronize()
        cells, back = s.get_costmap_pool()
        got_o = d_orig.cpu().numpy()
    assert len(seen) == ticks and len(out["kernel_ms"]) == ticks
    want_o = start
    for t in range(ticks):
        want_o, want_c = ref.roll(world, res, wox, woy, want_o, sx, sy, res, poses=seen[t], fill=t == ticks - 1)
    assert got_o.tolist() == want_o.tolist() == back.tolist()
    assert np.array_equal(cells, want_c)
    assert (np.abs(seen[-1] - seen[0]).max(axis=1) > res).any() and (want_o != start).any()    # robots and windows moved
    assert (cells == 254).any() and (cells == 0).any()
