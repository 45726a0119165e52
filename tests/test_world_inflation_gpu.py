"""The world inflation (K9) on the GPU: neo_mpc_inflate_world_map[_device] and neo_mpc_get_world_map against the
transcription of tests/world_inflation_reference.py -- exact equality of uint8 cells, no tolerance, no dropped case -- and
the call's place in the chain: set -> inflate -> roll, its refusals, a HIP graph on one stream, its order against a roll
on another stream (the delay and its validity conditions are those of tests/test_stream_ordering.py, imported), and K9 and
the fleet stamp (K8) on one handle, each with a cost table of its own that changes between the calls."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import fleet_stamp_reference as stamp_ref
from tests import footprint_gate_reference as gate_ref
from tests import rolling_window_reference as roll_ref
from tests import test_stream_ordering as so          # helpers only: the module object holds its tests, this one collects none
from tests import test_world_inflation as cpu
from tests import world_inflation_reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PARAMS = (0.45, 0.9, 3.0)            # inscribed_radius, inflation_radius, cost_scaling_factor: R = 18 at 5 cm
GEOMETRY = (-1.25, 2.5)              # the world's origin (the resolution is the case's)
rig = so.rig                         # the fixture: one handle and its arrays, closed behind the test


@functools.lru_cache(maxsize=None)
def seam_map():
    """200 x 150 cells, built to cross the seams of 64 x 64 tiles: lone seeds at columns 63 and 64 and at rows 63 and 64, a
    seed in each corner, a full row of seeds on the last row, and a 40 x 40 block of unknown cells astride the seams at column
    64 and row 128 whose top edge lies four rows below the lone seed of column 64 and whose bottom edge six rows above the
    last row: inside the inscribed radius of both at R = 18 and 12, so the block takes 253 on either side of the seam and
    refuses the ring's lower costs further in."""
    cells = np.zeros((150, 200), dtype=np.uint8)
    cells[104:144, 40:80] = 255
    cells[30, 63] = cells[100, 64] = 254
    cells[63, 120] = cells[64, 180] = 254
    for l, i in ((0, 0), (0, 199), (149, 0), (149, 199)):
        cells[l, i] = 254
    cells[149, :] = 254
    assert cells[30, 63] == cells[100, 64] == cells[63, 120] == cells[64, 180] == 254
    assert (cells[:149, 64] == 254).sum() == 1 and (cells[:149, 63] == 254).sum() == 1         # lone: one seed above the last row
    assert (cells[104:144, 40:80] == 255).all()
    cells.setflags(write=False)
    return cells


def all_cases():
    out = list(cpu.cases())
    for res, params in cpu.PARAMETER_SETS:
        want = ref.inflate_world(seam_map(), res, *params)
        reach = ref.table_for(res, *params)[1]
        block = want[104:144, 40:80]
        if reach in (12, 18):
            # the unknown block takes 253 from the lone seed of column 64 on both sides of the column seam and from the last
            # row below the row seam, and refuses everything lower: nothing in it is anything but 253 or 255
            assert (block[:8, :24] == 253).any() and (block[:8, 24:] == 253).any() and (block[128 - 104:] == 253).any()
            assert (block == 255).any() and np.isin(block, (253, 255)).all()
            assert (want[100, 64 - reach:64] > 0).all() and (want[30, 64:64 + reach] > 0).all()      # rings across the seam
        out.append(("seams-R%d" % reach, seam_map(), res, params, want))
    return out


def solver(params=None):
    from neo_mpc_planner2_amd.solver import BatchSolver
    return BatchSolver(params or {})


# ------------------------------------------------------------------------------------------ 5: against the transcription
def test_host_and_device_variants_equal_the_transcription():
    import torch
    changed = 0
    with solver() as s:
        for name, cells, res, params, want in all_cases():
            for where in ("host", "device"):
                raw = np.array(cells) if where == "host" else torch.from_numpy(np.array(cells)).to(DEV)
                s.set_world_map(raw, res, *GEOMETRY)
                back = s.get_world_map()
                assert np.array_equal(back[0], cells) and back[1:] == (res,) + GEOMETRY, (name, where)
                s.inflate_world_map(*params)
                got = s.get_world_map()
                assert got[1:] == (res,) + GEOMETRY, (name, where)                 # the geometry comes back as set
                assert got[0].shape == cells.shape
                assert np.array_equal(got[0], want), (name, where, int((got[0] != want).sum()))
                s.inflate_world_map(*params)                                       # a second call changes nothing
                assert np.array_equal(s.get_world_map()[0], want), (name, where, "second call")
            changed += int((want != cells).any())
    print("%d of %d cases change a cell" % (changed, len(all_cases())))
    assert changed >= 12 + 3


# ------------------------------------------------------------------------------------------ 6: the chain
def test_a_roll_cuts_its_windows_from_the_inflated_world():
    name, world, res, _, _ = cpu.cases()[-4]                   # 130 x 75 cells at 5 cm, 3 % seeds
    assert world.shape == (75, 130) and res == 0.05
    inflated = ref.inflate_world(world, res, *PARAMS)
    assert (inflated != world).any()
    wox, woy = GEOMETRY
    # three windows of 36 x 20 cells: two inside the world, one astride its right edge
    poses = np.array([(wox + 1.7, woy + 1.1, 0.0), (wox + 3.9, woy + 2.6, 1.0), (wox + 6.4, woy + 1.9, -2.0)])
    start = poses[:, :2] - (0.9, 0.5) + 0.013
    with solver() as s:
        s.set_world_map(np.array(world), res, wox, woy)
        origins = start.copy()
        s.roll_costmap_pool(36, 20, 0.05, origins, poses=poses)
        want_origins, want_raw = roll_ref.roll(world, res, wox, woy, start, 36, 20, 0.05, poses=poses, outside_value=255)
        got, back = s.get_costmap_pool()
        assert back.tolist() == want_origins.tolist() == origins.tolist()
        assert np.array_equal(got, want_raw)                   # the roll before the inflation: the raw world
        assert (want_raw[2] == 255).any() and (want_raw[2] != 255).any()          # astride the edge
        s.inflate_world_map(*PARAMS)
        got, _ = s.get_costmap_pool()
        assert np.array_equal(got, want_raw)                   # the inflation touches nothing but the world copy
        s.roll_costmap_pool(36, 20, 0.05, origins, poses=poses)
        again, want = roll_ref.roll(inflated, res, wox, woy, want_origins, 36, 20, 0.05, poses=poses, outside_value=255)
        got, back = s.get_costmap_pool()
        assert back.tolist() == again.tolist()
        assert np.array_equal(got, want) and (want != want_raw).any()


# ------------------------------------------------------------------------------------------ 7: refusals
def test_refusals_leave_the_world_map_alone():
    held = np.array(cpu.cases()[8][1])                         # 70 x 67 cells
    with solver() as s:
        lib, h = s._lib, s._handle
        size = C.c_uint32(7)
        assert lib.neo_mpc_inflate_world_map(h, *PARAMS) == -4 and lib.neo_mpc_last_error_code() == -4      # NEO_MPC_ERR_NO_COSTMAP
        assert lib.neo_mpc_inflate_world_map_device(h, *PARAMS, None) == -4
        assert lib.neo_mpc_get_world_map(h, None, C.byref(size), None, None, None, None) == -4 and size.value == 7
        s.set_world_map(held, 0.05, *GEOMETRY)

        def untouched():
            got = s.get_world_map()
            return np.array_equal(got[0], held) and got[1:] == (0.05,) + GEOMETRY

        bad = [(-0.1, 0.9, 3.0), (0.45, -0.9, 3.0), (0.45, 0.9, -3.0), (0.45, 0.9, float("nan")), (float("nan"), 0.9, 3.0),
               (0.45, float("inf"), 3.0), (0.45, 0.9, float("inf"))]
        for args in bad:
            assert lib.neo_mpc_inflate_world_map(h, *args) == -1 and lib.neo_mpc_last_error_code() == -1, args
            assert lib.neo_mpc_inflate_world_map_device(h, *args, None) == -1, args
            assert untouched(), args
        assert lib.neo_mpc_inflate_world_map(h, 0.45, 3.25, 3.0) == -5                # R = 65: NEO_MPC_ERR_UNSUPPORTED
        assert lib.neo_mpc_inflate_world_map_device(h, 0.45, 3.25, 3.0, None) == -5
        assert untouched()
        assert lib.neo_mpc_inflate_world_map(h, 0.45, 3.2, 3.0) == 0                  # R = 64 is served
        assert not untouched()


# ------------------------------------------------------------------------------------------ 8: one stream, one graph
def test_set_inflate_roll_can_be_captured_in_a_hip_graph():
    """After one eager call of each -- the inflation builds its cost table then -- set_world_map_device ->
    inflate_world_map_device -> roll_costmap_pool_device is captured on one stream, a linear chain, and replayed with the
    caller's raw device map rewritten in between: each replay's windows are the transcription's for the map of that replay."""
    import torch
    res, (wox, woy) = 0.05, GEOMETRY
    maps = [np.array(cpu.cases()[k][1]) for k in (-4, -8)]     # 130 x 75 cells at 3 % and at 0.2 % seeds
    maps.append(np.ascontiguousarray(maps[0][::-1, ::-1]))
    assert all(m.shape == (75, 130) for m in maps)
    poses = np.array([(wox + 1.7, woy + 1.1, 0.0), (wox + 3.9, woy + 2.6, 1.0), (wox + 6.4, woy + 1.9, -2.0)])
    start = poses[:, :2] - (0.9, 0.5) + 0.013
    with solver() as s:
        d_raw = torch.from_numpy(maps[0]).to(DEV)
        d_origins, d_poses = torch.from_numpy(start.copy()).to(DEV), torch.from_numpy(poses).to(DEV)

        def tick():
            s.set_world_map(d_raw, res, wox, woy)
            s.inflate_world_map(*PARAMS)
            s.roll_costmap_pool(36, 20, 0.05, d_origins, poses=d_poses)

        def expect(world, origins):
            return roll_ref.roll(ref.inflate_world(world, res, *PARAMS), res, wox, woy, origins, 36, 20, 0.05, poses=poses,
                                 outside_value=255)

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):          # the eager call, on the capture stream
            tick()
        torch.cuda.synchronize()
        origins, want = expect(maps[0], start)
        got, back = s.get_costmap_pool()
        assert back.tolist() == origins.tolist() and np.array_equal(got, want)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            tick()
        seen = [want]
        for world in maps[1:]:
            d_raw.copy_(torch.from_numpy(world).to(DEV))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            origins, want = expect(world, origins)
            got, back = s.get_costmap_pool()
            assert back.tolist() == origins.tolist()
            assert np.array_equal(got, want)
            assert np.array_equal(s.get_world_map()[0], ref.inflate_world(world, res, *PARAMS))
            assert not any(np.array_equal(want, w) for w in seen)                  # the windows changed with the map
            seen.append(want)


# ------------------------------------------------------------------------------------------ 9: two streams
@functools.lru_cache(maxsize=None)
def walled_world():
    """The stream-ordering world (256 x 256 cells) all free but for a lattice of walls every 40 cells: every window of the
    rig's pool holds a wall, so every window changes with the inflation."""
    cells = np.zeros((so.WORLD, so.WORLD), dtype=np.uint8)
    cells[::40, :] = 254
    cells[:, ::40] = 254
    cells.setflags(write=False)
    return cells


def _windows_of(world):
    return roll_ref.roll(world, so.RES, 0.0, 0.0, so.POOL_ORIGINS, so.WIN_X, so.WIN_Y, so.RES, outside_value=255)[1]


def test_a_roll_on_another_stream_waits_for_the_held_inflation(rig):
    """The inflation is held back on its stream, the roll is enqueued afterwards on another one: its windows show the
    inflated world (without the inflation's event the roll runs at once and cuts them from the raw one)."""
    r = rig(pool=True)
    back = r.readback("raw windows")[0]
    inflated = ref.inflate_world(walled_world(), so.RES, *PARAMS)

    def prepare():
        r.s.set_world_map(r.t(walled_world()), *so.WORLD_GEOM)
        r.roll()
        back.call()

    def check(want):
        assert np.array_equal(want["raw windows"], _windows_of(walled_world()))
        assert np.array_equal(want["inflated windows"], _windows_of(inflated))

    so.run(r, prepare, [so.Step("H", lambda: r.s.inflate_world_map(*PARAMS)), so.Step("A", r.roll)] + r.readback("inflated windows"),
           [("raw windows", "inflated windows", "any")], check=check)


def test_the_inflation_waits_for_the_held_roll(rig):
    """The roll is held back on its stream, the inflation is enqueued afterwards on another one: the roll's windows show the
    raw world (without the wait for the fence's last writer the inflation runs at once and the held roll cuts inflated ones)."""
    r = rig(pool=True)
    back = r.readback("inflated windows")[0]

    def prepare():
        r.s.set_world_map(r.t(walled_world()), *so.WORLD_GEOM)
        r.s.inflate_world_map(*PARAMS)
        r.roll()
        back.call()
        r.s.set_world_map(r.t(walled_world()), *so.WORLD_GEOM)

    def check(want):
        assert np.array_equal(want["raw windows"], _windows_of(walled_world()))

    so.run(r, prepare, [so.Step("H", r.roll), so.Step("A", lambda: r.s.inflate_world_map(*PARAMS))] + r.readback("raw windows"),
           [("raw windows", "inflated windows", "any")], check=check)


# ------------------------------------------------------------------------------------------ 10: K9 and K8 on one handle
CHAIN_WORLD = ((0.45, 0.9, 3.0), (0.2, 0.3, 5.0))             # the inflation's parameters by round: R = 18, 6 at 5 cm
CHAIN_STAMP = ((0.3, 0.6, 4.0), (0.45, 1.2, 2.0))             # the stamp's: R = 6, 12 at 0.1 m
CHAIN_RECT = ((0.3, 0.2), (-0.3, 0.2), (-0.3, -0.2), (0.3, -0.2))       # the shared footprint, 0.6 x 0.4 m
CHAIN_WINDOW = (36, 20, 0.1)


@functools.lru_cache(maxsize=None)
def chain_case():
    """(world, resolution, poses, start origins, [(origins, pool) after each round]) by the chain of the three transcriptions
    -- inflate_world, roll, stamp_pool -- with the asserts that the case tells the two cost tables apart: every stage changes
    cells, and either kernel with the other's table gives another result."""
    _, world, res, _, _ = cpu.cases()[16]
    assert world.shape == (75, 130) and res == 0.05 and (world == 254).sum() == 24
    wox, woy = GEOMETRY
    poses = np.array([(wox + 2.0, woy + 1.6, 0.3), (wox + 2.9, woy + 2.0, 1.0), (wox + 3.6, woy + 1.5, -2.0)])
    start = poses[:, :2] - (1.8, 1.0) + 0.013
    polygons = np.array([gate_ref.oriented(pose, CHAIN_RECT) for pose in poses])
    origins, rounds, counts = start, [], []
    for world_params, stamp_params in zip(CHAIN_WORLD, CHAIN_STAMP):
        world_table, stamp_table = ref.table_for(res, *world_params), stamp_ref.inflation_costs(CHAIN_WINDOW[2], *stamp_params)
        inflated = ref.inflate(world, *world_table)
        origins, cut = roll_ref.roll(inflated, res, wox, woy, origins, *CHAIN_WINDOW, poses=poses, outside_value=255)
        pool = stamp_ref.stamp_pool(cut, origins, CHAIN_WINDOW[2], polygons, *stamp_params)
        changed = [int((pool[k] != cut[k]).sum()) for k in range(3)]
        crossed = np.stack([stamp_ref.stamp_window(cut[k], origins[k], CHAIN_WINDOW[2], np.delete(polygons, k, axis=0), *world_table)[0]
                            for k in range(3)])
        print("R = %d, %d: the inflation changes %d cells (%d others with the stamp's table), the stamp %s (%d others with the "
              "world's table)" % (world_table[1], stamp_table[1], (inflated != world).sum(),
                                  (ref.inflate(world, *stamp_table) != inflated).sum(), changed, (crossed != pool).sum()))
        assert (inflated != world).any() and all(changed)
        assert (crossed != pool).any() and (ref.inflate(world, *stamp_table) != inflated).any()
        counts.append(((inflated != world).sum(), changed, (crossed != pool).sum(), (ref.inflate(world, *stamp_table) != inflated).sum()))
        pool.setflags(write=False)
        rounds.append((origins, pool))
    assert not np.array_equal(rounds[0][1], rounds[1][1])
    assert counts == [(8519, [98, 209, 116], 675, 7962), (2204, [334, 552, 355], 683, 4484)]        # the case, pinned down
    return world, res, poses, start, rounds


@pytest.mark.parametrize("where", ("host", "device"))
def test_inflation_and_stamp_on_one_handle_keep_their_tables_apart(where):
    """set -> inflate -> roll -> stamp twice on one handle, the inflation's and the stamp's parameters -- and reach --
    different from each other and changed between the rounds: after each round the pool is the chain of the three
    transcriptions, exactly.  NumPy arrays through the host calls, CUDA tensors through the device calls."""
    import torch
    world, res, poses, start, rounds = chain_case()
    put = (lambda a: np.array(a)) if where == "host" else (lambda a: torch.from_numpy(np.array(a)).to(DEV))
    footprint, d_poses, origins = put(np.asarray(CHAIN_RECT)), put(poses), put(start)
    with solver() as s:
        for world_params, stamp_params, (want_origins, want) in zip(CHAIN_WORLD, CHAIN_STAMP, rounds):
            s.set_world_map(put(world), res, *GEOMETRY)
            s.inflate_world_map(*world_params)
            s.roll_costmap_pool(*CHAIN_WINDOW, origins, poses=d_poses)
            s.stamp_fleet(*stamp_params, footprint=footprint, poses=d_poses)
            got, back = s.get_costmap_pool()
            assert back.tolist() == want_origins.tolist()
            assert np.array_equal(got, want), (where, world_params, stamp_params, int((got != want).sum()))
