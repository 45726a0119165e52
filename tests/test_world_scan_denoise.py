"""The speckle filter of the fleet's shared obstacle layer (K13): between the layer and its composition, a mark whose group of
occupied cells has fewer than G members reaches `live` as a free cell; the layer keeps it.

The contract is step 3b of the text in include/neo_mpc.h (neo_mpc_fleet_clear, neo_mpc_set_world_scan_denoise) and its executable
form the transcription in tests/world_denoise_reference.py, on top of tests/world_scan_layer_reference.py for the layer and of
the scan layer's own combine_into and inflate_from for `live`.  The step is integers only: every comparison is exact equality
of uint8 cells -- no tolerance, no dropped case."""
import collections
import ctypes as C
import functools
import math
import re

import numpy as np
import pytest

from neo_mpc_planner2_amd import _lib, abi
from tests import rolling_window_reference as roll_ref
from tests import world_denoise_reference as ref
from tests import world_scan_layer_reference as world_ref
from tests.c_probe import HEADER, run_c_probe
from tests.fleet_kit import (F32, FAR, RECT, Side, capture_fleet, cell_centre, denoised_of, gpu, inflation_for, pairs_fleet,
                             rectangle, replay_against_direct, rolled_pool, same, scanner, world_scan_callback, world_state)
from tests.world_scan_cases import UPDATE_FLAGS, WORLDS, expected, ranges_for
from tests.world_scan_cases import case as world_case

ENTRY_POINTS = ("neo_mpc_set_world_scan_denoise", "neo_mpc_get_world_scan_denoised")
MARK = world_ref.MARK
SETTINGS = ((2, 8), (2, 4), (3, 8), (16, 8), (16, 4))
DENOISE_WORLDS = ("130x67-2.5cm", "40x40-10cm")      # more than one tile each way, a width that is no multiple of 4; less than a tile
DENOISE_REACHES = (0, 3, 64)


# ------------------------------------------------------------------------------------------ 1: the rule by hand
def grid(rows):
    """A 12 x 10 grid from ten strings of twelve characters, the first string being row 0."""
    assert len(rows) == 10 and all(len(r) == 12 for r in rows)
    return np.array([[{".": 0, "?": 255, "#": 254, "w": 253}[c] for c in r] for r in rows], dtype=np.uint8)


def test_the_rule_by_hand():
    """Layer and world drawn cell by cell; '#' = 254, '.' = 0, '?' = 255, 'w' = 253."""
    layer = grid(["#?..........",      # (0, 0): a mark in the corner cell, alone
                  "?...#.......",      # (4, 1) and (5, 2): a diagonal pair
                  ".....#......",
                  "............",
                  ".#......#...",      # (1, 4), (1, 5), (2, 5): an L of three;  (8, 4): a lone mark
                  ".##.........",
                  "............",
                  "..#.....#...",      # (2, 7): a mark beside the world's 254 at (3, 7);  (8, 7): layer 254 over world 254, alone
                  "............",
                  "...........?"])     # (10, 9): layer 0 over world 254 and (11, 9) 255 beside it
    world = grid(["............",
                  "............",
                  "............",
                  "............",
                  "............",
                  "............",
                  "............",
                  "...#....#...",
                  "............",
                  "..........#w"])
    assert ref.denoise(layer, world, 0, 8).tobytes() == layer.tobytes() == ref.denoise(layer, world, 1, 4).tobytes()

    def freed(group, connectivity):
        got = ref.denoise(layer, world, group, connectivity)
        changed = np.argwhere(got != layer)
        assert (got[got != layer] == 0).all()
        for form in (ref.small_by_flood_fill, ref.small_by_bounded_ball):
            assert np.array_equal(ref.denoise(layer, world, group, connectivity, small=form), got)
        return sorted((int(i), int(l)) for l, i in changed)

    lone, corner, pair, ell = [(8, 4)], [(0, 0)], [(4, 1), (5, 2)], [(1, 4), (1, 5), (2, 5)]
    # G = 2: the lone marks go; the diagonal pair is a group under 8 and two groups of one under 4; the mark beside the
    # world's wall is a group of two WITH the wall and is kept
    assert freed(2, 8) == sorted(lone + corner)
    assert freed(2, 4) == sorted(lone + corner + pair)
    # G = 3: the pair goes under both, and so does the mark beside the one-cell wall; the L of three stays under both
    assert freed(3, 8) == sorted(lone + corner + pair + [(2, 7)]) == freed(3, 4)
    # G = 4: the L goes too
    assert freed(4, 8) == sorted(lone + corner + pair + ell + [(2, 7)]) == freed(4, 4)
    # layer 254 over world 254 is left as it is whatever G, and layer 0 over world 254 stays 0: nothing but marks changes
    for group in (2, 16):
        got = ref.denoise(layer, world, group, 8)
        assert got[7, 8] == 254 and got[9, 10] == 0 and got[9, 11] == 255
    # ... but layer 0 over world 254 COUNTS as occupied: a mark beside it is a group of two
    beside = layer.copy()
    beside[8, 10] = 254
    assert ref.denoise(beside, world, 2, 4)[8, 10] == 254 and ref.denoise(beside, world, 3, 4)[8, 10] == 0
    assert ref.denoise(beside, world * 0, 2, 4)[8, 10] == 0


# ------------------------------------------------------------------------------------------ 2: three forms agree
def test_flood_fill_label_and_bounded_ball_agree_on_random_grids():
    rng = np.random.default_rng(1301)
    stats = collections.Counter()
    kept = dropped = 0
    for k, density in enumerate(np.linspace(0.05, 0.45, 9)):
        sy, sx = (23, 31) if k % 2 else (17, 40)
        occ = rng.random((sy, sx)) < density
        for connectivity in (4, 8):
            by_fill = ref.group_sizes_by_flood_fill(occ, connectivity, stats)
            assert np.array_equal(by_fill, ref.group_sizes_by_label(occ, connectivity)), (density, connectivity)
            for group in (1, 2, 3, 5, 8, 16):
                want = occ & (by_fill < group)
                assert np.array_equal(ref.small_by_label(occ, group, connectivity), want)
                assert np.array_equal(ref.small_by_bounded_ball(occ, group, connectivity), want), (density, connectivity, group)
                kept += int((occ & ~want).sum())
                dropped += int(want.sum())
    print(dict(stats), kept, dropped)
    assert kept > 0 and dropped > 0
    for name in ("denoise: a neighbour outside the world", "denoise: a neighbour that is not occupied",
                 "denoise: a neighbour already in the group", "denoise: a neighbour joins the group",
                 "denoise: a group of one", "denoise: a group of several"):
        assert stats[name] > 0, name


# ------------------------------------------------------------------------------------------ 3: entry points
def test_entry_points_constant_and_refusals_without_a_handle(tmp_path):
    got = run_c_probe(tmp_path, '#include <stdio.h>\n#include "neo_mpc.h"\n'
                      'int main(void) {\n  printf("group %u\\n", NEO_MPC_MAX_DENOISE_GROUP);\n'
                      '  int (*set)(neo_mpc_handle*, uint32_t, uint32_t) = neo_mpc_set_world_scan_denoise;\n'
                      '  int (*get)(neo_mpc_handle*, uint8_t*) = neo_mpc_get_world_scan_denoised;\n'
                      '  void* volatile f[2] = {(void*)set, (void*)get};\n  return f[0] == 0 || f[1] == 0;\n}\n')
    assert int(got["group"]) == abi.MAX_DENOISE_GROUP == ref.MAX_GROUP == 16
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\s*\(" % name, text), name
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert "#define NEO_MPC_ABI_VERSION 2" in text and "#define NEO_MPC_BEHAVIOUR_VERSION 6" in text
    assert lib.neo_mpc_abi_version() == 2 and lib.neo_mpc_behaviour_version() == 6
    for group, connectivity in ((17, 8), (2, 0), (2, 5), (2, 6), (2, 8), (0, 4)):
        assert lib.neo_mpc_set_world_scan_denoise(None, group, connectivity) == -1
        assert lib.neo_mpc_last_error_code() == -1
    assert lib.neo_mpc_get_world_scan_denoised(None, None) == -1


# ------------------------------------------------------------------------------------------ the generator
def line(i, l, di, dl, n):
    return [(i + k * di, l + k * dl) for k in range(n)]


def stairs(i, l, n):
    """A chain that turns at every cell, connected under 4: right, up, right, up, ..."""
    return [(i + (k + 1) // 2, l + k // 2) for k in range(n)]


def shapes_for(world, group, connectivity):
    """name -> cells (i, l) to mark, and the world cells to make 254.  Every shape keeps a ring of two cells around it that
    holds no speckle and no wall of the random world map, so that it is exactly what its name says."""
    g = group
    shapes, walls = {}, []
    arm = g // 2 + 2                                     # the U: two arms `arm` cells high, a gap column, one cell below the gap
    if world == "130x67-2.5cm":
        shapes["straight G-1"], shapes["straight G"] = line(2, 2, 1, 0, g - 1), line(2, 5, 1, 0, g)
        shapes["diagonal G-1"], shapes["diagonal G"] = line(22, 2, 1, 1, g - 1), line(40, 2, 1, 1, g)
        shapes["stairs G-1"], shapes["stairs G"] = stairs(2, 10, g - 1), stairs(2, 22, g)
        shapes["across columns 63|64 G"], shapes["across columns 63|64 G-1"] = line(64 - g // 2, 22, 1, 0, g), line(65 - g // 2, 25, 1, 0, g - 1)
        start = min(63 - (g - 1) // 2, 67 - g)
        shapes["across rows 63|64 G"], shapes["across rows 63|64 G-1"] = line(20, start, 0, 1, g), line(24, start, 0, 1, g - 1)
        m = max(0, min((g - 3) // 2, 5))
        shapes["across the tile corner G"] = stairs(63 - m, 63 - m, g)
        shapes["row 0 G"], shapes["row 0 G-1"] = line(70, 0, 1, 0, g), line(95, 0, 1, 0, g - 1)
        shapes["last column G"], shapes["last column G-1"] = line(129, 5, 0, 1, g), line(129, 30, 0, 1, g - 1)
        shapes["G-1 ending on a wall"] = line(75, 12, 1, 0, g - 1)
        walls.append((75 + g - 1, 12))
        other = line(75 + g - 1, 31, 1, 0, g - 1) if connectivity == 4 else line(75, 32, 1, 0, g - 1)
        shapes["two groups of G-1"] = line(75, 30, 1, 0, g - 1) + other
        shapes["U"] = line(110, 5, 0, 1, arm) + line(112, 5, 0, 1, arm) + [(111, 5)]
        shapes["wider than 31"] = line(70, 48, 1, 0, 40)
    else:
        shapes["straight G-1"], shapes["straight G"] = line(2, 2, 1, 0, g - 1), line(2, 5, 1, 0, g)
        shapes["row 0 G"] = line(20, 0, 1, 0, g)
        shapes["last column G-1"] = line(39, 5, 0, 1, g - 1)
        shapes["diagonal G"] = line(2, 9, 1, 1, g)
        shapes["stairs G-1"] = stairs(22, 8, g - 1)
        shapes["G-1 ending on a wall"] = line(2, 30, 1, 0, g - 1)
        walls.append((2 + g - 1, 30))
        other = line(2 + g - 1, 35, 1, 0, g - 1) if connectivity == 4 else line(2, 36, 1, 0, g - 1)
        shapes["two groups of G-1"] = line(2, 34, 1, 0, g - 1) + other
        shapes["U"] = line(24, 20, 0, 1, arm) + line(26, 20, 0, 1, arm) + [(25, 20)]
        shapes["wider than 31"] = line(2, 38, 1, 0, 35)
    return shapes, walls


@functools.lru_cache(maxsize=None)
def denoise_case(world, group, connectivity):
    """(cells [sy, sx] of the world map, wox, woy, points [1, n, 2], sensor origin [1, 2], shapes).  The world map is random
    as in tests/world_scan_cases.py, so walls join groups; speckle of density 0.02 everywhere but around the shapes."""
    sx, sy, res = WORLDS[world]
    rng = np.random.default_rng(77 * sx + 5 * group + connectivity)
    cells = rng.choice(np.array([0, 0, 0, 0, 60, 150, 253, 254, 255, 255, 255], dtype=np.uint8), size=(sy, sx))
    wox, woy = (float(v) for v in rng.uniform(-5.0, 5.0, size=2))
    shapes, walls = shapes_for(world, group, connectivity)
    names = sorted(shapes)
    for a in names:                                      # the shapes are apart: no cell of one touches a cell of another
        for b in names:
            if a < b:
                assert min(max(abs(p[0] - q[0]), abs(p[1] - q[1])) for p in shapes[a] for q in shapes[b]) >= 2, (a, b)
    keep_out = np.zeros((sy, sx), dtype=bool)
    marks = np.zeros((sy, sx), dtype=bool)
    for cells_of in shapes.values():
        for i, l in cells_of:
            assert 0 <= i < sx and 0 <= l < sy, (i, l)
            keep_out[max(l - 2, 0):l + 3, max(i - 2, 0):i + 3] = True
            marks[l, i] = True
    cells[keep_out & (cells == 254)] = 253
    for i, l in walls:
        cells[l, i] = 254
    marks |= (rng.random((sy, sx)) < 0.02) & ~keep_out
    at = np.argwhere(marks)
    points = np.stack([wox + (at[:, 1] + 0.5) * res, woy + (at[:, 0] + 0.5) * res], 1)[None]
    sensor = np.array([[wox + sx * res / 2, woy + sy * res / 2]])
    for a in (cells, points, sensor):
        a.setflags(write=False)
    return cells, wox, woy, points, sensor, shapes


@functools.lru_cache(maxsize=None)
def marked_layer(world, group, connectivity):
    """(layer, D) of the transcription after the case's one update of marks, computed once per case."""
    cells, wox, woy, points, sensor, _ = denoise_case(world, group, connectivity)
    model = world_ref.WorldScanLayer()
    model.update(cells, WORLDS[world][2], wox, woy, 0.0, 0.0, 1.0, points=points, sensor_origins=sensor, flags=MARK, **FAR)
    layer, d = model.layer, ref.denoise(model.layer, cells, group, connectivity)
    layer.setflags(write=False)
    d.setflags(write=False)
    return layer, d


@functools.lru_cache(maxsize=None)
def expected_live(world, reach, group, connectivity):
    cells = denoise_case(world, group, connectivity)[0]
    table, got = ref.inflation_costs(WORLDS[world][2], *inflation_for(reach, WORLDS[world][2]))
    assert got == reach
    d = marked_layer(world, group, connectivity)[1]
    live = ref.scan_ref.inflate_from(ref.scan_ref.combine_into(cells, d), d, table, reach)
    live.setflags(write=False)
    return live


@pytest.mark.parametrize("world", DENOISE_WORLDS)
@pytest.mark.parametrize("group,connectivity", SETTINGS)
def test_the_shapes_of_the_cases_come_out_as_designed(world, group, connectivity):
    """The marks land where they were put, and the transcription keeps and drops the shapes their names promise."""
    cells, _, _, _, _, shapes = denoise_case(world, group, connectivity)
    layer, d = marked_layer(world, group, connectivity)
    for name, at in shapes.items():
        assert all(layer[l, i] == 254 for i, l in at), name
    assert np.array_equal(d, ref.denoise(layer, cells, group, connectivity, small=ref.small_by_flood_fill))

    def kept(name):
        values = {int(d[l, i]) for i, l in shapes[name]}
        assert len(values) == 1 and values <= {0, 254}, (name, values)
        return values == {254}

    for name in shapes:
        if name.endswith("G-1"):
            assert not kept(name), name                  # fewer than G cells, however they are connected
        elif name.endswith(" G"):                        # exactly G cells: under 4 a diagonal chain is groups of one
            assert kept(name) is (connectivity == 8 or not name.startswith("diagonal")), name
    assert kept("G-1 ending on a wall") and kept("U") and kept("wider than 31")
    assert not kept("two groups of G-1")                 # a window count that ignores connectivity keeps them
    assert len(shapes["two groups of G-1"]) == 2 * (group - 1) >= group
    speckle = (layer == 254) & (d == 0)
    assert speckle.sum() > sum(len(s) for n, s in shapes.items() if not kept(n))   # ... and random speckle is dropped too


# ------------------------------------------------------------------------------------------ 4: equality with the transcription
CASES = [(w, r, g, c) for w in DENOISE_WORLDS for r in DENOISE_REACHES for g, c in SETTINGS]


@pytest.mark.gpu
@pytest.mark.parametrize("world,reach,group,connectivity", CASES, ids=["%s-R%d-G%d-c%d" % c for c in CASES])
def test_filtered_updates_equal_the_transcription(world, reach, group, connectivity):
    from neo_mpc_planner2_amd.solver import BatchSolver
    sx, sy, res = WORLDS[world]
    cells, wox, woy, points, sensor, _ = denoise_case(world, group, connectivity)
    layer, d = marked_layer(world, group, connectivity)
    live = expected_live(world, reach, group, connectivity)
    params = inflation_for(reach, res)
    assert (d != layer).any() and ((d == 254) & (cells != 254)).any()
    with BatchSolver({}) as s:
        s.set_world_scan_denoise(group, connectivity)
        for put in (gpu, np.array):                                       # the device and the host variants
            s.set_world_map(put(cells), res, wox, woy)
            s.reset_world_scan_layer()
            for repeat in range(2):                                       # repeated with the same inputs: nothing changes
                s.update_world_scan_layer(*params, points=put(points), sensor_origins=put(sensor), flags=MARK, **FAR)
                got_layer, got_live = world_state(s)
                got_d = denoised_of(s)
                assert np.array_equal(got_layer, layer), (put.__name__, repeat)       # the layer is not changed by the filter
                assert np.array_equal(got_d, d), (put.__name__, repeat, np.argwhere(got_d != d)[:8].tolist())
                assert np.array_equal(got_live, live), (put.__name__, repeat, int((got_live != live).sum()))
            assert np.array_equal(s.get_world_map()[0], cells)            # the static map is what it was
    print("%s R=%d G=%d/%d: %d marks, %d dropped" % (world, reach, group, connectivity, int((layer == 254).sum()),
                                                    int((d != layer).sum())))


# ------------------------------------------------------------------------------------------ 5: off is as before
@pytest.mark.gpu
def test_off_is_the_update_as_it_was():
    from neo_mpc_planner2_amd.solver import BatchSolver
    key = ("96x70-5cm", 3, 3, 64, 255)
    sx, sy, res = WORLDS[key[0]]
    cells, wox, woy, updates, polygons = world_case(key[0], key[2], key[3])
    want, _ = expected(*key)
    params, ranges = inflation_for(key[1], res), ranges_for(key[0])
    for setting in (None, (0, 4), (1, 8)):
        with BatchSolver({}) as s:
            if setting is not None:
                s.set_world_scan_denoise(16, 4)                           # ... and off again, before any update
                s.set_world_scan_denoise(*setting)
            s.set_world_map(gpu(cells), res, wox, woy)
            for k, ((points, counts, sensors), flags) in enumerate(zip(updates, UPDATE_FLAGS)):
                kw = dict(flags=flags, clear=dict(polygons=gpu(polygons), padding=1.5 * res), **ranges)
                if points is not None:
                    kw.update(points=gpu(points), sensor_origins=gpu(sensors), point_counts=gpu(counts, np.int32))
                else:
                    kw.update(on_device=True)
                s.update_world_scan_layer(*params, **kw)
                got = world_state(s)
                assert np.array_equal(got[0], want[k][0]) and np.array_equal(got[1], want[k][1]), (setting, k)
                assert np.array_equal(denoised_of(s), want[k][0]), (setting, k)   # the getter returns the layer


# ------------------------------------------------------------------------------------------ 6: the layer remembers
@pytest.mark.gpu
def test_the_layer_remembers_a_lone_mark_until_its_neighbour_comes():
    from neo_mpc_planner2_amd.solver import BatchSolver
    world = np.zeros((70, 70), dtype=np.uint8)
    params = (0.5, 2.5, 1.0)                                              # 1 m cells: a ring of three cells around a seed
    sensor = np.array([[35.5, 35.5]])
    first, second = np.array([[cell_centre(63, 20)]]), np.array([[cell_centre(64, 20)]])   # either side of the tile boundary
    model = ref.DenoisedWorldScanLayer(2, 8)
    with BatchSolver({}) as s:
        s.set_world_scan_denoise(2)
        for put in (gpu, np.array):
            s.set_world_map(put(world), 1.0, 0.0, 0.0)
            s.reset_world_scan_layer()
            model.reset()
            model.set_denoise(2, 8)
            s.set_world_scan_denoise(2, 8)
            # update 1 marks one cell: in the layer, not in live
            s.update_world_scan_layer(*params, points=put(first), sensor_origins=put(sensor), flags=MARK, **FAR)
            layer, live = world_state(s)
            assert layer[20, 63] == 254 and (layer == 254).sum() == 1 and not live.any() and denoised_of(s)[20, 63] == 0
            want = model.update(world, 1.0, 0.0, 0.0, *params, points=first, sensor_origins=sensor, flags=MARK, **FAR)
            assert same((layer, live, denoised_of(s)), (model.layer, want, model.denoised))
            # update 2, marks alone, marks its neighbour: both are in live with their rings
            s.update_world_scan_layer(*params, points=put(second), sensor_origins=put(sensor), flags=MARK, **FAR)
            layer, live = world_state(s)
            want = model.update(world, 1.0, 0.0, 0.0, *params, points=second, sensor_origins=sensor, flags=MARK, **FAR)
            assert layer[20, 63] == 254 and layer[20, 64] == 254 and live[20, 63] == 254 and live[20, 64] == 254
            assert 0 < live[20, 61] < 253 and 0 < live[22, 64] < 253 and live[20, 59] == 0    # (R = 3: the ring ends three cells out)
            assert same((layer, live, denoised_of(s)), (model.layer, want, model.denoised))
        # a lone mark again; the setter to off and an update without a scan puts it back, the setter to on removes it
        s.reset_world_scan_layer()
        model.reset()
        s.update_world_scan_layer(*params, points=first, sensor_origins=sensor, flags=MARK, **FAR)
        model.update(world, 1.0, 0.0, 0.0, *params, points=first, sensor_origins=sensor, flags=MARK, **FAR)
        held = world_state(s)
        assert not held[1].any()
        s.set_world_scan_denoise(0)
        assert same(world_state(s), held)                                   # the setter itself changes nothing
        s.update_world_scan_layer(*params, flags=0, **FAR)
        model.set_denoise(0)
        want = model.update(world, 1.0, 0.0, 0.0, *params, flags=0, **FAR)
        layer, live = world_state(s)
        assert live[20, 63] == 254 and 0 < live[20, 65] < 253 and same((layer, live), (model.layer, want))
        assert np.array_equal(denoised_of(s), layer)
        s.set_world_scan_denoise(2, 4)
        s.update_world_scan_layer(*params, flags=0, **FAR)
        layer, live = world_state(s)
        assert layer[20, 63] == 254 and not live.any() and denoised_of(s)[20, 63] == 0
        # the setting survives a reset of the layer and a new world map
        s.reset_world_scan_layer()
        s.set_world_map(world, 1.0, 0.0, 0.0)
        s.update_world_scan_layer(*params, points=first, sensor_origins=sensor, flags=MARK, **FAR)
        layer, live = world_state(s)
        assert layer[20, 63] == 254 and not live.any()


# ------------------------------------------------------------------------------------------ 7: order
@pytest.mark.gpu
def test_the_filter_runs_behind_the_footprint_clearing_of_the_same_update():
    """A group of G = 3 cells in a row of which the fleet footprint clearing frees one: the other two are dropped in the
    same update."""
    from neo_mpc_planner2_amd.solver import BatchSolver
    world = np.zeros((32, 32), dtype=np.uint8)
    points = np.array([[cell_centre(10, 12), cell_centre(11, 12), cell_centre(12, 12)]])
    sensor = np.array([[20.5, 20.5]])
    clear = dict(polygons=np.array([rectangle(12.1, 11.1, 13.9, 12.9)]), padding=0.0)      # cells (12, 11), (12, 12), (13, *)
    params = (0.0, 0.0, 1.0)
    with BatchSolver({}) as s:
        s.set_world_scan_denoise(3, 4)
        model = ref.DenoisedWorldScanLayer(3, 4)
        for put in (gpu, np.array):
            s.set_world_map(put(world), 1.0, 0.0, 0.0)
            s.reset_world_scan_layer()
            model.reset()
            s.update_world_scan_layer(*params, points=put(points), sensor_origins=put(sensor), flags=MARK, **FAR)
            assert (world_state(s)[1] == 254).sum() == 3                     # without the clearing: a group of three, kept
            s.reset_world_scan_layer()
            s.update_world_scan_layer(*params, points=put(points), sensor_origins=put(sensor), flags=MARK,
                                      clear=dict(polygons=put(clear["polygons"]), padding=0.0), **FAR)
            want = model.update(world, 1.0, 0.0, 0.0, *params, points=points, sensor_origins=sensor, flags=MARK, clear=clear, **FAR)
            layer, live = world_state(s)
            assert layer[12, 10] == 254 and layer[12, 11] == 254 and layer[12, 12] == 0 and (layer == 254).sum() == 2
            assert not (live == 254).any() and same((layer, live, denoised_of(s)), (model.layer, want, model.denoised))


# ------------------------------------------------------------------------------------------ 8: the roll
@pytest.mark.gpu
def test_the_roll_cuts_its_windows_from_the_filtered_map():
    from neo_mpc_planner2_amd.solver import BatchSolver
    res, size = 0.05, 60
    world = np.zeros((200, 200), dtype=np.uint8)
    params = (0.1, 0.3, 3.0)
    poses = np.array([(0.012, 0.017, 0.0), (1.512, 0.017, 0.0)])
    pallet = np.array([(0.7 + 0.05 * (j % 3), -0.1 + 0.05 * (j // 3)) for j in range(12)])
    speck = np.array([(1.9, 0.4)])                                        # in robot 1's window, more than a ring from the pallet
    points = np.stack([np.concatenate([pallet, speck]), np.full((13, 2), np.nan)])
    start = poses[:, :2] - size * res / 2 + 0.013
    plain, model = world_ref.WorldScanLayer(), ref.DenoisedWorldScanLayer(2, 8)
    with_speck = plain.update(world, res, -5.0, -5.0, *params, points=points, sensor_origins=poses[:, :2])
    live = model.update(world, res, -5.0, -5.0, *params, points=points, sensor_origins=poses[:, :2])
    alone = world_ref.WorldScanLayer().update(world, res, -5.0, -5.0, *params, points=points[:, :12], sensor_origins=poses[:, :2])
    ring = with_speck != alone                                            # what the speck and its ring raise
    assert ring.sum() > 20 and (model.layer == 254).sum() - (model.denoised == 254).sum() == 1
    assert np.array_equal(live, alone) and not live[ring].any()
    want_origins, want = roll_ref.roll(live, res, -5.0, -5.0, start, size, size, res, poses=poses, outside_value=255)
    unfiltered = roll_ref.roll(with_speck, res, -5.0, -5.0, start, size, size, res, poses=poses, outside_value=255)[1]
    assert (unfiltered[1] != want[1]).sum() > 20 and (want[1] == 254).any()
    with BatchSolver({}) as s:
        s.set_world_scan_denoise(2)
        s.set_world_map(gpu(world), res, -5.0, -5.0)
        s.update_world_scan_layer(*params, points=gpu(points), sensor_origins=gpu(poses[:, :2]))
        assert same(world_state(s), (model.layer, live))
        pool, origins = rolled_pool(s, size, size, res, start.copy(), poses)
        assert origins.tolist() == want_origins.tolist() and np.array_equal(pool, want)
        assert not pool[1][unfiltered[1] != want[1]].any()               # no cell the speck's ring would have raised


# ------------------------------------------------------------------------------------------ 9: refusals
@pytest.mark.gpu
def test_refused_settings_leave_everything_and_the_setting_in_force_alone():
    from neo_mpc_planner2_amd.solver import BatchSolver
    world_name, group, connectivity = "40x40-10cm", 3, 4
    sx, sy, res = WORLDS[world_name]
    cells, wox, woy, points, sensor, _ = denoise_case(world_name, group, connectivity)
    layer, d = marked_layer(world_name, group, connectivity)
    live = expected_live(world_name, 3, group, connectivity)
    params = inflation_for(3, res)
    poses = np.array([[sensor[0, 0], sensor[0, 1], 0.0]])
    size = 24
    start = sensor - size * res / 2 + 0.013
    with BatchSolver({}) as s:
        lib, h = s._lib, s._handle
        assert lib.neo_mpc_set_world_scan_denoise(h, 17, 8) == -1 and lib.neo_mpc_set_world_scan_denoise(h, 2, 5) == -1   # no world map needed to refuse
        assert lib.neo_mpc_set_world_scan_denoise(h, group, connectivity) == 0             # ... or to accept
        assert lib.neo_mpc_get_world_scan_denoised(h, None) == -4
        s.set_world_map(cells, res, wox, woy)
        assert lib.neo_mpc_get_world_scan_denoised(h, None) == -4                          # no layer yet
        s.update_world_scan_layer(*params, points=points, sensor_origins=sensor, flags=MARK, **FAR)
        assert lib.neo_mpc_get_world_scan_denoised(h, None) == 0
        rolled_pool(s, size, size, res, start.copy(), poses)

        def state():
            return world_state(s) + (denoised_of(s), s.get_costmap_pool()[0])

        held = state()
        assert same(held[:3], (layer, live, d)) and (d != layer).any()
        for bad in ((17, 8), (17, 4), (0xFFFFFFFF, 8), (2, 0), (2, 5), (2, 6), (0, 5), (1, 0), (group, 7)):
            assert lib.neo_mpc_set_world_scan_denoise(h, *bad) == -1, bad
            assert lib.neo_mpc_last_error_code() == -1 and same(state(), held), bad
        assert lib.neo_mpc_set_world_scan_denoise(None, 2, 8) == -1 and lib.neo_mpc_get_world_scan_denoised(None, None) == -1
        # the setting in force is still (3, 4): an update without a scan composes the same D and live
        s.update_world_scan_layer(*params, flags=0, **FAR)
        assert same(state(), held)
        # ... which (3, 8) and off do not
        other = ref.denoise(layer, cells, 3, 8)
        assert (other != d).any()
        s.set_world_scan_denoise(3, 8)
        s.update_world_scan_layer(*params, flags=0, **FAR)
        assert np.array_equal(denoised_of(s), other)
        s.reset_world_scan_layer()
        assert lib.neo_mpc_get_world_scan_denoised(h, None) == -4


# ------------------------------------------------------------------------------------------ 10: graph capture
@pytest.mark.gpu
def test_the_filtered_tick_can_be_captured_in_a_hip_graph():
    """The chain of tests/test_world_scan_layer.py's capture test with the filter on at G = 3: after one eager call, world scan
    from ranges -> roll -> stamp -> gate -> solve is captured on one stream, a linear chain, and replayed twice with ranges
    and poses rewritten in between; layer, D, live, pool, gate costs and commands equal direct calls on a second handle."""
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

    class FilteredSide(Side):
        def __init__(self, fleet, tick):
            super().__init__(fleet, tick)
            self.ranges = gpu(tick[1])

        def open_solver(self):
            s = super().open_solver()
            s.set_world_scan_denoise(3)
            return s

        def set_inputs(self, tick):
            super().set_inputs(tick)
            self.ranges.copy_(gpu(tick[1]))

        def tick(self):                                                   # (the eager one allocates D)
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
            return common + (self.s.get_costmap_pool()[0].tobytes(), layer.tobytes(), live.tobytes(),
                             self.s.get_world_scan_denoised().tobytes())

    # pool, layer, live and D changed
    with replay_against_direct(lambda: FilteredSide(f, ticks[0]), ticks, changed=(4, 5, 6, 7)) as (_, a, _):
        shape = f.world.shape
        layer, live, d = (np.frombuffer(x, dtype=np.uint8).reshape(shape) for x in a[5:8])
        assert (layer == 254).any() and (d != layer).any() and np.array_equal(d, ref.denoise(layer, f.world, 3, 8))


# ------------------------------------------------------------------------------------------ 11: the closed loop
@pytest.mark.gpu
def test_closed_loop_a_stray_return_no_longer_stops_a_robot_and_a_wall_still_does():
    """64 robots in 32 pairs on a free world map, fleet_kit.pairs_fleet: the even robot of a pair stands 1.5 m
    behind the odd one and its front scanner looks at it; the odd robots' own ranges hold nothing.  In a third of the pairs
    ONE beam of the even robot returns, from the odd robot's front edge -- the world cell that the odd robot's window shows in
    the column its gate walks for that edge at tick 0; in the others all beams return a wall 0.3 m in front of the odd robot's
    centre, a group of many cells.  Without the filter every odd robot is stopped by the latch at some tick; with G = 2 the
    ones behind the stray return never are and the ones behind the wall still are.  The even robots' rays run through the
    previous tick's marks before they mark again, so a stray return stays one cell.  A handle on which the setter was never
    called runs the loop as it was, bit for bit."""
    import torch
    from neo_mpc_planner2_amd import fleet as fleet_loop
    from neo_mpc_planner2_amd.solver import BatchSolver, DeviceBatch
    from oracle import mpc_oracle as orc
    ticks = 4
    wox = woy = -10.0
    world = np.zeros((400, 400), dtype=np.uint8)
    p = pairs_fleet()
    count, size, res, beams, probs, st, warm, xy, origins = p.count, p.size, p.res, p.beams, p.probs, p.st, p.warm, p.xy, p.origins
    stray = np.arange(32) % 3 == 0                                       # pairs 0, 3, 6, ...: a third
    ranges = np.full((count, 1, beams), np.inf, dtype=F32)               # (no INF_IS_VALID: nothing, not even a clearing ray)
    for pair in range(32):
        seer, odd = 2 * pair, 2 * pair + 1
        if not stray[pair]:
            ranges[seer, 0] = (1.7 / np.cos(p.angle)).astype(F32)          # x = 0.1 + 1.7 in the even robot's base frame
            continue
        ox = roll_ref.move_origin(origins[odd], xy[odd], size, size, res)[0]
        column = math.floor((xy[odd, 0] + RECT[0][0] - ox) / res)        # the window column of the front edge
        shown = roll_ref.world_cell(ox + (column + 0.5) * res, wox, res, 400)          # ... and the world column it shows
        ranges[seer, 0, beams // 2] = wox + (shown + 0.5) * res - (xy[seer, 0] + 0.1)
    assert abs(p.angle[beams // 2]) < 1e-12 and stray.sum() == 11
    world_scan = world_scan_callback((0.1, 0.3, 3.0), gpu(ranges), p.front)

    runs, marks = {}, {}
    for how, group in (("never set", None), ("off", 0), ("G = 2", 2)):
        with BatchSolver(orc.make_params()) as s:
            if group is not None:
                s.set_world_scan_denoise(group)
            s.set_world_map(world, res, wox, woy)
            flags = []
            d_orig = gpu(origins)
            s.roll_costmap_pool(size, size, res, d_orig)
            b = DeviceBatch(probs, st, warm, "cuda:0")
            fleet_loop.closed_loop(s, b, ticks, after_tick=lambda t, cm: flags.append(cm.copy()), footprint=RECT,
                                   rolling=(size, size, res, d_orig), world_scan=world_scan)
            torch.cuda.synchronize()
            runs[how] = np.array(flags)
            marks[how] = (s.get_world_scan_layer()[0], s.get_world_scan_denoised())
    assert runs["never set"].tobytes() == runs["off"].tobytes()
    ever = {how: ((f["flags"] & abi.FLAG_STOPPED) != 0).any(axis=0) for how, f in runs.items()}
    behind_stray, behind_wall = ever["off"][1::2][stray], ever["off"][1::2][~stray]
    print("odd robots ever stopped, behind a stray return: %.3f without the filter, %.3f with; behind a wall: %.3f, %.3f; even "
          "robots: %.3f, %.3f" % (behind_stray.mean(), ever["G = 2"][1::2][stray].mean(), behind_wall.mean(),
                                  ever["G = 2"][1::2][~stray].mean(), ever["off"][0::2].mean(), ever["G = 2"][0::2].mean()))
    layer, d = marks["G = 2"]
    assert (layer == 254).sum() > (d == 254).sum() > 0 and np.array_equal(d, ref.denoise(layer, world, 2, 8))
    assert behind_stray.all() and behind_wall.all()
    assert not ever["G = 2"][1::2][stray].any() and ever["G = 2"][1::2][~stray].all()
