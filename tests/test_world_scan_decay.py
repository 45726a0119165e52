"""The decay of the fleet's shared obstacle layer (K14): a mark that no scan update has made again for max_age scan updates
becomes unknown_value in the layer itself, behind every mark and in front of the footprint clearing.

The contract is step 2b of the text in include/neo_mpc.h (neo_mpc_fleet_clear, neo_mpc_set_world_scan_decay) and its executable
form the transcription in tests/world_decay_reference.py, composed with tests/world_scan_layer_reference.py for the rays, the
marks and the footprints and with tests/world_denoise_reference.py for D and `live`.  The step is integers only: every
comparison is exact equality of uint8 cells and uint32 ages -- no tolerance, no dropped case."""
import collections
import functools
import math
import re

import numpy as np
import pytest

from neo_mpc_planner2_amd import _lib, abi
from tests import rolling_window_reference as roll_ref
from tests import world_decay_reference as ref
from tests import world_denoise_reference as denoise_ref
from tests import world_scan_layer_reference as world_ref
from tests.c_probe import HEADER, kernel_resources, run_c_probe
from tests.fleet_kit import (F32, FAR, RECT, capture, cell_centre, denoised_of, eager_on_side_stream, gpu, inflation_for,
                             pairs_fleet, rectangle, rolled_pool, same, scanner, world_state)
from tests.world_scan_cases import WORLDS

ENTRY_POINTS = ("neo_mpc_set_world_scan_decay", "neo_mpc_get_world_scan_ages")
CLEAR, MARK = world_ref.CLEAR, world_ref.MARK
SCAN = CLEAR | MARK
NO_AGE = ref.NO_AGE
DECAY_WORLDS = ("130x67-2.5cm", "40x40-10cm")       # 8710 cells: a tail of 6 behind the 16-cell groups; 1600: none
AGES = (1, 2, 5)
#: the seven updates of the equality tests: scan, scan with other points (some marks made again, some not), none, rays alone,
#: marks alone, scan, scan
SEQUENCE = (SCAN, SCAN, 0, CLEAR, MARK, SCAN, SCAN)
NONE = dict(flags=0, **FAR)


# ------------------------------------------------------------------------------------------ 1: the rule by hand
@pytest.mark.parametrize("unknown", (255, 0))
def test_the_rule_by_hand(unknown):
    """An 8 x 8 world of 1 m cells, the sensor in cell (0, 0), a = (5, 1), b = (2, 5), R = 0; the table of the contract, for
    both forms of the transcription, and with A = 1."""
    world = np.full((8, 8), 7, dtype=np.uint8)
    sensor = np.array([[0.5, 0.5]])
    a, b = (5, 1), (2, 5)
    both, only_a = np.array([[cell_centre(*a), cell_centre(*b)]]), np.array([[cell_centre(*a)]])
    along_row_0 = np.array([[cell_centre(6, 0)]])                       # a ray through neither
    for by_definition in (False, True):
        model = ref.DecayingWorldScanLayer(2, by_definition=by_definition)

        def update(points=None, flags=0):
            live = model.update(world, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, points=points, sensor_origins=sensor, flags=flags,
                                unknown_value=unknown, **FAR)
            ages = model.ages()
            assert ((ages != NO_AGE) == (model.layer == 254)).all()
            return model.layer.copy(), ages, live

        layer, ages, live = update(both, SCAN)
        assert (layer[a[1], a[0]], layer[b[1], b[0]]) == (254, 254) and (ages[a[1], a[0]], ages[b[1], b[0]]) == (0, 0)
        assert (layer == 254).sum() == 2 and live[b[1], b[0]] == 254
        layer, ages, live = update(only_a, SCAN)
        assert (layer[a[1], a[0]], layer[b[1], b[0]]) == (254, 254) and (ages[a[1], a[0]], ages[b[1], b[0]]) == (0, 1)
        held = (layer, ages, live)
        assert same(update(), held)                                     # flags == 0: unchanged
        layer, ages, live = update(along_row_0, CLEAR)                  # CLEAR alone, the ray not through b: the marks unchanged
        assert np.array_equal(ages, held[1]) and (layer[0, :6] == 0).all() and (layer == 254).sum() == 2
        layer, ages, live = update(only_a, SCAN)
        assert layer[a[1], a[0]] == 254 and ages[a[1], a[0]] == 0
        assert layer[b[1], b[0]] == unknown and ages[b[1], b[0]] == NO_AGE and live[b[1], b[0]] == 7   # the world shows through
        assert (layer == 254).sum() == 1
        # A = 1: b is gone after the second update
        model = ref.DecayingWorldScanLayer(1, by_definition=by_definition)
        assert update(both, SCAN)[0][b[1], b[0]] == 254
        layer, ages, live = update(only_a, SCAN)
        assert layer[b[1], b[0]] == unknown and layer[a[1], a[0]] == 254 and ages[a[1], a[0]] == 0


# ------------------------------------------------------------------------------------------ 2: the two forms agree
def test_the_two_forms_agree_on_random_sequences_and_across_the_wrap_of_the_clock():
    """Random sequences of scan updates, updates without a scan and clears on a 9 x 13 layer, by both forms, the clock
    started at 0 and three scan updates below 2^32: the four runs agree after every update in the layer and in the ages."""
    rng = np.random.default_rng(1401)
    stats = collections.Counter()
    for max_age in (1, 2, 5):
        for unknown in (255, 0):
            runs = [dict(form=form, clock=start, layer=np.full((9, 13), unknown, dtype=np.uint8),
                         stamp=np.full((9, 13), start, dtype=np.uint32))
                    for form in (ref.step_by_definition, ref.step) for start in (0, ref.WRAP - 3)]
            for k in range(40):
                kind = rng.choice(["scan", "none", "clear"], p=[0.6, 0.2, 0.2])
                cleared, marked = rng.random((9, 13)) < 0.1, rng.random((9, 13)) < 0.15
                got = []
                for r in runs:
                    if kind != "none":
                        r["layer"][cleared] = 0
                    if kind == "scan":
                        r["layer"][marked] = 254
                    extra = (stats,) if r["form"] is ref.step_by_definition else ()
                    r["clock"] = r["form"](r["layer"], r["stamp"], r["clock"], marked, max_age, unknown, kind == "scan", *extra)
                    got.append((r["layer"], ref.ages(r["layer"], r["stamp"], r["clock"])))
                for other in got[1:]:
                    assert same(other, got[0]), (max_age, unknown, k)
                ages = got[0][1]
                assert (ages[got[0][0] == 254] < max_age).all() and (ages[got[0][0] != 254] == NO_AGE).all()
            assert runs[1]["clock"] < 100 < runs[0]["clock"] + 100      # the second clock went through 2^32
    print(dict(stats))
    for name in ("decay: a scan update advances the clock", "decay: the clock wraps", "decay: an update that is no scan update",
                 "decay: a mark is stamped", "decay: a mark expires", "decay: a mark is young enough",
                 "decay: an age across the wrap"):
        assert stats[name] > 0, name


# ------------------------------------------------------------------------------------------ 3: entry points, the kernels' resources
def test_entry_points_constant_and_refusals_without_a_handle(tmp_path):
    got = run_c_probe(tmp_path, '#include <stdio.h>\n#include "neo_mpc.h"\n'
                      'int main(void) {\n  printf("no_age %u\\n", NEO_MPC_NO_AGE);\n'
                      '  int (*set)(neo_mpc_handle*, uint32_t) = neo_mpc_set_world_scan_decay;\n'
                      '  int (*get)(neo_mpc_handle*, uint32_t*) = neo_mpc_get_world_scan_ages;\n'
                      '  void* volatile f[2] = {(void*)set, (void*)get};\n  return f[0] == 0 || f[1] == 0;\n}\n')
    assert int(got["no_age"]) == abi.NO_AGE == ref.NO_AGE == 0xFFFFFFFF
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\s*\(" % name, text), name
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert "#define NEO_MPC_ABI_VERSION 2" in text and "#define NEO_MPC_BEHAVIOUR_VERSION 6" in text
    assert lib.neo_mpc_abi_version() == 2 and lib.neo_mpc_behaviour_version() == 6
    for max_age in (0, 1, 50, 0xFFFFFFFF):
        assert lib.neo_mpc_set_world_scan_decay(None, max_age) == -1
        assert lib.neo_mpc_last_error_code() == -1
    assert lib.neo_mpc_get_world_scan_ages(None, None) == -1


def test_the_new_kernels_are_scratch_free(tmp_path):
    rows = kernel_resources(tmp_path, '#include "world_scan_decay.h"\n')
    mine = {name: row for name, row in rows.items() if "k_world_scan_" in name}
    for kernel in ("k_world_scan_tick", "k_world_scan_stamp_fill", "k_world_scan_marks_stamped", "k_world_scan_decay"):
        row = [r for name, r in mine.items() if kernel + "E" in name]
        assert len(row) == 1, (kernel, sorted(mine))
        assert row[0]["ScratchSize"] == 0 and row[0]["VGPRs"] <= 32, (kernel, row[0])
    assert len(mine) == 4, sorted(mine)


# ------------------------------------------------------------------------------------------ the generator
def square(x, y, half):
    return rectangle(x - half, y - half, x + half, y + half)


@functools.lru_cache(maxsize=None)
def decay_case(world, robots):
    """(cells [sy, sx], wox, woy, sensors [robots, 2], polygons [robots, 4, 2], per update of SEQUENCE points [robots, 24, 2] or
    None).  Points in random cells of the world; half of an update's points are those of the update before it; the first and the
    sixth update mark the world's last two cells, which the second and the seventh do not mark again."""
    sx, sy, res = WORLDS[world]
    rng = np.random.default_rng(1400 + sx + robots)
    cells = rng.choice(np.array([0, 0, 0, 0, 60, 150, 253, 254, 255, 255, 255], dtype=np.uint8), size=(sy, sx))
    wox, woy = (float(v) for v in rng.uniform(-5.0, 5.0, size=2))
    span = np.array([sx * res, sy * res])
    sensors = np.array([wox, woy]) + span * rng.uniform(0.3, 0.7, size=(robots, 2))
    polygons = np.array([square(x, y, 2.2 * res) for x, y in sensors])

    def pick(keep=None, tail=False):
        at = np.stack([rng.integers(0, sx, size=(robots, 24)), rng.integers(0, sy, size=(robots, 24))], -1)
        if tail:                                                    # the last cells of the world: the sweep's tail where it has one
            at[0, 0], at[0, 1] = (sx - 1, sy - 1), (sx - 2, sy - 1)
        points = np.array([wox, woy]) + (at + 0.5 + rng.uniform(-0.4, 0.4, size=at.shape)) * res
        if keep is not None:
            points[:, 12:] = keep[:, 12:]
        return points

    first = pick(tail=True)
    second = pick(first)
    rays, alone = pick(), pick(second)
    third = pick(alone, tail=True)
    fourth = pick(third)
    updates = (first, second, None, rays, alone, third, fourth)
    for a in (cells, sensors, polygons) + tuple(u for u in updates if u is not None):
        a.setflags(write=False)
    return cells, wox, woy, sensors, polygons, updates


def settings_of(robots):
    """(G, unknown_value) of a case: the filter on and unknown 0 with three robots."""
    return (2, 0) if robots == 3 else (0, 255)


def model_state(model, live):
    return model.layer.copy(), live.copy(), model.denoised.copy(), model.ages()


@functools.lru_cache(maxsize=None)
def expected(world, reach, max_age, robots):
    """The transcription on a case: (layer, live, D, ages) after every update of SEQUENCE."""
    cells, wox, woy, sensors, polygons, updates = decay_case(world, robots)
    res = WORLDS[world][2]
    group, unknown = settings_of(robots)
    model, out = ref.DecayingWorldScanLayer(max_age, group, 8), []
    for points, flags in zip(updates, SEQUENCE):
        live = model.update(cells, res, wox, woy, *inflation_for(reach, res), points=points, sensor_origins=sensors, flags=flags,
                            clear=dict(polygons=polygons, padding=0.5 * res), unknown_value=unknown, **FAR)
        out.append(model_state(model, live))
    return out


def device_state(s):
    """(layer, live, D, ages) of the handle."""
    layer, live = world_state(s)
    return layer, live, denoised_of(s), s.get_world_scan_ages()


def differing(got, want):
    return [int((a != b).sum()) for a, b in zip(got, want)]


def test_the_case_expires_marks_keeps_marks_and_reaches_the_tail():
    """What the equality tests rest on: with A = 1 and 2 marks expire, with A = 5 the marks of the first update reach the age
    of 4 and stay, marks of earlier updates survive, and the 130 x 67 world has marks in the six cells behind its last group of
    sixteen, which expire there."""
    for world in DECAY_WORLDS:
        sx, sy, _ = WORLDS[world]
        assert (sx * sy) % 16 == (6 if world == "130x67-2.5cm" else 0)
        for max_age in AGES:
            want = expected(world, 0, max_age, 1)
            marks = [(layer == 254).sum() for layer, _, _, _ in want]
            oldest = [int(ages[ages != NO_AGE].max()) for _, _, _, ages in want]
            assert max(oldest) == max_age - 1 and all(m > 0 for m in marks), (world, max_age, oldest)
            assert want[0][0][sy - 1, sx - 1] == 254 and want[0][0][sy - 1, sx - 2] == 254
            forever = expected(world, 0, 1000, 1)
            expired = any(((a[0] == 254) & (b[0] != 254)).any() for a, b in zip(forever, want))
            assert expired is (max_age < 5), (world, max_age)            # (five scan updates: with A = 5 the oldest mark is 4)
            assert same(want[2], want[1])                                # flags == 0 changes nothing
    tail = expected("130x67-2.5cm", 0, 1, 1)
    assert tail[0][0][66, 129] == 254 and tail[1][0][66, 129] == 255 and tail[5][0][66, 128] == 254 and tail[6][0][66, 128] == 255
    # (A = 1: a scan update leaves its own marks alone)
    assert (expected("40x40-10cm", 0, 1, 1)[1][3][expected("40x40-10cm", 0, 1, 1)[1][0] == 254] == 0).all()


# ------------------------------------------------------------------------------------------ 4: equality with the transcription
CASES = [(w, r, a, n) for w in DECAY_WORLDS for r in (0, 3) for a in AGES for n in (1, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("world,reach,max_age,robots", CASES, ids=["%s-R%d-A%d-%drobots" % c for c in CASES])
def test_decaying_updates_equal_the_transcription(world, reach, max_age, robots):
    from neo_mpc_planner2_amd.solver import BatchSolver
    sx, sy, res = WORLDS[world]
    cells, wox, woy, sensors, polygons, updates = decay_case(world, robots)
    want = expected(world, reach, max_age, robots)
    group, unknown = settings_of(robots)
    params = inflation_for(reach, res)
    with BatchSolver({}) as s:
        s.set_world_scan_decay(max_age)
        s.set_world_scan_denoise(group)
        for put in (gpu, np.array):                                       # the device and the host variants
            s.set_world_map(put(cells), res, wox, woy)
            s.reset_world_scan_layer()
            for k, (points, flags) in enumerate(zip(updates, SEQUENCE)):
                kw = dict(flags=flags, clear=dict(polygons=put(polygons), padding=0.5 * res), unknown_value=unknown, **FAR)
                if points is not None:
                    kw.update(points=put(points), sensor_origins=put(sensors))
                elif put is gpu:
                    kw.update(on_device=True)
                s.update_world_scan_layer(*params, **kw)
                got = device_state(s)
                assert same(got, want[k]), (put.__name__, k, differing(got, want[k]))
            assert np.array_equal(s.get_world_map()[0], cells)            # the static map is what it was
    print("%s R=%d A=%d %d robots: marks after each update %s" % (world, reach, max_age, robots,
                                                                  [int((w[0] == 254).sum()) for w in want]))


LASER_SCANNERS = [scanner((0.02, 0.01, 0.2), -1.6, 3.2 / 29, 0.01, 50.0), scanner((-0.02, -0.01, 3.0), -1.6, 3.2 / 29, 0.01, 50.0)]
RANGE_CASES = [(w, a) for w in DECAY_WORLDS for a in AGES]


@pytest.mark.gpu
@pytest.mark.parametrize("world,max_age", RANGE_CASES, ids=["%s-A%d" % c for c in RANGE_CASES])
def test_decaying_updates_from_ranges_equal_the_transcription(world, max_age):
    """SEQUENCE from ranges, three robots with two scanners of 30 beams each at fixed poses, R = 3, G = 2: half of an update's
    ranges are those of the update before it, so those marks are made again.  The transcription is fed with the points the
    device projected, as in tests/test_world_scan_layer.py."""
    import torch
    from neo_mpc_planner2_amd.solver import BatchSolver
    sx, sy, res = WORLDS[world]
    cells, wox, woy, sensors, polygons, _ = decay_case(world, 3)
    params = inflation_for(3, res)
    rng = np.random.default_rng(1450 + sx + max_age)
    poses = np.concatenate([sensors, rng.uniform(-3.0, 3.0, size=(3, 1))], 1)
    ranges, last = [], None
    for flags in SEQUENCE:
        now = rng.uniform(0.05, 0.45, size=(3, 2, 30)) * max(sx, sy) * res
        now[:, :, 5] = np.inf                                             # (no INF_IS_VALID: nothing)
        if last is not None:
            now[:, :, 15:] = last[:, :, 15:]
        last = now
        ranges.append(now.astype(F32) if flags else None)
    clear = dict(polygons=polygons, padding=0.5 * res)
    with BatchSolver({}) as s:
        s.set_world_scan_decay(max_age)
        s.set_world_scan_denoise(2)
        expired = 0
        for put in (gpu, np.array):
            model = ref.DecayingWorldScanLayer(max_age, 2, 8)
            s.set_world_map(put(cells), res, wox, woy)
            s.reset_world_scan_layer()
            for k, (r, flags) in enumerate(zip(ranges, SEQUENCE)):
                if r is None:
                    s.update_world_scan_layer(*params, clear=dict(polygons=put(polygons), padding=0.5 * res),
                                              **(dict(on_device=True) if put is gpu else {}), **NONE)
                    live = model.update(cells, res, wox, woy, *params, clear=clear, **NONE)
                else:
                    points, origins = s.project_laser(gpu(r), gpu(poses), LASER_SCANNERS)
                    torch.cuda.synchronize()
                    points, origins = points.cpu().numpy(), origins.cpu().numpy()
                    s.update_world_scan_layer_from_ranges(*params, put(r), put(poses), LASER_SCANNERS, flags=flags,
                                                          clear=dict(polygons=put(polygons), padding=0.5 * res), **FAR)
                    before = model.layer
                    live = model.update(cells, res, wox, woy, *params, points=points, sensor_origins=origins, flags=flags,
                                        clear=clear, **FAR)
                    if before is not None:
                        expired += int(((before == 254) & (model.layer == 255)).sum())
                got, want = device_state(s), model_state(model, live)
                assert same(got, want), (put.__name__, k, differing(got, want))
        assert (expired > 0) is (max_age < 5) and (model.layer == 254).any()   # (five scan updates: with A = 5 nothing is old enough)


# ------------------------------------------------------------------------------------------ hand-made worlds for what follows
def marks_at(*at):
    """Points [1, n, 2] at the centres of the 1 m cells `at`."""
    return np.array([[cell_centre(i, l) for i, l in at]])


class Pair:
    """A handle and the transcription side by side on a world of 1 m cells at the origin: every update goes to both, and the
    handle's layer, live, D and ages must equal the transcription's."""

    def __init__(self, s, put, world, params=(0.0, 0.0, 1.0), max_age=0, group=0, unknown=255):
        self.s, self.put, self.world, self.params, self.unknown = s, put, world, params, unknown
        self.sensor = np.array([[20.5, 20.5]])
        self.model = ref.DecayingWorldScanLayer(max_age, group, 8)
        s.set_world_scan_decay(max_age)
        s.set_world_scan_denoise(group)
        s.set_world_map(put(world), 1.0, 0.0, 0.0)
        s.reset_world_scan_layer()

    def set_decay(self, max_age):
        self.s.set_world_scan_decay(max_age)
        self.model.set_decay(max_age)

    def update(self, points=None, flags=0, clear=None):
        kw = dict(flags=flags, unknown_value=self.unknown, **FAR)
        mine = dict(kw)
        if points is not None:
            kw.update(points=self.put(points), sensor_origins=self.put(self.sensor))
            mine.update(points=points, sensor_origins=self.sensor)
        elif self.put is gpu:
            kw.update(on_device=True)
        if clear is not None:
            kw.update(clear=dict(polygons=self.put(clear["polygons"]), padding=clear["padding"]))
            mine.update(clear=clear)
        self.s.update_world_scan_layer(*self.params, **kw)
        live = self.model.update(self.world, 1.0, 0.0, 0.0, *self.params, **mine)
        layer, got_live = world_state(self.s)
        assert same((layer, got_live, denoised_of(self.s)), (self.model.layer, live, self.model.denoised))
        if self.model.decaying:
            ages = self.s.get_world_scan_ages()
            assert np.array_equal(ages, self.model.ages())
            return layer, got_live, ages
        assert self.s._lib.neo_mpc_get_world_scan_ages(self.s._handle, None) == -5
        return layer, got_live, None


def at(array, cell):
    return int(array[cell[1], cell[0]])


X, Y = (30, 12), (31, 12)
ELSEWHERE = marks_at((5, 30))                                           # a ray from (20, 20) away from X and Y


# ------------------------------------------------------------------------------------------ 5: exactness of the age
@pytest.mark.gpu
@pytest.mark.parametrize("max_age", (1, 3))
def test_a_mark_is_there_after_max_age_minus_one_further_scan_updates_and_gone_after_max_age(max_age):
    """X is marked by every scan update and never expires; its neighbour Y, marked once, is there after A - 1 further scan
    updates and gone after A, whatever updates without a scan and with rays alone lie between."""
    from neo_mpc_planner2_amd.solver import BatchSolver
    world = np.zeros((40, 40), dtype=np.uint8)
    with BatchSolver({}) as s:
        for put in (gpu, np.array):
            p = Pair(s, put, world, max_age=max_age)
            layer, _, ages = p.update(marks_at(X, Y), MARK)
            assert at(layer, X) == 254 and at(layer, Y) == 254 and at(ages, Y) == 0
            for further in range(1, max_age + 1):
                for points, flags in ((None, 0), (ELSEWHERE, CLEAR), (None, 0)):
                    layer, _, ages = p.update(points, flags)
                    assert at(layer, Y) == 254 and at(ages, Y) == further - 1 and at(ages, X) == 0
                layer, _, ages = p.update(marks_at(X), MARK)
                assert at(layer, X) == 254 and at(ages, X) == 0
                if further < max_age:
                    assert at(layer, Y) == 254 and at(ages, Y) == further
                else:
                    assert at(layer, Y) == 255 and at(ages, Y) == NO_AGE
            for _ in range(3):                                           # ... and X goes on
                layer, _, ages = p.update(marks_at(X), SCAN)
                assert at(layer, X) == 254 and at(ages, X) == 0 and (layer == 254).sum() == 1


# ------------------------------------------------------------------------------------------ 6: off is the update as it was
@pytest.mark.gpu
def test_off_is_the_update_as_it_was_and_the_ages_getter_refuses():
    from neo_mpc_planner2_amd.solver import BatchSolver
    world_name, robots = "130x67-2.5cm", 3
    sx, sy, res = WORLDS[world_name]
    cells, wox, woy, sensors, polygons, updates = decay_case(world_name, robots)
    params = inflation_for(3, res)
    for group in (0, 2):                                                  # K12's transcription, and K13's
        model, want = denoise_ref.DenoisedWorldScanLayer(group, 8), []
        for points, flags in zip(updates, SEQUENCE):
            live = model.update(cells, res, wox, woy, *params, points=points, sensor_origins=sensors, flags=flags,
                                clear=dict(polygons=polygons, padding=0.5 * res), **FAR)
            want.append((model.layer.copy(), live.copy(), model.denoised.copy()))
        if group == 0:
            plain = world_ref.WorldScanLayer()
            for (points, flags), w in zip(zip(updates, SEQUENCE), want):
                live = plain.update(cells, res, wox, woy, *params, points=points, sensor_origins=sensors, flags=flags,
                                    clear=dict(polygons=polygons, padding=0.5 * res), **FAR)
                assert same((plain.layer, live), w[:2])
        for setting in (None, 0, (7, 0)):                                 # never set, set to 0, on and off again before any update
            with BatchSolver({}) as s:
                for max_age in (() if setting is None else np.atleast_1d(setting)):
                    s.set_world_scan_decay(int(max_age))
                s.set_world_scan_denoise(group)
                assert s._lib.neo_mpc_get_world_scan_ages(s._handle, None) == -4       # no layer
                s.set_world_map(gpu(cells), res, wox, woy)
                for k, (points, flags) in enumerate(zip(updates, SEQUENCE)):
                    kw = dict(flags=flags, clear=dict(polygons=gpu(polygons), padding=0.5 * res), **FAR)
                    if points is not None:
                        kw.update(points=gpu(points), sensor_origins=gpu(sensors))
                    else:
                        kw.update(on_device=True)
                    s.update_world_scan_layer(*params, **kw)
                    got = world_state(s) + (denoised_of(s),)
                    assert same(got, want[k]), (group, setting, k, differing(got, want[k]))
                    assert s._lib.neo_mpc_get_world_scan_ages(s._handle, None) == -5   # a layer, and no ages
                    assert s._lib.neo_mpc_last_error_code() == -5


@pytest.mark.gpu
def test_on_off_on_treats_the_marks_present_as_new_and_the_setting_survives_resets():
    from neo_mpc_planner2_amd.solver import BatchSolver
    world = np.zeros((40, 40), dtype=np.uint8)
    with BatchSolver({}) as s:
        for put in (gpu, np.array):
            p = Pair(s, put, world, max_age=2)
            p.update(marks_at(X, Y), MARK)
            layer, _, ages = p.update(marks_at(X), MARK)
            assert at(ages, X) == 0 and at(ages, Y) == 1
            held = world_state(s)
            p.set_decay(0)
            assert same(world_state(s), held)                               # the setter itself changes nothing ...
            assert np.array_equal(s.get_world_scan_ages(), ages)         # ... and the last update still ran with decay
            layer, _, ages = p.update()                                  # off: Pair.update checks that the getter refuses
            assert ages is None and at(layer, Y) == 254
            p.update(marks_at(X), MARK)                                  # a scan update with decay off: Y would have expired
            p.set_decay(2)
            layer, _, ages = p.update()
            assert at(ages, X) == 0 and at(ages, Y) == 0                 # both count as made by the last scan update
            layer, _, ages = p.update(marks_at(X), MARK)
            assert at(ages, Y) == 1
            layer, _, ages = p.update(marks_at(X), MARK)
            assert at(layer, Y) == 255 and at(layer, X) == 254
            # the setting survives a reset of the layer and a new world map
            s.reset_world_scan_layer()
            s.set_world_map(put(world), 1.0, 0.0, 0.0)
            p.model.reset()
            layer, _, ages = p.update(marks_at(Y), MARK)
            assert at(ages, Y) == 0 and (layer == 254).sum() == 1
            p.update(marks_at(X), MARK)
            layer, _, ages = p.update(marks_at(X), MARK)
            assert at(layer, Y) == 255 and at(ages, X) == 0


# ------------------------------------------------------------------------------------------ 7: marks made with decay off
@pytest.mark.gpu
def test_marks_made_with_decay_off_expire_max_age_scan_updates_after_it_comes_on():
    from neo_mpc_planner2_amd.solver import BatchSolver
    world = np.zeros((40, 40), dtype=np.uint8)
    with BatchSolver({}) as s:
        for put in (gpu, np.array):
            p = Pair(s, put, world, max_age=0)
            for _ in range(4):                                           # scan updates nobody counts
                layer, _, ages = p.update(marks_at(X), MARK)
            p.update(marks_at(Y), MARK)
            assert ages is None
            p.set_decay(3)
            for k in (1, 2):
                layer, _, ages = p.update(ELSEWHERE, MARK)
                assert at(layer, X) == 254 and at(layer, Y) == 254 and at(ages, X) == k and at(ages, Y) == k
            layer, _, ages = p.update(ELSEWHERE, MARK)
            assert at(layer, X) == 255 and at(layer, Y) == 255 and (layer == 254).sum() == 1


# ------------------------------------------------------------------------------------------ 8: max_age lowered and raised
@pytest.mark.gpu
def test_a_lowered_max_age_acts_with_the_next_update_without_a_scan_and_a_raised_one_brings_nothing_back():
    from neo_mpc_planner2_amd.solver import BatchSolver
    world = np.zeros((40, 40), dtype=np.uint8)
    first, second, third = (3, 3), (10, 25), (39, 39)
    with BatchSolver({}) as s:
        for put in (gpu, np.array):
            p = Pair(s, put, world, max_age=5)
            p.update(marks_at(first), MARK)
            p.update(marks_at(second), MARK)
            p.update(marks_at(third), MARK)
            layer, _, ages = p.update(marks_at(third), MARK)
            assert [at(ages, c) for c in (first, second, third)] == [3, 2, 0] and (layer == 254).sum() == 3
            p.set_decay(2)
            layer, _, ages = p.update()                                  # flags == 0
            assert [at(layer, c) for c in (first, second, third)] == [255, 255, 254] and at(ages, third) == 0
            held = world_state(s)
            p.set_decay(10)
            layer, _, ages = p.update()
            assert same(world_state(s), held) and at(ages, third) == 0      # nothing comes back, nothing else goes
            layer, _, ages = p.update(marks_at(first), MARK)
            assert [at(ages, c) for c in (first, third)] == [0, 1] and at(layer, second) == 255


# ------------------------------------------------------------------------------------------ 9: what live shows
@pytest.mark.gpu
@pytest.mark.parametrize("unknown", (255, 0))
def test_under_an_expired_mark_live_is_the_composition_without_it_and_its_ring_is_gone(unknown):
    """Marks over a world cell that is 0, one that is 255 and one that the world map's own inflation raised to 120; R = 3.
    While they stand each has its ring in live; once they have expired live is, everywhere, what an update of a layer that
    never held them composes -- the static map's cell where unknown_value is 255 or the cell is not 255 (updateWithMax puts
    an unknown_value of 0 over a world cell of 255, marked or not)."""
    from neo_mpc_planner2_amd.solver import BatchSolver
    world = np.zeros((40, 40), dtype=np.uint8)
    world[5:9, 20:30] = 255
    world[30, 5:35] = 254
    world[28:33, 5:35][world[28:33, 5:35] == 0] = 120
    free, unknown_cell, inflated = (10, 15), (25, 7), (12, 28)
    params = (0.5, 2.5, 1.0)
    with BatchSolver({}) as s:
        for put in (gpu, np.array):
            p = Pair(s, put, world, params=params, max_age=1, unknown=unknown)
            never = p.update()[1]                                        # a layer of unknown_value alone
            layer, live, _ = p.update(marks_at(free, unknown_cell, inflated), MARK)
            for c in (free, unknown_cell, inflated):
                assert at(layer, c) == 254 and at(live, c) == 254
            ring = live != never
            assert ring.sum() >= 3 and 0 < at(live, (free[0] + 2, free[1])) < 253
            layer, live, _ = p.update(marks_at((0, 39)), MARK)
            assert same((live[:, 4:],), (never[:, 4:],)) and not (layer[:, 4:] == 254).any()   # (column 0 holds the new mark)
            for c in (free, inflated):
                assert at(live, c) == at(world, c) and at(layer, c) == unknown
            assert at(live, unknown_cell) == (255 if unknown == 255 else 0)


# ------------------------------------------------------------------------------------------ 10: order
@pytest.mark.gpu
def test_the_survivor_of_a_pair_whose_partner_expired_is_a_lone_mark_to_the_filter():
    from neo_mpc_planner2_amd.solver import BatchSolver
    world = np.zeros((40, 40), dtype=np.uint8)
    with BatchSolver({}) as s:
        for put in (gpu, np.array):
            p = Pair(s, put, world, params=(0.5, 2.5, 1.0), max_age=2, group=2)
            layer, live, _ = p.update(marks_at(X, Y), MARK)
            assert at(live, X) == 254 and at(live, Y) == 254
            layer, live, _ = p.update(marks_at(X), MARK)
            assert at(live, X) == 254 and at(live, Y) == 254             # Y at age 1: still a pair
            layer, live, ages = p.update(marks_at(X), MARK)
            d = denoised_of(s)
            assert at(layer, Y) == 255 and at(layer, X) == 254 and at(ages, X) == 0
            assert at(d, X) == 0 and not live.any()                      # X stays in the layer and is free in D: no ring either


@pytest.mark.gpu
def test_the_footprint_clearing_runs_behind_the_expiry_of_the_same_update():
    """A = 1, unknown_value 255.  Update 1 marks P and Q.  Update 2 marks Z and W and clears an outline over P and Z: P expired
    AND was cleared, and is 0 -- the clearing is the later step; Q expired outside the outline and is 255; Z was marked now
    and cleared: 0; W stays."""
    from neo_mpc_planner2_amd.solver import BatchSolver
    world = np.zeros((40, 40), dtype=np.uint8)
    P, Q, Z, W = (11, 11), (30, 30), (12, 12), (31, 5)
    clear = dict(polygons=np.array([rectangle(10.1, 10.1, 12.9, 12.9)]), padding=0.0)
    with BatchSolver({}) as s:
        for put in (gpu, np.array):
            p = Pair(s, put, world, max_age=1)
            p.update(marks_at(P, Q), MARK)
            layer, live, ages = p.update(marks_at(Z, W), MARK, clear=clear)
            assert [at(layer, c) for c in (P, Q, Z, W)] == [0, 255, 0, 254]
            assert (layer == 0).sum() == 9 and (layer == 254).sum() == 1 and at(ages, W) == 0


@pytest.mark.gpu
def test_the_roll_cuts_its_windows_from_the_decayed_map():
    from neo_mpc_planner2_amd.solver import BatchSolver
    world = np.zeros((40, 40), dtype=np.uint8)
    params = (0.5, 2.5, 1.0)
    poses = np.array([(30.2, 12.3, 0.0)])
    size = 16
    start = poses[:, :2] - size / 2 + 0.013
    with BatchSolver({}) as s:
        p = Pair(s, gpu, world, params=params, max_age=1)
        _, live, _ = p.update(marks_at(X, Y), MARK)
        want = roll_ref.roll(live, 1.0, 0.0, 0.0, start, size, size, 1.0, poses=poses, outside_value=255)
        pool, origins = rolled_pool(s, size, size, 1.0, start.copy(), poses)
        assert origins.tolist() == want[0].tolist() and np.array_equal(pool, want[1]) and (pool == 254).sum() == 2
        _, live, _ = p.update(marks_at(X), MARK)
        want = roll_ref.roll(live, 1.0, 0.0, 0.0, start, size, size, 1.0, poses=poses, outside_value=255)
        pool, origins = rolled_pool(s, size, size, 1.0, start.copy(), poses)
        assert np.array_equal(pool, want[1]) and (pool == 254).sum() == 1
        lone = world_ref.WorldScanLayer().update(world, 1.0, 0.0, 0.0, *params, points=marks_at(X), sensor_origins=p.sensor,
                                                 flags=MARK, **FAR)
        assert np.array_equal(live, lone)                                # Y's ring went with it


# ------------------------------------------------------------------------------------------ 11: graph capture
@pytest.mark.gpu
def test_a_captured_update_that_is_replayed_advances_the_clock():
    """World scan from ranges -> roll, captured once behind one eager call, A = 3.  One robot, one scanner of two beams: beam 0
    keeps returning from cell X, beam 1 returned from cell Y in the eager call and never again.  Y is there after replay
    A - 1 and gone after replay A; X stays.  A clock on the host, or one passed as a kernel argument, is frozen at capture."""
    import torch
    from neo_mpc_planner2_amd.solver import BatchSolver
    max_age, size = 3, 32
    world = np.zeros((40, 40), dtype=np.uint8)
    two_beams = [scanner((0.0, 0.0, 0.0), 0.0, math.pi / 2, 0.05, 30.0)]
    poses = gpu(np.array([(10.5, 10.5, 0.0)]))
    ranges = gpu(np.array([[[5.0, 7.0]]], dtype=F32))                     # (15, 10) and (10, 17)
    origins = gpu(np.array([(10.5 - size / 2 + 0.013, 10.5 - size / 2 + 0.013)]))
    cx, cy = (15, 10), (10, 17)
    with BatchSolver({}) as s:
        s.set_world_scan_decay(max_age)
        s.set_world_map(gpu(world), 1.0, 0.0, 0.0)

        def tick():
            s.update_world_scan_layer_from_ranges(0.0, 0.0, 1.0, ranges, poses, two_beams, **FAR)
            s.roll_costmap_pool(size, size, 1.0, origins, poses=poses)

        def seen():
            torch.cuda.synchronize()
            layer, live = s.get_world_scan_layer()
            return layer, s.get_world_scan_ages(), s.get_costmap_pool()[0]

        side = eager_on_side_stream(tick)                                # (it allocates)
        layer, ages, pool = seen()
        assert at(layer, cx) == 254 and at(layer, cy) == 254 and at(ages, cx) == 0 and at(ages, cy) == 0
        assert (layer == 254).sum() == 2 and (pool == 254).sum() == 2
        g = capture(tick, side)
        ranges.copy_(gpu(np.array([[[5.0, np.inf]]], dtype=F32)))        # (no INF_IS_VALID: beam 1 is nothing, not even a ray)
        torch.cuda.synchronize()
        for replay in range(1, max_age + 2):
            g.replay()
            layer, ages, pool = seen()
            assert at(layer, cx) == 254 and at(ages, cx) == 0, replay
            if replay < max_age:
                assert at(layer, cy) == 254 and at(ages, cy) == replay and (pool == 254).sum() == 2, replay
            else:
                assert at(layer, cy) == 255 and at(ages, cy) == NO_AGE and (pool == 254).sum() == 1, replay


# ------------------------------------------------------------------------------------------ 12: the closed loop
@pytest.mark.gpu
def test_closed_loop_a_wall_seen_once_lets_the_robots_go_again_and_a_wall_seen_every_tick_does_not():
    """64 robots in 32 pairs on a free world map, fleet_kit.pairs_fleet with 161 beams: the even robot of a pair stands
    1.5 m behind the odd one and its front scanner looks at it.  Its ranges hold a short wall 0.15 m in front of the odd robot's
    centre, from 0.2 m to 0.4 m to its LEFT: it crosses the left edge of that robot's outline, so its footprint gate reads 254
    and the robot is stopped for that tick, and it lies more than the inscribed ring away from the line the robot's own
    rollout runs along, so the latch of py:338-341, which holds for three seconds, is not what stops it.  In half of the
    pairs the wall is in the ranges of the first tick only and every later beam is invalid, so that no ray clears it; in
    the other half it is in every tick's ranges.  Every tick is a scan update.  Without decay every odd robot is stopped to
    the last tick.  With A = 3 the mark of tick 0 is in the layer after the scan updates of ticks 0, 1 and 2 and gone after
    that of tick 3: the robots behind a wall seen once are stopped in ticks 0 to 2 and move from tick 3 on, the others are
    stopped either way."""
    import torch
    from neo_mpc_planner2_amd import fleet as fleet_loop
    from neo_mpc_planner2_amd.solver import BatchSolver, DeviceBatch
    from oracle import mpc_oracle as orc
    ticks = 6
    wox = woy = -10.0
    world = np.zeros((400, 400), dtype=np.uint8)
    p = pairs_fleet(beams=161)
    count, size, res, beams, probs, st, warm, angle = p.count, p.size, p.res, p.beams, p.probs, p.st, p.warm, p.angle
    # the wall: x = 0.1 + 1.55 in the even robot's base frame, y from 0.2 to 0.4 (the even robots move a few centimetres in these
    # ticks and their wall with them: it goes on crossing the left edge, which reaches from -0.35 to 0.35)
    across = 1.55 * np.tan(angle)
    on_wall = (across >= 0.2) & (across <= 0.4)
    assert on_wall.sum() >= 8
    wall = np.where(on_wall, 1.55 / np.cos(angle), np.inf).astype(F32)
    once = np.arange(32) % 2 == 0                                        # pairs 0, 2, 4, ...
    nothing = np.full((count, 1, beams), np.inf, dtype=F32)              # (no INF_IS_VALID: nothing, not even a clearing ray)
    first, later = nothing.copy(), nothing.copy()
    first[0::2, 0] = wall
    later[0::2, 0][~once] = wall
    d_first, d_later = gpu(first), gpu(later)
    params = (0.1, 0.3, 3.0)

    def world_scan(t, poses):                                            # (fleet_kit.world_scan_callback with two sets of ranges)
        return dict(zip(("inscribed_radius", "inflation_radius", "cost_scaling_factor"), params),
                    ranges=d_first if t == 0 else d_later, poses=poses, scanners=[p.front])

    stopped, moving = {}, {}
    for how, max_age in (("never set", None), ("A = 3", 3)):
        with BatchSolver(orc.make_params()) as s:
            if max_age is not None:
                s.set_world_scan_decay(max_age)
            s.set_world_map(world, res, wox, woy)
            commands = []
            d_orig = gpu(p.origins)
            s.roll_costmap_pool(size, size, res, d_orig)
            b = DeviceBatch(probs, st, warm, "cuda:0")
            fleet_loop.closed_loop(s, b, ticks, after_tick=lambda t, cm: commands.append(cm.copy()), footprint=RECT,
                                   rolling=(size, size, res, d_orig), world_scan=world_scan)
            torch.cuda.synchronize()
            commands = np.array(commands)
            stopped[how] = ((commands["flags"] & abi.FLAG_STOPPED) != 0)[:, 1::2]          # [tick, pair]: the odd robots
            moving[how] = (commands["vel"][:, 1::2, 0] > 0.0)
    for how in stopped:
        print("%s: odd robots stopped per tick, wall seen once %s, wall seen every tick %s" %
              (how, stopped[how][:, once].mean(axis=1).tolist(), stopped[how][:, ~once].mean(axis=1).tolist()))
    assert stopped["never set"].all()                                    # without decay: everybody, to the last tick
    assert stopped["A = 3"][:, ~once].all()                              # a wall in every tick's ranges: either way
    assert stopped["A = 3"][:3, once].all()
    assert not stopped["A = 3"][3:, once].any() and moving["A = 3"][3:, once].all()
