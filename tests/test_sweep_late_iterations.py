"""The stage-wise search direction in the late iterations of the longest routed searches, bit for bit: the calls of
tools/record_sweep_late_iterations.py made again and held against tests/golden/recorded/G22_sweep_late_iterations.npz with no
tolerance.  G21 (tests/test_stagewise_phases.py) pins the direction in iterations 1-3; these are the sweeps behind them --
second-order terms on, sliding, pinned and kink stages -- on the 64 instances of C2 (seed 0) with the longest stage-wise
searches (the rows of tests/test_edge_lookup_gpu.py), up to the last iteration any of them reaches under the hook; the
rows of searches that ended earlier are the hook's NaN fill and are compared like the rest (the recorder says why no late
iteration has all 64).  Whatever carries the sweep's gains from its backward to its forward half is held here: a gain
taken from the wrong stage changes every live row.

The same rows then go through the whole search as one batch of 64 (full SIMDs) and as 64 batches of one (lone waves):
commands, state records and warm starts must be the same bytes both ways and the rows of G20 (tests/test_k1_bitwise.py),
and the direction of iteration 8 (two thirds of the searches still run) from lone waves must be the fixture's rows.
The candidate pass' lookups run in both settings: an addend of its objective taken out of order shows in the costs and,
behind them, in which candidate won.  Re-record only for a deliberate numeric change (the rule of G20)."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def recorder():
    spec = importlib.util.spec_from_file_location("record_sweep_late_iterations",
                                                  os.path.join(ROOT, "tools", "record_sweep_late_iterations.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "recorded", "G22_sweep_late_iterations.npz"))


def _raw(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(len(a), -1).copy()


def _differing(want, got):
    return np.nonzero((_raw(want) != _raw(got)).any(axis=1))[0]


def test_late_directions_are_bit_for_bit_the_fixture(recorder, fixture):
    got = recorder.compute()
    names = ["rows"] + ["direction_cold_k%d" % k for k in recorder.ITERATIONS]
    assert sorted(got) == sorted(fixture.files) == sorted(names)
    assert recorder.FIRST == 4 and len(fixture["rows"]) == recorder.ROWS and 1213 in fixture["rows"].tolist()
    for name in names:
        w, g = fixture[name], np.ascontiguousarray(got[name])
        assert w.dtype == g.dtype and w.shape == g.shape, (name, w.dtype, g.dtype, w.shape, g.shape)
        rows = _differing(w, g)
        assert len(rows) == 0, "%s differs in %d of %d rows, first %s" % (name, len(rows), len(w), fixture["rows"][rows][:8])
    # every recorded iteration pins something, the first one nearly every row
    live = [int((~recorder.nan_rows(fixture["direction_cold_k%d" % k])).sum()) for k in recorder.ITERATIONS]
    assert min(live) >= 1 and live[0] >= recorder.ROWS - recorder.ROWS // 8 and live == sorted(live, reverse=True), live


def _solve(s, probs):
    from neo_mpc_planner2_amd import synthetic
    probs = np.ascontiguousarray(probs)
    st, warm = synthetic.make_states(probs, 3)
    cmds, _ = s.solve(probs, st, warm)
    return _raw(cmds), _raw(st), np.ascontiguousarray(warm)


def test_batch_and_lone_waves_agree_and_are_the_fixtures(recorder, fixture, golden_dir):
    from neo_mpc_planner2_amd.solver import BatchSolver
    g20 = np.load(os.path.join(golden_dir, "recorded", "G20_k1_bitwise.npz"))
    rows, pick, _ = recorder.pick_rows()
    assert np.array_equal(rows, fixture["rows"]) and np.array_equal(g20["wall_rows"][pick], rows)
    params, cmap, probs = recorder.workload()
    lone_k = 8
    last = "direction_cold_k%d" % lone_k
    assert (~recorder.nan_rows(fixture[last])).sum() >= recorder.ROWS // 2
    zero = np.zeros((1, 9), dtype=np.float64)
    with BatchSolver(params) as s:
        s.set_costmap(*cmap)
        batch = _solve(s, probs)
        alone = [_solve(s, probs[i:i + 1]) for i in range(recorder.ROWS)]
        lone_direction = np.concatenate([s.direction(probs[i:i + 1], zero, lone_k) for i in range(recorder.ROWS)])
    for k, name in enumerate(("commands", "states", "warm")):
        single = np.concatenate([a[k] for a in alone])
        bad = _differing(single, batch[k])
        assert len(bad) == 0, "%s: the batch of %d and the batches of one differ in rows %s" % (name, recorder.ROWS, rows[bad][:8])
        want = g20["wall_" + name][pick]
        assert want.dtype == batch[k].dtype and want.shape == batch[k].shape, (name, want.dtype, want.shape)
        bad = _differing(want, batch[k])
        assert len(bad) == 0, "%s: rows %s are not G20's" % (name, rows[bad][:8])
    bad = _differing(fixture[last], lone_direction)
    assert len(bad) == 0, "%s from lone waves: rows %s are not the fixture's" % (last, rows[bad][:8])
