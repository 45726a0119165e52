"""What the phases of K1's stage-wise iteration hand to one another, bit for bit: the calls of
tools/record_stagewise_phases.py made again and held against tests/golden/recorded/G21_stagewise_phases.npz with no
tolerance, NaN pattern included -- the total gradient behind the adjoint and the tangent-cone pass, and the search
direction behind riccati_prepare, the sweep and riccati_finish, on the instances the routed kernel sends to its
three-stage stage-wise branch (registers hand the lane's stage from phase to phase there) and on the general routed kernel
("cut": the same headers with the hand-offs as that kernel has them).  When tests/test_k1_bitwise.py fails, the first
array named here tells the phase.  Re-record only for a deliberate numeric change (the rule of G20).

The CPU part pins the identity the step test's reduction rests on: the maximum of |d| taken three entries per lane and
then over three lanes equals the one taken one entry per lane over nine lanes, NaN and INFINITY included."""
import importlib.util
import itertools
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recorder():
    spec = importlib.util.spec_from_file_location("record_stagewise_phases", os.path.join(ROOT, "tools", "record_stagewise_phases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.gpu
def test_phase_outputs_are_bit_for_bit_the_fixture(golden_dir):
    rec = _recorder()
    want = np.load(os.path.join(golden_dir, "recorded", "G21_stagewise_phases.npz"))
    got = rec.compute()
    assert sorted(got) == sorted(want.files)
    # (rows first, then in the order the phases run: gradient, then the directions iteration by iteration)
    order = ["wall_rows"] + [g + s for g in ("wall", "cut") for s in
                             ("_gradient_cold", "_gradient_warm", "_direction_cold_k1", "_direction_cold_k2",
                              "_direction_cold_k3", "_direction_warm_k1")]
    assert sorted(order) == sorted(want.files)
    for name in order:
        w, g = want[name], np.ascontiguousarray(got[name])
        assert w.dtype == g.dtype and w.shape == g.shape, (name, w.dtype, g.dtype, w.shape, g.shape)
        wb, gb = w.reshape(len(w), -1).view(np.uint8), g.reshape(len(g), -1).view(np.uint8)
        if not np.array_equal(wb, gb):
            rows = np.nonzero((wb != gb).any(axis=1))[0]
            raise AssertionError("%s differs in %d of %d rows, first %s" % (name, len(rows), len(w), rows[:8]))
    # every routed instance of this workload runs at least four iterations: the cold directions of iterations 1-3 exist
    for k in rec.COLD_ITERATIONS:
        for a in (want["wall_direction_cold_k%d" % k], got["wall_direction_cold_k%d" % k]):
            assert not rec.nan_rows(a).any(), k


def _rule(dm, v):
    """k1_solve.h: dm = (v == v) ? fmaxf(dm, v) : INFINITY, in float32 (fmaxf hands back the operand that is not NaN)."""
    return np.float32(np.inf) if v != v else np.fmax(dm, v)


def _fold(values):
    dm = np.float32(0.0)
    for v in values:
        dm = _rule(dm, v)
    return dm


def _lanes_max(per_lane):
    """wave_max_f_few: fmaxf over the lanes' values, which are never NaN (the rule above has turned NaN into INFINITY)."""
    assert not any(v != v for v in per_lane)
    m = per_lane[0]
    for v in per_lane[1:]:
        m = np.fmax(m, v)
    return m


def test_step_test_maximum_does_not_depend_on_the_lane_layout():
    special = [np.float32(x) for x in (0.0, 1e-30, 3.5e-4, 1.0, 7.25, 3.0e38, np.inf, np.nan)]
    rng = np.random.default_rng(21)
    cases = [list(t) + [np.float32(0.0)] * 6 for t in itertools.product(special, repeat=3)]     # one stage: every triple
    cases += [list(rng.permutation(np.array(list(t) + [special[i % 8] for i in range(6)], dtype=np.float32)))
              for t in itertools.product(special, repeat=3)]
    cases += [list(np.abs(rng.standard_normal(9)).astype(np.float32)) for _ in range(200)]
    for d in cases:
        d = [np.float32(abs(v)) if v == v else v for v in d]      # (float)fabs(d[k]): non-negative or NaN
        nine = _lanes_max([_fold([v]) for v in d])                                   # one entry per lane, nine lanes
        three = _lanes_max([_fold(d[3 * i:3 * i + 3]) for i in range(3)])            # three per lane, three lanes
        assert nine.tobytes() == three.tobytes(), (d, nine, three)
        finite = [v for v in d if v == v]
        want = np.float32(np.inf) if len(finite) < 9 else np.float32(max(finite))
        assert nine.tobytes() == want.tobytes(), (d, nine, want)
