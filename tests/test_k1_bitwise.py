"""K1's results, bit for bit: the groups of tools/record_k1_bitwise.py solved again and held against the recorded outputs
(tests/golden/recorded/G20_k1_bitwise.npz) with no tolerance -- solution, command records (velocities, cost, status, iterations,
evaluations, flags), state records and warm starts.  The groups reach every path of the shared solver headers: the routed
kernel's stage-wise branch cold and over eight closed-loop warm ticks, its dense branch, the general routed kernel with
bounds active ("cut", "turn"), and the run-time-sized stage-wise kernel at control_steps 8 and 32.

An edit of the device code that is meant to leave results alone (scheduling, where a load is issued, an instruction
selected for a select) passes this as it stands; when it fails, the first array named tells the group, and the groups tell
the path.  Re-record -- `python tools/record_k1_bitwise.py` on the MI355X -- ONLY for a deliberate numeric change (a stop
rule, the order of a sum, a number format), with the build that carries it, in the commit that makes the change."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def recorder():
    spec = importlib.util.spec_from_file_location("record_k1_bitwise", os.path.join(ROOT, "tools", "record_k1_bitwise.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_k1_outputs_are_bit_for_bit_the_fixture(recorder, golden_dir):
    want = np.load(os.path.join(golden_dir, "recorded", "G20_k1_bitwise.npz"))
    got = recorder.compute()
    assert sorted(got) == sorted(want.files)
    # (the instances K1 routes to the stage-wise direction first: every other array of the group is indexed by them)
    for name in ["wall_rows", "free_rows"] + sorted(want.files):
        w, g = want[name], got[name]
        assert w.dtype == g.dtype and w.shape == g.shape, (name, w.dtype, g.dtype, w.shape, g.shape)
        if not np.array_equal(w.view(np.uint8), np.ascontiguousarray(g).view(np.uint8)):
            rows = np.nonzero((w.reshape(len(w), -1).view(np.uint8) != np.ascontiguousarray(g).reshape(len(g), -1).view(np.uint8)).any(axis=1))[0]
            raise AssertionError("%s differs in %d of %d rows, first %s" % (name, len(rows), len(w), rows[:8]))
