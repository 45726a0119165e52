"""The wall model's reads issued together (csrc/costmap.h edge_stickiness under the static-tile kernels), on the device: the
64 instances of C2 (seed 0) with the longest stage-wise searches -- instance 1213, the search a C2 launch waits for, among
them -- solved cold as one batch of 64 and as 64 batches of one.  The smallest shape that reaches the wall model with a wall
on one axis, on both, and with hops, in a full launch and in a lone wave.  Both must give the same bytes in commands, state
records and warm starts, and the batch's rows must be the rows of the exact fixture (G20, tests/test_k1_bitwise.py): no
tolerance anywhere."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS = 64


def _raw(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(len(a), -1).copy()


def _solve(s, probs):
    from neo_mpc_planner2_amd import synthetic
    probs = np.ascontiguousarray(probs)
    st, warm = synthetic.make_states(probs, 3)
    cmds, _ = s.solve(probs, st, warm)
    return _raw(cmds), _raw(st), np.ascontiguousarray(warm)


def test_longest_wall_searches_batched_and_alone_are_the_fixture(golden_dir):
    import bench
    from neo_mpc_planner2_amd import abi, synthetic
    from neo_mpc_planner2_amd.solver import BatchSolver
    want = np.load(os.path.join(golden_dir, "recorded", "G20_k1_bitwise.npz"))
    wall = want["wall_rows"]
    iters = want["wall_commands"].view(abi.COMMAND_DTYPE).reshape(-1)["iterations"]
    pick = np.sort(np.argsort(-iters.astype(np.int64), kind="stable")[:ROWS])    # (rows of the fixture's wall group)
    assert 1213 in wall[pick].tolist() and iters[pick].max() == 19
    cfg, cmap, probs, _, _ = synthetic.make_workload("C2", seed=0, batch=4096)
    probs = probs[wall[pick]]
    with BatchSolver(bench.readme_params(3)) as s:
        s.set_costmap(*cmap)
        batch = _solve(s, probs)
        alone = [_solve(s, probs[i:i + 1]) for i in range(ROWS)]
    for k, name in enumerate(("commands", "states", "warm")):
        single = np.concatenate([a[k] for a in alone])
        rows = np.nonzero((_raw(single) != _raw(batch[k])).any(axis=1))[0]
        assert len(rows) == 0, "%s: the batch of %d and the batches of one differ in rows %s" % (name, ROWS, wall[pick][rows][:8])
        fixture = want["wall_" + name][pick]
        assert fixture.dtype == batch[k].dtype and fixture.shape == batch[k].shape, (name, fixture.dtype, fixture.shape)
        rows = np.nonzero((_raw(fixture) != _raw(batch[k])).any(axis=1))[0]
        assert len(rows) == 0, "%s: rows %s are not the fixture's" % (name, wall[pick][rows][:8])
