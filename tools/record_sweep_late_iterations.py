#!/usr/bin/env python3
"""Exact fixture of the stage-wise search direction in the LATE iterations of the longest routed searches (GPU box):
tests/golden/recorded/G22_sweep_late_iterations.npz, the raw output of the library's direction hook
(BatchSolver.direction) with the library NEO_MPC_LIB points at (default: the tree's).  tests/test_sweep_late_iterations.py
makes the same calls again and compares bytes.  G21 (tools/record_stagewise_phases.py) pins the direction in iterations
1-3 only; the sweeps behind them are the ones that carry the second-order terms and meet sliding, pinned and kink stages,
and whatever hands the sweep's gains from its backward to its forward half must be right there too.

    python tools/record_sweep_late_iterations.py [OUT.npz]   (default: tests/golden/recorded/G22_sweep_late_iterations.npz)
    python tools/record_sweep_late_iterations.py --digest     (prints one digest per array, writes nothing)
    python tools/record_sweep_late_iterations.py --scan       (NaN rows per iteration up to the longest search's count)

Re-record ONLY for a deliberate numeric change of K1, with the build that carries it (the rule of G20).

Rows: the 64 instances of C2 (synthetic.make_workload("C2", seed=0), README parameters) with the longest stage-wise
searches -- the rows of tests/test_edge_lookup_gpu.py, instance 1213 among them -- picked from G20's recorded iteration
counts.  Recorded: the direction from u = 0 in iterations FIRST ... LAST.  A search that ended before the iteration asked
for leaves a NaN row, and the hook's searches are not the solves G20 counted: the hook takes u as a warm start (no reset,
no steepest-descent first iteration), so they end earlier -- of the 64, one before iteration 4, 20 before iteration 8, all
but one before iteration 16, and that one before iteration 18 (--scan).  No iteration behind G21's has all 64 rows, so the
NaN rows are recorded as they are and compared with the rest: they pin where each search ends.  LAST is the last
iteration at which a row still holds a direction; the recorder refuses to write a fixture with an iteration that holds
none, or whose first iteration has lost more than one row in eight.
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, "tests", "golden", "recorded", "G22_sweep_late_iterations.npz")
G20 = os.path.join(ROOT, "tests", "golden", "recorded", "G20_k1_bitwise.npz")
LIMIT_BYTES = 300 * 1024
ROWS = 64
FIRST, LAST = 4, 17
ITERATIONS = tuple(range(FIRST, LAST + 1))


def nan_rows(a):
    return np.isnan(a).any(axis=1)


def pick_rows():
    """(rows of C2, rows of G20's wall group, their recorded iteration counts): the ROWS longest stage-wise searches."""
    from neo_mpc_planner2_amd import abi
    g20 = np.load(G20)
    wall = g20["wall_rows"]
    iters = g20["wall_commands"].view(abi.COMMAND_DTYPE).reshape(-1)["iterations"]
    pick = np.sort(np.argsort(-iters.astype(np.int64), kind="stable")[:ROWS])
    return wall[pick], pick, iters[pick]


def workload():
    """(parameters, costmap, the ROWS problems) of the fixture."""
    import bench
    from neo_mpc_planner2_amd import synthetic
    rows, _, _ = pick_rows()
    cfg, cmap, probs, _, _ = synthetic.make_workload("C2", seed=0, batch=4096)
    return bench.readme_params(3), cmap, np.ascontiguousarray(probs[rows])


def compute(iterations=ITERATIONS):
    """Every call of the fixture with the library the package loads; {name: array}."""
    from neo_mpc_planner2_amd.solver import BatchSolver
    rows, _, _ = pick_rows()
    params, cmap, probs = workload()
    zero = np.zeros((len(probs), 9), dtype=np.float64)
    out = {"rows": rows.astype(np.int32)}
    with BatchSolver(params) as s:
        s.set_costmap(*cmap)
        for k in iterations:
            out["direction_cold_k%d" % k] = s.direction(probs, zero, k)
    return out


def digests(arrays):
    return {k: hashlib.md5(np.ascontiguousarray(v).tobytes()).hexdigest()[:16] for k, v in sorted(arrays.items())}


def main():
    scan = "--scan" in sys.argv[1:]
    arrays = compute(tuple(range(FIRST, int(pick_rows()[2].max()) + 1)) if scan else ITERATIONS)
    for k, d in digests(arrays).items():
        a = arrays[k]
        share = " NaN rows %d of %d" % (nan_rows(a).sum(), len(a)) if a.dtype == np.float64 else ""
        print("%-22s %-10s %s%s" % (k, a.shape, d, share))
    if scan or "--digest" in sys.argv[1:]:
        return
    bad = [k for k in sorted(arrays) if arrays[k].dtype == np.float64 and nan_rows(arrays[k]).all()]
    if bad:
        raise SystemExit("not written: no search of the %d reaches %s" % (ROWS, ", ".join(bad)))
    if nan_rows(arrays["direction_cold_k%d" % FIRST]).sum() > ROWS // 8:
        raise SystemExit("not written: more than %d searches ended before iteration %d" % (ROWS // 8, FIRST))
    path = next((a for a in sys.argv[1:] if not a.startswith("--")), FIXTURE)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    print("wrote %s (%d bytes)" % (path, size))
    if size > LIMIT_BYTES:
        raise SystemExit("%s is larger than %d bytes" % (path, LIMIT_BYTES))


if __name__ == "__main__":
    main()
