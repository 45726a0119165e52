#!/usr/bin/env python3
"""Exact fixture of what the phases of K1's stage-wise iteration hand to one another (GPU box):
tests/golden/recorded/G21_stagewise_phases.npz, the raw outputs of the library's two test hooks -- the total gradient
behind the tangent-cone pass (BatchSolver.gradient) and the search direction of a given iteration behind the sweep
(BatchSolver.direction) -- with the library NEO_MPC_LIB points at (default: the tree's).  tests/test_stagewise_phases.py
makes the same calls again and compares bytes.  When G20 (tests/test_k1_bitwise.py) fails, this one says in which
phase the difference arose: adjoint + cone (gradient), or prepare + sweep + finish (direction).

    python tools/record_stagewise_phases.py [OUT.npz]   (default: tests/golden/recorded/G21_stagewise_phases.npz)
    python tools/record_stagewise_phases.py --digest     (prints one digest per array, writes nothing)

Re-record ONLY for a deliberate numeric change of K1, with the build that carries it (the rule of G20).

Groups (C2 = synthetic.make_workload("C2", seed=0), README parameters unless stated):
  wall   the C2 instances K1 flags NEO_MPC_FLAG_WALL_IN_REACH (the routed kernel's three-stage stage-wise branch)
  cut    the first 256 C2 instances at bench.GENERAL_SETS["C2/cut"] (the general routed kernel: the shared headers with the
         register hand-offs of the three-stage tame kernels off where they are off)
Per group: gradient at u = 0 and at u = the group's warm start of G20 (`<group>_warm`); direction from u = 0 in
iterations 1, 2, 3 and from the warm start in iteration 1.  A search that ended before the iteration asked for leaves
a NaN row; the cold wall rows may hold none (every routed instance of this workload runs at least four iterations):
the recorder refuses to write a fixture that has one.
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, "tests", "golden", "recorded", "G21_stagewise_phases.npz")
G20 = os.path.join(ROOT, "tests", "golden", "recorded", "G20_k1_bitwise.npz")
LIMIT_BYTES = 300 * 1024
COLD_ITERATIONS = (1, 2, 3)


def nan_rows(a):
    return np.isnan(a).any(axis=1)


def _hooks(out, tag, params, cmap, probs, warm):
    from neo_mpc_planner2_amd.solver import BatchSolver
    probs = np.ascontiguousarray(probs)
    zero = np.zeros_like(warm)
    with BatchSolver(params) as s:
        s.set_costmap(*cmap)
        out[tag + "_gradient_cold"] = s.gradient(probs, zero)
        out[tag + "_gradient_warm"] = s.gradient(probs, warm)
        for k in COLD_ITERATIONS:
            out[tag + "_direction_cold_k%d" % k] = s.direction(probs, zero, k)
        out[tag + "_direction_warm_k1"] = s.direction(probs, warm, 1)


def compute():
    """Every call of the fixture with the library the package loads; {name: array}."""
    import bench
    from neo_mpc_planner2_amd import abi, synthetic
    from neo_mpc_planner2_amd.solver import BatchSolver
    g20 = np.load(G20)
    out = {}
    cfg, cmap, probs, st, warm = synthetic.make_workload("C2", seed=0, batch=4096)
    params = bench.readme_params(3)
    # which instances take the stage-wise branch: K1's own flag, from one cold solve of the whole batch (as G20 does)
    with BatchSolver(params) as s:
        s.set_costmap(*cmap)
        cmds, _ = s.solve(probs, st.copy(), warm.copy())
    wall = np.nonzero((cmds["flags"] & abi.FLAG_WALL_IN_REACH) != 0)[0]
    out["wall_rows"] = wall.astype(np.int32)
    if not np.array_equal(out["wall_rows"], g20["wall_rows"]):
        raise SystemExit("the flagged rows are not G20's wall_rows: its wall_warm does not belong to them")
    _hooks(out, "wall", params, cmap, probs[wall], np.ascontiguousarray(g20["wall_warm"]))
    over = dict(params)
    over.update(bench.GENERAL_SETS["C2/cut"])
    _hooks(out, "cut", over, cmap, probs[:256], np.ascontiguousarray(g20["cut_warm"]))
    return out


def digests(arrays):
    return {k: hashlib.md5(np.ascontiguousarray(v).tobytes()).hexdigest()[:16] for k, v in sorted(arrays.items())}


def main():
    arrays = compute()
    for k, d in digests(arrays).items():
        a = arrays[k]
        share = " NaN rows %d of %d" % (nan_rows(a).sum(), len(a)) if a.dtype == np.float64 else ""
        print("%-26s %-12s %s%s" % (k, a.shape, d, share))
    bad = [k for k in ("wall_direction_cold_k%d" % k for k in COLD_ITERATIONS) if nan_rows(arrays[k]).any()]
    if "--digest" in sys.argv[1:]:
        return
    if bad:
        raise SystemExit("not written: a routed search ended before its fourth iteration (NaN rows in %s)" % ", ".join(bad))
    path = next((a for a in sys.argv[1:] if not a.startswith("--")), FIXTURE)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    print("wrote %s (%d bytes)" % (path, size))
    if size > LIMIT_BYTES:
        raise SystemExit("%s is larger than %d bytes" % (path, LIMIT_BYTES))


if __name__ == "__main__":
    main()
