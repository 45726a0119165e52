#!/usr/bin/env python3
"""Exact fixture of K1's results (GPU box): tests/golden/recorded/G20_k1_bitwise.npz, the raw outputs of the library NEO_MPC_LIB
points at (default: the tree's) on groups small enough for a test of seconds that still reach every path of the shared
solver headers -- tests/test_k1_bitwise.py solves them again and compares bit for bit.  Outputs only: the inputs come
from seeds.

    python tools/record_k1_bitwise.py [OUT.npz]       (default: tests/golden/recorded/G20_k1_bitwise.npz)
    python tools/record_k1_bitwise.py --digest         (prints one digest per array, writes nothing)

Re-record ONLY for a deliberate numeric change of K1 (a stop rule, a sum's order, a number format), with the build
that carries it, and say so in the commit: an edit that is meant to leave results alone must pass against the fixture
as it is.

Groups (README parameters unless stated; "C2" etc. are synthetic.CONFIGS, seed 0, the first 4096 instances drawn):
  wall     every C2 instance K1 flags NEO_MPC_FLAG_WALL_IN_REACH (the routed kernel's stage-wise branch), cold, then 8
           closed-loop warm ticks of those instances (fleet.closed_loop): every tick's commands, the last tick's state and
           warm start
  free     the first 128 unflagged C2 instances (the dense branch), cold
  cut      the first 256 C2 instances at bench.GENERAL_SETS["C2/cut"] (general routed kernel, bounds active)
  turn     the first 256 at bench.GENERAL_SETS["C2/turn"]
  c3, c5   the first 256 of C3 and the first 128 of C5 (the run-time-sized sweep and candidate_block)
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, "tests", "golden", "recorded", "G20_k1_bitwise.npz")
WARM_TICKS = 8


def _raw(a):
    """A record array as its bytes, one row per instance (the fixture compares whole records, padding included)."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(len(a), -1).copy()


def _cold(out, tag, params, cmap, probs, n):
    from neo_mpc_planner2_amd import synthetic
    from neo_mpc_planner2_amd.solver import BatchSolver
    probs = np.ascontiguousarray(probs)
    st, warm = synthetic.make_states(probs, n)
    with BatchSolver(params) as s:
        s.set_costmap(*cmap)
        cmds, x = s.solve(probs, st, warm)
    out[tag + "_solution"] = x
    out[tag + "_commands"] = _raw(cmds)
    out[tag + "_states"] = _raw(st)
    out[tag + "_warm"] = warm
    return cmds


def compute():
    """Every group solved with the library the package loads; {name: array}."""
    import torch
    import bench
    from neo_mpc_planner2_amd import abi, fleet, synthetic
    from neo_mpc_planner2_amd.solver import BatchSolver, DeviceBatch
    out = {}
    cfg, cmap, probs, st, warm = synthetic.make_workload("C2", seed=0, batch=4096)
    params = bench.readme_params(3)
    # which instances take the stage-wise branch: K1's own flag, from one cold solve of the whole batch
    with BatchSolver(params) as s:
        s.set_costmap(*cmap)
        cmds, _ = s.solve(probs, st.copy(), warm.copy())
    flagged = (cmds["flags"] & abi.FLAG_WALL_IN_REACH) != 0
    wall, free = np.nonzero(flagged)[0], np.nonzero(~flagged)[0][:128]
    out["wall_rows"] = wall.astype(np.int32)
    out["free_rows"] = free.astype(np.int32)
    _cold(out, "wall", params, cmap, probs[wall], 3)
    _cold(out, "free", params, cmap, probs[free], 3)
    # the flagged instances in a closed 30 Hz loop, warm-started tick by tick
    p = np.ascontiguousarray(probs[wall])
    st_w, warm_w = synthetic.make_states(p, 3)
    ticks = []
    with BatchSolver(params) as s:
        s.set_costmap(torch.from_numpy(cmap[0]).to("cuda:0"), *cmap[1:])
        b = DeviceBatch(p, st_w, warm_w, "cuda:0", want_solution=False)

        fleet.closed_loop(s, b, 1 + WARM_TICKS, after_tick=lambda t, cm: ticks.append(_raw(cm)))
        # (every tick's state and warm start feed the next tick's commands: the last tick's stand for all of them)
        out["wall_loop_commands"] = np.stack(ticks[1:])   # (tick 0: the cold solve above at the loop's tick interval)
        out["wall_loop_states"] = _raw(b.states_host())
        out["wall_loop_warm"] = b.warm.cpu().numpy().copy()
    for tag in ("cut", "turn"):
        over = dict(params)
        over.update(bench.GENERAL_SETS["C2/" + tag])
        _cold(out, tag, over, cmap, probs[:256], 3)
    for tag, name, count in (("c3", "C3", 256), ("c5", "C5", 128)):
        cfg, cmap, probs, _, _ = synthetic.make_workload(name, seed=0, batch=4096)
        n = cfg["control_steps"]
        _cold(out, tag, bench.readme_params(n), cmap, probs[:count], n)
    return out


def digests(arrays):
    return {k: hashlib.md5(np.ascontiguousarray(v).tobytes()).hexdigest()[:16] for k, v in sorted(arrays.items())}


def main():
    arrays = compute()
    for k, d in digests(arrays).items():
        print("%-22s %-18s %s" % (k, arrays[k].shape, d))
    if "--digest" in sys.argv[1:]:
        return
    path = next((a for a in sys.argv[1:] if not a.startswith("--")), FIXTURE)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **arrays)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
