#!/usr/bin/env python3
"""Development aid (GPU box): are two builds of libneo_mpc bit-identical on a workload?  Solves each group below with the
library NEO_MPC_LIB points at and prints a digest of the raw solutions and one of the raw command records (velocities,
objective, status, iterations, evaluations, flags -- a stop rule that fires an iteration earlier shows there first).
Groups: the first 4096 instances of C3 / C5 / the "turn" set / C2, and -- the kernels of neo_mpc_kernels.hip a caller reaches
only by pinning `method`, which tests/test_k1_bitwise.py (G20) does not -- 1024 instances of C2 each with L-BFGS and dense Newton
at control_steps 3, dense Newton at 5 (the run-time-sized dense kernel), L-BFGS at 8, and the "cut" set under dense Newton.
usage: NEO_MPC_LIB=<lib> python tools/bitwise_ab.py"""
import hashlib, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from neo_mpc_planner2_amd import abi, synthetic
from neo_mpc_planner2_amd.solver import BatchSolver

LBFGS, NEWTON = 1, 2   # NEO_MPC_METHOD_* (include/neo_mpc.h)
GROUPS = [  # workload, control_steps (None: the workload's), instances, parameter overrides, label
    ("C3", None, 4096, {}, ""), ("C5", None, 4096, {}, ""), ("C2", None, 4096, bench.GENERAL_SETS["C2/turn"], "turn"),
    ("C2", None, 4096, {}, ""),
    ("C2", 3, 1024, dict(method=LBFGS), "lbfgs n3"), ("C2", 3, 1024, dict(method=NEWTON), "newton n3"),
    ("C2", 5, 1024, dict(method=NEWTON), "newton n5"), ("C2", 8, 1024, dict(method=LBFGS), "lbfgs n8"),
    ("C2", 3, 1024, dict(bench.GENERAL_SETS["C2/cut"], method=NEWTON), "cut newton n3"),
]


def digest(a):
    return hashlib.md5(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


for wl, steps, count, over, label in GROUPS:
    cfg, cmap, probs, st, warm = synthetic.make_workload(wl, seed=0, batch=count)
    n = steps or cfg["control_steps"]
    if steps:
        st, warm = synthetic.make_states(probs, n)
    params = bench.readme_params(n); params.update(over)
    with BatchSolver(params) as s:
        s.set_costmap(*cmap)
        cm, x = s.solve(probs, st, warm)
    assert cm.dtype == abi.COMMAND_DTYPE
    print("%-3s %-14s solutions %s commands %s iterations %.3f converged %d" %
          (wl, label, digest(x), digest(cm), cm["iterations"].mean(), (cm["status"] == 0).sum()))
