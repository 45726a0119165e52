#!/usr/bin/env python3
"""Study: kernel time of the lone longest search of the headline workload -- the instance of C2 (seed 0, 4096) with the
most iterations among those K1 routes to the stage-wise direction, solved cold as a batch of one.  A C2 launch lasts as
long as this one wave's dependent chain; alone on the device its time does not depend on what else the launch holds or
on how the box's other tenants load it.  Kernel time from the dispatch-stamped events (solve_device(..., events=)):
the median of 50 launches behind 10 warm-up launches, with the library NEO_MPC_LIB points at (default: the tree's).
usage: [NEO_MPC_LIB=<lib>] python tools/lone_longest_search.py [--instance 1213]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instance", type=int, default=1213, help="row of synthetic.make_workload('C2', seed=0) (1213: 19 iterations)")
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    import torch
    import bench
    from neo_mpc_planner2_amd import _lib, synthetic
    from neo_mpc_planner2_amd.solver import BatchSolver, DeviceBatch
    cfg, cmap, probs, _, _ = synthetic.make_workload("C2", seed=0, batch=4096)
    p = np.ascontiguousarray(probs[args.instance:args.instance + 1])
    st, warm = synthetic.make_states(p, 3)
    dev = torch.device("cuda:0")
    with BatchSolver(bench.readme_params(3)) as s:
        s.set_costmap(torch.from_numpy(cmap[0]).to(dev), *cmap[1:])
        base = DeviceBatch(p, st, warm, dev, want_solution=False)
        sets = [base.fresh_state() for _ in range(args.warmup + args.launches)]   # (every launch cold: a state of its own)
        stream = torch.cuda.current_stream()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in sets]
        for e0, e1 in evs:
            e0.record(stream)
            e1.record(stream)
        torch.cuda.synchronize()
        for b, ev in zip(sets, evs):
            s.solve_device(base.problems, b.states, b.warm, b.commands, velocities=b.vel, events=ev)
            torch.cuda.synchronize()
        ms = np.array([a.elapsed_time(b) for a, b in evs[args.warmup:]])
        cmds = sets[-1].commands_host()
    print(json.dumps({"study": "lone_longest_search", "lib": os.path.basename(_lib.LIB_PATH), "instance": args.instance,
                      "iterations": int(cmds["iterations"][0]), "launches": args.launches, "warmup": args.warmup,
                      "kernel_us_median": round(1e3 * float(np.median(ms)), 2), "kernel_us_min": round(1e3 * float(ms.min()), 2),
                      "kernel_us_max": round(1e3 * float(ms.max()), 2)}))


if __name__ == "__main__":
    main()
