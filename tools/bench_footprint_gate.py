#!/usr/bin/env python3
"""K6 (the footprint gate, neo_mpc_footprint_gate_device) on its own: synthetic.RECT_FOOTPRINT on config C2's costmap at
4096 and at 262 144 robots, HIP events around each launch, median over the timed launches after a warm-up (and the same
number of launches back to back inside one event pair, per launch) -- and, for scale, K1's kernel time for the same
4096-robot fleet (one cold tick of config C2, stamped by the dispatch itself).  A record, not a gate: bench.py does not
run it.

    python tools/bench_footprint_gate.py [--steps 30] [--warmup 5] [--robots 4096 262144]
Prints one JSON line.  The gate's share of a tick is gate_ms / k1_ms at 4096 robots.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, nargs="+", default=[4096, 262144])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    assert args.steps >= 20, "median over at least 20 launches"
    import torch
    from neo_mpc_planner2_amd import synthetic
    from neo_mpc_planner2_amd.solver import BatchSolver, DeviceBatch
    from oracle import mpc_oracle
    dev = "cuda:0"
    cfg, cmap, probs, st, warm = synthetic.make_workload("C2", seed=0)
    stream = torch.cuda.current_stream()
    out = {"kernel": "k_footprint_gate", "footprint": "RECT_FOOTPRINT", "map": "C2 (500x500, 5 cm)", "steps": args.steps,
           "gate": []}
    with BatchSolver(mpc_oracle.make_params(control_steps=cfg["control_steps"])) as s:
        s.set_costmap(*cmap)
        base = torch.tensor(np.asarray(synthetic.RECT_FOOTPRINT, dtype=np.float64), device=dev)
        for count in args.robots:
            p = synthetic.make_problems(count, cfg["map_size"], seed=1000)
            q = p["cur_q"]
            yaw = np.arctan2(2 * q[:, 3] * q[:, 2], 1 - 2 * q[:, 2] ** 2)
            poses = torch.from_numpy(np.concatenate([p["cur_xy"], yaw[:, None]], 1)).to(dev)
            costs = torch.zeros(count, dtype=torch.float64, device=dev)
            polys = torch.zeros((count, 4, 2), dtype=torch.float64, device=dev)
            for _ in range(args.warmup):
                s.footprint_gate_device(base, costs, poses=poses, footprints_out=polys)
            torch.cuda.synchronize()
            ms = []
            for _ in range(args.steps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                s.footprint_gate_device(base, costs, poses=poses, footprints_out=polys)
                b.record(stream)
                torch.cuda.synchronize()
                ms.append(a.elapsed_time(b))
            # ... and the same launches back to back inside ONE event pair: the event records around a single launch add their
            # own packets to what is read as kernel time, which matters for a kernel of a few microseconds
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(args.steps):
                s.footprint_gate_device(base, costs, poses=poses, footprints_out=polys)
            b.record(stream)
            torch.cuda.synchronize()
            train_ms = a.elapsed_time(b) / args.steps
            c = costs.cpu().numpy()
            # what the kernel has to move: a pose, a cost and four oriented vertices per robot, and the outline's cells
            # (2 x (14 + 10) cells of 5 cm around a 0.7 m x 0.5 m rectangle at yaw 0; more when it is turned)
            out["gate"].append({"robots": count, "gate_ms_median": float(np.median(ms)), "gate_ms_min": float(np.min(ms)),
                                "gate_ms_max": float(np.max(ms)), "gate_ms_back_to_back": train_ms, "robots_per_s": count / (float(np.median(ms)) * 1e-3),
                                "bytes_per_robot_records": 24 + 8 + 64,
                                "lethal_fraction": float((c >= 254).mean()), "free_fraction": float((c == 0).mean())})
        # K1 for the same 4096-robot fleet, same handle, same session: cold ticks of config C2 from fresh state
        k1 = []
        for _ in range(args.steps):
            db = DeviceBatch(probs, st, warm, dev, want_solution=False)
            evs = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            for e in evs:
                e.record(stream)
            torch.cuda.synchronize()
            s.solve_device(db.problems, db.states, db.warm, db.commands, events=evs)
            torch.cuda.synchronize()
            k1.append(evs[0].elapsed_time(evs[1]))
        out["k1_robots"] = len(probs)
        out["k1_ms_median"] = float(np.median(k1[args.warmup:]))
    first = out["gate"][0]
    if first["robots"] == out["k1_robots"]:
        out["gate_share_of_k1"] = first["gate_ms_median"] / out["k1_ms_median"]
        out["gate_share_of_k1_back_to_back"] = first["gate_ms_back_to_back"] / out["k1_ms_median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
