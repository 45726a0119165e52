#!/usr/bin/env python3
"""K16 (the grid planner, neo_mpc_replan_plans_device) on its own: 1, 64 and 1024 robots at windows of 32, 64 and 128 cells on a
walled yard -- synthetic.make_costmap(1000) at 5 cm with a lethal wall every 48 cells along both axes, a gap of 6 cells in the
middle of every wall segment --, every robot's goal 0.4 W cells east and 0.3 W cells north of its start.  HIP events around each
launch; medians and the spread.  Beside the times, the number of relaxation sweeps the transcription predicts for the first
robots of the fleet: the most moves on a cheapest path to the goal from any cell of the window, plus the sweep that sees no
change -- what a Jacobi relaxation needs; the kernel relaxes in place and needs at most as many.  A record, not a gate:
bench.py does not run it, and there is no earlier planner to compare with.

    python tools/bench_replan.py [--steps 20] [--warmup 3] [--predict 4]
Prints one JSON line.
"""
import argparse
import heapq
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def walled_yard():
    from neo_mpc_planner2_amd import synthetic
    cells, res, ox, oy = synthetic.make_costmap(1000, seed=0)
    cells = cells.copy()
    for at in range(48, 1000, 48):
        wall = np.ones(1000, dtype=bool)
        for gap in range(21, 1000, 48):
            wall[gap:gap + 6] = False
        cells[at, wall] = 254
        cells[wall, at] = 254
    return cells, res, ox, oy


def predicted_sweeps(q):
    """Dijkstra over (cost, moves) from the goal of the search `q` (tests/grid_planner_reference.Search) -> the most moves on
    a cheapest path from any reached cell, plus one."""
    from tests import grid_planner_reference as ref
    best = {q.g: (0, 0)}
    heap = [(0, 0, q.g)]
    while heap:
        d, hops, b = heapq.heappop(heap)
        if (d, hops) > best[b] or not q.traversable(b):
            continue
        for k in range(8):
            a = (b[0] - ref.MOVES[k][0], b[1] - ref.MOVES[k][1])
            if not q.inside(a) or not q.leaves(a) or not q.allowed(a, k):
                continue
            cand = (q.step(a, k) + d, hops + 1)
            if cand < best.get(a, (1 << 32, 0)):
                best[a] = cand
                heapq.heappush(heap, cand + (a,))
    return max(h for _, h in best.values()) + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--predict", type=int, default=4, help="robots per case whose sweep count the transcription predicts")
    args = ap.parse_args()
    import torch
    from neo_mpc_planner2_amd import abi
    from neo_mpc_planner2_amd.solver import BatchSolver
    from tests import grid_planner_reference as ref
    dev = "cuda:0"
    cells, res, ox, oy = walled_yard()
    rng = np.random.default_rng(5)
    stream = torch.cuda.current_stream()
    kw = dict(max_cost=253, unknown_cost=0, neutral_cost=50)
    out = {"kernel": "k_replan", "world": "make_costmap(1000), 5 cm, walls every 48 cells with 6-cell gaps", "steps": args.steps,
           "cases": {}}
    with BatchSolver({}) as s:
        s.set_world_map(torch.from_numpy(cells).to(dev), res, ox, oy)
        for window in (32, 64, 128):
            for count in (1, 64, 1024):
                start_cells = rng.integers(150, 850, size=(count, 2))
                goal_cells = start_cells + (int(0.4 * window), int(0.3 * window))
                starts = (start_cells + 0.5) * res + (ox, oy)
                goals = (goal_cells + 0.5) * res + (ox, oy)
                stride = 4 * window
                d_starts, d_goals = torch.from_numpy(starts).to(dev), torch.from_numpy(goals).to(dev)
                d_cells = torch.zeros((count, stride, 2), dtype=torch.int32, device=dev)
                d_poses = torch.zeros((count, stride, 3), dtype=torch.float64, device=dev)
                d_results = torch.zeros(count * 24, dtype=torch.uint8, device=dev)
                ms = []
                for step in range(args.warmup + args.steps):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(stream)
                    s.replan_plans_device(d_starts, d_goals, window, d_cells, d_results, path_poses=d_poses, **kw)
                    b.record(stream)
                    torch.cuda.synchronize()
                    if step >= args.warmup:
                        ms.append(a.elapsed_time(b))
                r = d_results.cpu().numpy().view(abi.REPLAN_DTYPE)
                sweeps = []
                for i in range(min(count, args.predict)):
                    rec, path, q = ref.replan_one(cells, res, ox, oy, starts[i], goals[i], window, 253, 0, 50, stride)
                    assert rec == tuple(r[i].tolist())[:5], (window, count, i, rec, r[i])
                    if rec[0] in (0, 1, 5) and len(path) != 1:
                        sweeps.append(predicted_sweeps(q))
                out["cases"]["W %d, %d robots" % (window, count)] = dict(
                    ms_median=float(np.median(ms)), ms_min=float(np.min(ms)), ms_max=float(np.max(ms)),
                    status_counts=np.bincount(r["status"], minlength=6).tolist(), length_max=int(r["length"].max()),
                    predicted_sweeps=sweeps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
