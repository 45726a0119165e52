#!/usr/bin/env python3
"""K15 (the plan check, neo_mpc_check_plans_device) on its own: 4096 plans of 1000 poses on a 1000 x 1000 world at 5 cm, point
mode and footprint mode (synthetic.RECT_FOOTPRINT), the check starting at pose 0 and at the plan's middle -- beside K4
(neo_mpc_select_carrots_device) on the same plans, same handle, same session: K4 streams the same bytes (every pose once for
the closest pose, [begin, end) once more), so it is the yardstick.  The variants ALTERNATE launch by launch inside one loop,
HIP events around each launch; medians and the spread of each.  A record, not a gate: bench.py does not run it.

The headline world is the yard with every cell capped at 252 -- nothing blocks under max_cost 253, every pose of [begin, end)
is read: the full stream.  `yard` is the same world as it is, where most plans end early at their first blocked pose.

    python tools/bench_plan_check.py [--steps 30] [--warmup 5] [--plans 4096] [--poses 1000]
Prints one JSON line.  pose_stream_GBps = 24 B x (poses + end - begin) x plans / median time.
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
    ap.add_argument("--plans", type=int, default=4096)
    ap.add_argument("--poses", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    assert args.steps >= 20, "median over at least 20 launches"
    import torch
    from neo_mpc_planner2_amd import abi, synthetic
    from neo_mpc_planner2_amd.solver import BatchSolver
    dev = "cuda:0"
    count, n = args.plans, args.poses
    yard, res, ox, oy = synthetic.make_costmap(1000, seed=0)
    # (1.4 cm a pose: a plan of 1000 poses that starts within 10 m of the middle stays on the 50 m world)
    plan_poses, offsets, _ = synthetic.make_plans(count, seed=1, min_len=n, max_len=n, spacing=0.014)
    plans = plan_poses.reshape(count, n, 3)
    d_plans = torch.from_numpy(plan_poses).to(dev)
    d_offsets = torch.from_numpy(offsets.astype(np.int32)).to(dev)
    d_robots = {"begin 0": torch.from_numpy(plans[:, 0].copy()).to(dev), "begin middle": torch.from_numpy(plans[:, n // 2].copy()).to(dev)}
    d_results = torch.zeros(count * 24, dtype=torch.uint8, device=dev)
    d_fp = torch.tensor(np.asarray(synthetic.RECT_FOOTPRINT, dtype=np.float64), device=dev)
    d_slow = torch.zeros(count, dtype=torch.int32, device=dev)
    d_carrots = torch.zeros(count * 80, dtype=torch.uint8, device=dev)
    lp = abi.NeoMpcLookaheadParams(0.5, 0.5, 0.5, 1e9)       # (no cut-off: K4 scans [begin, end) to the plan's end as well)
    stream = torch.cuda.current_stream()
    out = {"kernel": "k_plan_check", "plans": count, "poses": n, "world": "make_costmap(1000), 5 cm", "footprint": "RECT_FOOTPRINT",
           "steps": args.steps, "worlds": {}}
    with BatchSolver({}) as s:
        for world_name, cells in (("open", np.minimum(yard, 252)), ("yard", yard)):
            s.set_world_map(torch.from_numpy(np.ascontiguousarray(cells)).to(dev), res, ox, oy)
            variants = {}
            for where, robots in d_robots.items():
                variants["k4, " + where] = lambda r=robots: s.select_carrots_device(lp, d_plans, d_offsets, r, d_slow, d_carrots)
                variants["point, " + where] = lambda r=robots: s.check_plans_device(d_plans, d_offsets, d_results, robot_poses=r)
                variants["footprint, " + where] = lambda r=robots: s.check_plans_device(d_plans, d_offsets, d_results,
                                                                                        robot_poses=r, footprint=d_fp)
            ms = {k: [] for k in variants}
            spans = {}
            for step in range(args.warmup + args.steps):
                for name, launch in variants.items():          # the variants alternate launch by launch
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(stream)
                    launch()
                    b.record(stream)
                    torch.cuda.synchronize()
                    if step >= args.warmup:
                        ms[name].append(a.elapsed_time(b))
                    elif step == 0 and not name.startswith("k4"):
                        r = d_results.cpu().numpy().view(abi.PLAN_CHECK_DTYPE)
                        read = np.where(r["status"] == 1, r["first_blocked"] + 1, r["end"]).astype(np.int64) - r["begin"]
                        spans[name] = dict(blocked_fraction=float((r["status"] == 1).mean()), poses_checked_mean=float(read.mean()))
            rows = {}
            for name, t in ms.items():
                med = float(np.median(t))
                row = dict(ms_median=med, ms_min=float(np.min(t)), ms_max=float(np.max(t)))
                where = name.split(", ")[1]
                begin = 0 if where == "begin 0" else n // 2
                # the bytes of the pose stream K4 and point mode share: every pose once, [begin, end) once more (where nothing
                # blocks: a check that ends early reads less)
                if world_name == "open":
                    row["pose_stream_GBps"] = 24.0 * (n + n - begin) * count / (med * 1e-3) / 1e9
                row["ratio_to_k4"] = med / float(np.median(ms["k4, " + where]))
                row.update(spans.get(name, {}))
                rows[name] = row
            out["worlds"][world_name] = rows
    print(json.dumps(out))


if __name__ == "__main__":
    main()
