#!/usr/bin/env python3
"""K8 (the fleet stamp) on its own, with HIP events: 4096 and 65 535 windows of 200 x 200 cells at 5 cm, RECT_FOOTPRINT,
the robots spread over a square yard so that a window holds about four others (the figure is printed).  Beside it, in the
same process and for the same fleet: K7's roll, which streams the whole pool where K8 rewrites a few thousand cells per
neighbour.  Every figure is the median of event pairs around back-to-back calls (an event pair around one short call
measures the event records as much as the kernels); the pool is rolled before every timed stamp so that K8 always meets
unstamped windows, and the roll's own time is taken out.
usage: bench_fleet_stamp.py [windows ...]"""
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from neo_mpc_planner2_amd import synthetic  # noqa: E402
from neo_mpc_planner2_amd.mpc_optimization_server import README_PARAMS  # noqa: E402
from neo_mpc_planner2_amd.solver import BatchSolver  # noqa: E402

counts = [int(a) for a in sys.argv[1:]] or [4096, 65535]
dev = "cuda:0"
RES, SIZE = synthetic.RESOLUTION, 200
STAMP = (0.45, 0.9, 3.0)          # inscribed_radius, inflation_radius, cost_scaling_factor
NEIGHBOURS = 4.0                  # other robots whose centre lies in a robot's window, on average
REPS, PER = 6, 5


def timed(fn):
    for _ in range(2):
        fn()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
    for e0, e1 in evs:
        e0.record()
        for _ in range(PER):
            fn()
        e1.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in evs])) / PER


params = dict(README_PARAMS)
params.update(control_steps=3)
rows = []
for count in counts:
    # a uniform fleet with NEIGHBOURS robots per window area
    window_m = SIZE * RES
    side = math.sqrt((count - 1) * window_m * window_m / NEIGHBOURS)
    wsize = int(math.ceil(side / RES)) + 2 * SIZE
    world = torch.zeros((wsize, wsize), dtype=torch.uint8, device=dev)
    rng = np.random.default_rng(13)
    xy = rng.uniform(0.0, side, size=(count, 2))
    poses_h = np.concatenate([xy, rng.uniform(-math.pi, math.pi, size=(count, 1))], 1)
    sample = xy[:: max(1, count // 512)]
    inside = (np.abs(sample[:, None, :] - xy[None, :, :]) <= window_m / 2).all(axis=2).sum(axis=1) - 1
    with BatchSolver(params) as s:
        s.set_world_map(world, RES, -window_m, -window_m)
        poses = torch.from_numpy(poses_h).to(dev)
        origins = (poses[:, :2] - window_m / 2.0).contiguous()
        base = torch.tensor(np.asarray(synthetic.RECT_FOOTPRINT, dtype=np.float64), device=dev)
        roll = lambda: s.roll_costmap_pool(SIZE, SIZE, RES, origins, poses=poses)
        stamp = lambda: s.stamp_fleet(*STAMP, footprint=base, poses=poses)
        roll()
        stamp()
        torch.cuda.synchronize()
        first = s.get_costmap_pool(0, 64)[0]
        roll_ms = timed(roll)
        both_ms = timed(lambda: (roll(), stamp()))
        again_ms = timed(stamp)            # windows that carry the stamps already: the same search, no byte changes
        torch.cuda.synchronize()
    rows.append({"windows": count, "yard_m": side, "others_in_a_window_mean": float(inside.mean()),
                 "stamped_cells_per_window_first_64": float((first == 254).sum() / 64.0),
                 "changed_cells_per_window_first_64": float((first != 0).sum() / 64.0),
                 "roll_ms": roll_ms, "roll_plus_stamp_ms": both_ms, "stamp_ms": both_ms - roll_ms,
                 "stamp_again_ms": again_ms, "stamp_over_roll": (both_ms - roll_ms) / roll_ms})
    del world
    torch.cuda.empty_cache()
print(json.dumps({"kernel": "k_stamp_boxes + k_stamp_fleet", "size": SIZE, "resolution": RES, "footprint": "RECT_FOOTPRINT",
                  "stamp": STAMP, "runs": rows}))
