#!/usr/bin/env python3
"""K7 (rolling windows) on its own: 4096 windows of 200 x 200 cells cut from one 2000 x 2000 world map, at equal and at
2 : 1 resolution (window cells twice the world's).  Beside it, in the same run:
  * the only route to the same pool without K7 -- a torch gather that builds the raw windows in HBM, then
    neo_mpc_set_costmap_pool_device (K3) over them;
  * K3 alone over that raw pool: the yardstick for the write stream (the roll writes the same bytes and reads far fewer).
Every figure is the median of event pairs around 20 back-to-back calls (an event pair around one 100-us call measures
the event records as much as the kernels).  usage: bench_roll_pool.py [windows] [size] [world_size]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from neo_mpc_planner2_amd import synthetic  # noqa: E402
from neo_mpc_planner2_amd.mpc_optimization_server import README_PARAMS  # noqa: E402
from neo_mpc_planner2_amd.solver import BatchSolver  # noqa: E402

count = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
size = int(sys.argv[2]) if len(sys.argv) > 2 else 200
wsize = int(sys.argv[3]) if len(sys.argv) > 3 else 2000
dev = "cuda:0"
WRES = synthetic.RESOLUTION
REPS, PER = 8, 20


def timed(fn):
    for _ in range(5):
        fn()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
    for e0, e1 in evs:
        e0.record()
        for _ in range(PER):
            fn()
        e1.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in evs])) / PER


world, _, wox, woy = synthetic.make_costmap(wsize, seed=7)
border = 16
pitch = (size + 2 * border + 127) // 128 * 128
written = count * pitch * (size + 2 * border)
params = dict(README_PARAMS)
params.update(control_steps=3)
rows = []
with BatchSolver(params) as s:
    d_world = torch.from_numpy(world).to(dev)
    s.set_world_map(d_world, WRES, wox, woy)
    rng = np.random.default_rng(11)
    for ratio in (1, 2):
        res = WRES * ratio
        half = wsize * WRES / 2.0
        # robots over the whole world: windows at its edges hang over them
        poses = torch.from_numpy(np.concatenate([rng.uniform(-half, half, size=(count, 2)), np.zeros((count, 1))], 1)).to(dev)
        origins = (poses[:, :2] - size * res / 2.0).contiguous()
        s.roll_costmap_pool(size, size, res, origins, poses=poses)
        roll_ms = timed(lambda: s.roll_costmap_pool(size, size, res, origins, poses=poses))
        refill_ms = timed(lambda: s.roll_costmap_pool(size, size, res, origins))
        torch.cuda.synchronize()
        rolled = s.get_costmap_pool(0, 8)[0]
        # the route without K7: gather the raw windows with torch (float64 index arithmetic, like the contract's, once per
        # axis), then K3
        final = origins.clone()

        def gather():
            ar = torch.arange(size, device=dev, dtype=torch.float64) + 0.5
            qx = (final[:, 0:1] + ar[None, :] * res - wox) / WRES
            qy = (final[:, 1:2] + ar[None, :] * res - woy) / WRES
            okx, oky = (qx >= 0) & (qx < wsize), (qy >= 0) & (qy < wsize)
            mx, my = qx.clamp(0, wsize - 1).long(), qy.clamp(0, wsize - 1).long()
            raw = d_world[my[:, :, None], mx[:, None, :]]
            return torch.where(oky[:, :, None] & okx[:, None, :], raw, torch.full_like(raw, 255))

        raw = gather()
        gather_ms = timed(gather)
        k3_ms = timed(lambda: s.set_costmap_pool(raw, res, final))
        both_ms = timed(lambda: s.set_costmap_pool(gather(), res, final))
        torch.cuda.synchronize()
        same = bool(np.array_equal(s.get_costmap_pool(0, 8)[0], rolled))
        rows.append({"window_to_world_resolution": ratio, "roll_ms": roll_ms, "roll_written_GBps": written / (roll_ms * 1e-3) / 1e9,
                     "refill_without_poses_ms": refill_ms, "torch_gather_ms": gather_ms, "k3_alone_ms": k3_ms,
                     "k3_written_GBps": written / (k3_ms * 1e-3) / 1e9, "torch_gather_plus_k3_ms": both_ms,
                     "roll_over_k3": roll_ms / k3_ms, "first_8_windows_equal_the_gathered_ones": same})
print(json.dumps({"kernel": "k_roll_index + k_roll_fill", "windows": count, "size": size, "world": wsize,
                  "written_bytes": written, "raw_pool_bytes": count * size * size, "world_bytes": wsize * wsize, "runs": rows}))
