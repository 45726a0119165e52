#!/usr/bin/env python3
"""K11 (the laser projection) and the scan update fed from ranges: 4096 robots with two scanners of 1081 beams each -- 8.9 M
beams a scan -- in windows of 200 x 200 cells at 5 cm, the pool shape of bench_scan_layer.py.  Measured, in one process:
  project            k_laser_project alone into caller's buffers (HIP events around back-to-back calls);
  update_from_ranges the whole neo_mpc_update_scan_layer_from_ranges_device: projection, shift, clear, mark, apply;
  update_from_points neo_mpc_update_scan_layer_device on points that are on the device already, one scanner's worth (1081
                     points a robot) and both scanners' as ONE observation of 2162 points seen from the front scanner (not
                     the contract's result -- the rear points get the wrong origin -- but the same rays' worth of work): what
                     the update costs without the projection;
  host alternative   what a caller did before K11: NumPy projection of every beam on the host, then the points uploaded
                     through neo_mpc_update_scan_layer, one call a scanner (wall clock around calls that end synchronised).
Every figure is given as median [min, max] over the repetitions.  Nothing rolls in between, so every update after the first
meets the layers it left.  The bytes K11 must move are counted from the shapes: 4 read and 16 written per beam (the beam
tables, 35 KB, stay in L2).
usage: bench_laser_scan.py [robots [beams]]"""
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from neo_mpc_planner2_amd import synthetic  # noqa: E402
from neo_mpc_planner2_amd.mpc_optimization_server import README_PARAMS  # noqa: E402
from neo_mpc_planner2_amd.solver import BatchSolver, laser_beam_table  # noqa: E402

count = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
beams = int(sys.argv[2]) if len(sys.argv) > 2 else 1081
dev = "cuda:0"
RES, SIZE, SOURCES = synthetic.RESOLUTION, 200, 2
INFLATION = (0.45, 0.9, 3.0)      # inscribed_radius, inflation_radius, cost_scaling_factor
RANGES = dict(obstacle_max_range=4.0, raytrace_max_range=4.5)
REPS, PER, HOST_REPS = 8, 5, 3
INCREMENT = 1.5 * math.pi / (beams - 1)             # 270 degrees
SCANNERS = [dict(mount_x=0.3, mount_y=0.0, mount_yaw=0.0, angle_min=-0.75 * math.pi, angle_increment=INCREMENT, range_min=0.05,
                 range_max=30.0, flags=1),
            dict(mount_x=-0.3, mount_y=0.0, mount_yaw=math.pi, angle_min=-0.75 * math.pi, angle_increment=INCREMENT, range_min=0.05,
                 range_max=30.0, flags=1)]


def spread(ms):
    return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}


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
    return spread([a.elapsed_time(b) / PER for a, b in evs])


def host_projection(ranges, poses, tables):
    """The contract's projection on whole arrays, float64 -> points [sources, count, beams, 2], origins [sources, count, 2]:
    a scanner's points lie together, as the one-observation update takes them."""
    r = ranges.astype(np.float64)
    points = np.empty((len(SCANNERS), ranges.shape[0], ranges.shape[2], 2))
    origins = np.empty((len(SCANNERS), ranges.shape[0], 2))
    S, C = np.sin(poses[:, 2])[:, None], np.cos(poses[:, 2])[:, None]
    x, y = poses[:, 0][:, None], poses[:, 1][:, None]
    for s, sc in enumerate(SCANNERS):
        rs = np.where(np.isposinf(r[:, s]) & bool(sc["flags"] & 1), sc["range_max"] - 1e-4, r[:, s])
        rs = np.where((rs >= sc["range_min"]) & (rs < sc["range_max"]), rs, np.nan)
        bx, by = sc["mount_x"] + rs * tables[s][None, :, 0], sc["mount_y"] + rs * tables[s][None, :, 1]
        points[s, :, :, 0], points[s, :, :, 1] = (x + bx * C) - by * S, (y + bx * S) + by * C
        origins[s, :, 0] = (x + sc["mount_x"] * C - sc["mount_y"] * S)[:, 0]
        origins[s, :, 1] = (y + sc["mount_x"] * S + sc["mount_y"] * C)[:, 0]
    return points, origins


params = dict(README_PARAMS)
params.update(control_steps=3)
window_m = SIZE * RES
side = math.sqrt(count) * window_m / 2.0
wsize = int(math.ceil(side / RES)) + 2 * SIZE
world = torch.zeros((wsize, wsize), dtype=torch.uint8, device=dev)
rng = np.random.default_rng(13)
h_poses = np.concatenate([rng.uniform(0.0, side, size=(count, 2)), rng.uniform(-math.pi, math.pi, size=(count, 1))], 1)
h_ranges = rng.uniform(0.5, 4.5, size=(count, SOURCES, beams)).astype(np.float32)
h_ranges[:, :, ::50] = np.inf                       # beams that met nothing
poses, ranges = torch.from_numpy(h_poses).to(dev), torch.from_numpy(h_ranges).to(dev)
points = torch.zeros((count, SOURCES, beams, 2), dtype=torch.float64, device=dev)
sensors = torch.zeros((count, SOURCES, 2), dtype=torch.float64, device=dev)
tables = [laser_beam_table(sc, beams) for sc in SCANNERS]
out = {"kernel": "k_laser_project", "robots": count, "sources": SOURCES, "beams": beams, "size": SIZE, "resolution": RES,
       "inflation": INFLATION, "reps": REPS, "calls_per_rep": PER, "host_reps": HOST_REPS}
with BatchSolver(params) as s:
    s.set_world_map(world, RES, -window_m, -window_m)
    origins = (poses[:, :2] - window_m / 2.0).contiguous()
    s.roll_costmap_pool(SIZE, SIZE, RES, origins, poses=poses)
    project = lambda: s.project_laser(ranges, poses, SCANNERS, points_out=points, origins_out=sensors)
    from_ranges = lambda: s.update_scan_layer_from_ranges(*INFLATION, ranges, poses, SCANNERS, **RANGES)
    project()
    from_ranges()
    torch.cuda.synchronize()
    # the device's projection against the host's: the same formulas, NumPy's sin and cos of the yaw
    want = host_projection(h_ranges, h_poses, tables)
    got = points.cpu().numpy().transpose(1, 0, 2, 3)
    assert np.array_equal(np.isnan(got), np.isnan(want[0]))
    out["max_abs_difference_to_numpy_m"] = float(np.nanmax(np.abs(got - want[0])))
    out["project_ms"] = timed(project)
    moved = count * SOURCES * beams * 20
    out["project_bytes"] = moved
    out["project_GB_per_s_at_median"] = moved / out["project_ms"]["median"] / 1e6
    out["update_from_ranges_ms"] = timed(from_ranges)
    one = points[:, 0].contiguous()
    both = points.reshape(count, SOURCES * beams, 2)
    front = sensors[:, 0].contiguous()
    out["update_from_points_one_scanner_ms"] = timed(lambda: s.update_scan_layer(*INFLATION, points=one, sensor_origins=front, **RANGES))
    out["update_from_points_both_as_one_observation_ms"] = timed(lambda: s.update_scan_layer(*INFLATION, points=both, sensor_origins=front, **RANGES))
    # the host alternative: wall clock, every call ends synchronised
    torch.cuda.synchronize()
    project_s, upload_s = [], []
    for _ in range(HOST_REPS):
        t0 = time.perf_counter()
        h_points, h_origins = host_projection(h_ranges, h_poses, tables)
        t1 = time.perf_counter()
        for k in range(SOURCES):
            s.update_scan_layer(*INFLATION, points=h_points[k], sensor_origins=h_origins[k], **RANGES)
        t2 = time.perf_counter()
        project_s.append(1e3 * (t1 - t0))
        upload_s.append(1e3 * (t2 - t1))
    out["host_numpy_projection_ms"] = spread(project_s)
    out["host_update_from_points_two_calls_ms"] = spread(upload_s)
    out["host_alternative_ms"] = spread(np.add(project_s, upload_s))
    out["points_bytes"] = count * SOURCES * beams * 16
    out["ranges_bytes"] = count * SOURCES * beams * 4
print(json.dumps(out))
