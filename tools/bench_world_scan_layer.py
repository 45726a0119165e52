#!/usr/bin/env python3
"""K12 (the fleet's shared obstacle layer on the world map) with HIP events: a yard of 2000 x 2000 cells at 5 cm, 4096 robots,
R = 18 -- fed from one 360-point observation per robot (the points of bench_scan_layer.py) and from two scanners of 1081 beams
each (the ranges of bench_laser_scan.py).  An update is up to five launches (k_laser_project, k_world_scan_rays clear,
k_world_scan_rays mark, k_world_scan_footprints, k_world_scan_compose); the flags and the clear record pick which run, so
their times are differences of updates that leave the same layer behind: flags 0 is the composition alone, MARK alone adds
the marking launch (on a layer that holds the marks already), CLEAR alone the clearing one (on a layer it has cleared of
marks: the composition then inflates nothing, so flags 0 is timed on both kinds of layer), flags 0 with the record adds the
footprints.  Beside it, for windows of 200 x 200 cells: K7's roll behind an update, and -- unless --alone is given -- the
per-window updates of K10 and K11 from tools/bench_scan_layer.py and tools/bench_laser_scan.py, run as child processes one
after the other on the same card, their JSON taken over as it is.
With --denoise G (may be given more than once), at the end and on the layer of a full scan again: K13's launch
(k_world_scan_denoise, 8-connectivity) as the difference of flags-0 updates with the filter on and off, and how many marks it
dropped.  Without the option the filter is never set and nothing of it runs.
With --decay A (may be given more than once), behind that and on the layer of a full scan again: what K14 adds to an update
without a scan -- its sweep, k_world_scan_decay, as the difference of flags-0 updates with decay on and off -- and to a full
scan update -- k_world_scan_tick, the stamped marking launch in place of the plain one, and the sweep --, both beside the
composition alone measured in the same run; and how many marks the timed scan updates left.  Every robot's scan marks its
cells again in every update, so nothing expires while it is timed: the sweep fetches a stamp under every mark and stores
nothing, which is what it does in a fleet whose scanners run.  Without the option decay is never set and nothing of it runs.
Every figure is median [min, max] of event pairs around back-to-back calls.
usage: bench_world_scan_layer.py [--alone] [--denoise G]... [--decay A]... [robots]"""
import json
import math
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import torch  # noqa: E402

from neo_mpc_planner2_amd import abi, synthetic  # noqa: E402
from neo_mpc_planner2_amd.mpc_optimization_server import README_PARAMS  # noqa: E402
from neo_mpc_planner2_amd.solver import BatchSolver  # noqa: E402

args = [a for a in sys.argv[1:] if a != "--alone"]
alone = "--alone" in sys.argv[1:]
denoise = [int(args[k + 1]) for k, a in enumerate(args) if a == "--denoise"]
decay = [int(args[k + 1]) for k, a in enumerate(args) if a == "--decay"]
args = [a for k, a in enumerate(args) if a not in ("--denoise", "--decay") and (k == 0 or args[k - 1] not in ("--denoise", "--decay"))]
count = int(args[0]) if args else 4096
dev = "cuda:0"
RES, WORLD, SIZE, POINTS, SOURCES, BEAMS = synthetic.RESOLUTION, 2000, 200, 360, 2, 1081
INFLATION = (0.45, 0.9, 3.0)      # inscribed_radius, inflation_radius, cost_scaling_factor: R = 18 at 5 cm
RANGES = dict(obstacle_max_range=4.0, raytrace_max_range=4.5)
PADDING = math.sqrt(2.0) * RES + 0.03
REPS, PER = 8, 5
INCREMENT = 1.5 * math.pi / (BEAMS - 1)             # 270 degrees
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


def minus(a, b):
    """A launch as the difference of two updates: of the medians, with the spread of both left to the reader."""
    return {"median": a["median"] - b["median"], "of": [a, b]}


params = dict(README_PARAMS)
params.update(control_steps=3)
side = WORLD * RES
world = torch.zeros((WORLD, WORLD), dtype=torch.uint8, device=dev)
rng = np.random.default_rng(13)
h_poses = np.concatenate([rng.uniform(5.0, side - 5.0, size=(count, 2)), rng.uniform(-math.pi, math.pi, size=(count, 1))], 1)
poses = torch.from_numpy(h_poses).to(dev)
angle = torch.linspace(0.0, 2 * math.pi, POINTS + 1, dtype=torch.float64, device=dev)[:-1]
reach = torch.from_numpy(rng.uniform(0.5, 4.5, size=(count, POINTS))).to(dev)
sensors = poses[:, :2].contiguous()
points = (sensors[:, None, :] + reach[..., None] * torch.stack([torch.cos(angle), torch.sin(angle)], -1)[None]).contiguous()
h_ranges = rng.uniform(0.5, 4.5, size=(count, SOURCES, BEAMS)).astype(np.float32)
h_ranges[:, :, ::50] = np.inf                       # beams that met nothing
ranges = torch.from_numpy(h_ranges).to(dev)
footprint = torch.tensor(np.asarray(synthetic.RECT_FOOTPRINT, dtype=np.float64), device=dev)
out = {"kernel": "k_world_scan_rays + k_world_scan_footprints + k_world_scan_compose", "robots": count, "world": WORLD,
       "resolution": RES, "inflation": INFLATION, "points_per_robot": POINTS, "sources": SOURCES, "beams": BEAMS,
       "window": SIZE, "padding": PADDING, "reps": REPS, "calls_per_rep": PER}
with BatchSolver(params) as s:
    s.set_world_map(world, RES, 0.0, 0.0)
    origins = (poses[:, :2] - SIZE * RES / 2.0).contiguous()
    clear = dict(footprint=footprint, poses=poses, padding=PADDING)
    roll = lambda: s.roll_costmap_pool(SIZE, SIZE, RES, origins, poses=poses)
    update = lambda flags, **kw: s.update_world_scan_layer(*INFLATION, points=points, sensor_origins=sensors, flags=flags,
                                                           **RANGES, **kw)
    from_ranges = lambda **kw: s.update_world_scan_layer_from_ranges(*INFLATION, ranges, poses, SCANNERS, **RANGES, **kw)
    update(abi.SCAN_CLEAR | abi.SCAN_MARK)
    roll()
    torch.cuda.synchronize()
    layer, live = s.get_world_scan_layer()
    out["marks_per_robot"] = float((layer == 254).sum()) / count
    out["free_layer_cells_per_robot"] = float((layer == 0).sum()) / count
    out["world_cells_changed"] = int((live != 0).sum())
    out["roll_ms"] = timed(roll)
    # a layer that holds the marks of a full scan: the composition inflates around them
    out["update_full_ms"] = timed(lambda: update(abi.SCAN_CLEAR | abi.SCAN_MARK))
    out["update_full_with_footprints_ms"] = timed(lambda: update(abi.SCAN_CLEAR | abi.SCAN_MARK, clear=clear))
    update(abi.SCAN_CLEAR | abi.SCAN_MARK)          # (the marks under the hulls back in place)

    def full_and_roll():
        update(abi.SCAN_CLEAR | abi.SCAN_MARK)
        roll()

    out["update_full_plus_roll_ms"] = timed(full_and_roll)
    compose = timed(lambda: update(0))
    out["compose_ms"] = compose
    out["mark_ms"] = minus(timed(lambda: update(abi.SCAN_MARK)), compose)   # (marks the cells that are marked: the same layer)
    # a layer without a lethal cell -- CLEAR alone clears the marks its rays end on: the composition inflates nothing
    update(abi.SCAN_CLEAR)
    torch.cuda.synchronize()
    out["marks_left_by_clear_alone"] = int((s.get_world_scan_layer()[0] == 254).sum())
    compose_free = timed(lambda: update(0))
    out["compose_no_lethal_cell_ms"] = compose_free
    out["clear_ms"] = minus(timed(lambda: update(abi.SCAN_CLEAR)), compose_free)
    out["footprints_ms"] = minus(timed(lambda: update(0, clear=clear)), compose_free)
    # from ranges: both scanners of every robot, projection included
    from_ranges()
    torch.cuda.synchronize()
    layer = s.get_world_scan_layer()[0]
    out["from_ranges_marks_per_robot"] = float((layer == 254).sum()) / count
    out["update_from_ranges_ms"] = timed(from_ranges)
    out["update_from_ranges_with_footprints_ms"] = timed(lambda: from_ranges(clear=clear))

    def ranges_and_roll():
        from_ranges()
        roll()

    out["update_from_ranges_plus_roll_ms"] = timed(ranges_and_roll)
    p_out = torch.zeros((count, SOURCES, BEAMS, 2), dtype=torch.float64, device=dev)
    o_out = torch.zeros((count, SOURCES, 2), dtype=torch.float64, device=dev)
    out["project_ms"] = timed(lambda: s.project_laser(ranges, poses, SCANNERS, points_out=p_out, origins_out=o_out))
    torch.cuda.synchronize()
    for group in denoise:
        # the filter, on the layer of a full scan of points: flags 0 with it against flags 0 without, the same layer
        update(abi.SCAN_CLEAR | abi.SCAN_MARK)
        off = timed(lambda: update(0))
        s.set_world_scan_denoise(group, 8)
        update(0)                                   # (allocates D)
        on = timed(lambda: update(0))
        torch.cuda.synchronize()
        layer, kept = s.get_world_scan_layer()[0], s.get_world_scan_denoised()
        s.set_world_scan_denoise(0)
        out["denoise_%d" % group] = {"minimal_group_size": group, "connectivity": 8, "marks": int((layer == 254).sum()),
                                     "marks_dropped": int(((layer == 254) & (kept == 0)).sum()),
                                     "compose_with_filter_ms": on, "denoise_ms": minus(on, off)}
    for max_age in decay:
        # decay, on the layer of a full scan of points: updates with it against the same updates without, the same layer
        update(abi.SCAN_CLEAR | abi.SCAN_MARK)
        off, full_off = timed(lambda: update(0)), timed(lambda: update(abi.SCAN_CLEAR | abi.SCAN_MARK))
        s.set_world_scan_decay(max_age)
        update(0)                                   # (allocates the stamps and the clock, and fills the stamps)
        on, full_on = timed(lambda: update(0)), timed(lambda: update(abi.SCAN_CLEAR | abi.SCAN_MARK))
        torch.cuda.synchronize()
        layer, ages = s.get_world_scan_layer()[0], s.get_world_scan_ages()
        s.set_world_scan_decay(0)
        update(0)
        out["decay_%d" % max_age] = {"max_age": max_age, "marks": int((layer == 254).sum()),
                                     "oldest_mark": int(ages[layer == 254].max()), "stamp_bytes": int(ages.nbytes),
                                     "compose_ms": off, "compose_with_decay_ms": on, "decay_sweep_ms": minus(on, off),
                                     "update_full_ms": full_off, "update_full_with_decay_ms": full_on,
                                     "decay_in_a_scan_update_ms": minus(full_on, full_off)}
del world, points, ranges
torch.cuda.empty_cache()
if not alone:
    # the per-window layers, by their own tools, one fresh process after the other on this card
    for name, argv in (("bench_scan_layer", ["bench_scan_layer.py", str(count)]), ("bench_laser_scan", ["bench_laser_scan.py", str(count)])):
        run = subprocess.run([sys.executable, os.path.join(HERE, argv[0])] + argv[1:], capture_output=True, text=True, timeout=900)
        line = [ln for ln in run.stdout.splitlines() if ln.startswith("{")]
        out[name] = json.loads(line[-1]) if run.returncode == 0 and line else {"failed": run.returncode, "stderr": run.stderr[-400:]}
print(json.dumps(out))
