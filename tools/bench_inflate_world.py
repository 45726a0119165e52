#!/usr/bin/env python3
"""K9 (the world inflation) on its own, with HIP events: a world map of 2000 x 2000 cells at 5 cm, R = 18 cells (0.9 m), at
three seed patterns -- an empty map, a yard (outer walls, rows of shelves, a few pallets) and 3 % random seeds.  Beside it,
in the same process and on the same map: neo_mpc_set_world_map_device's device-to-device copy, the scale to read the kernel
against -- both are one pass over four million cells.  Every figure is the median of event pairs around back-to-back calls
(an event pair around one short call measures the event records as much as the kernel).  The raw map is set again before
every timed inflation, so K9 always meets an uninflated map, and the copy's own time is taken out: `inflate_ms` is the
difference of two medians, copy + inflate less copy, and so carries the launch gaps of two back-to-back calls, not of one
(on the empty map they are a good part of it).  An inflation of the
inflated map -- every search runs, no byte changes -- is printed separately and is not the figure.
usage: bench_inflate_world.py [size]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from neo_mpc_planner2_amd.mpc_optimization_server import README_PARAMS  # noqa: E402
from neo_mpc_planner2_amd.solver import BatchSolver  # noqa: E402

SIZE = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
RES = 0.05
INFLATION = (0.45, 0.9, 3.0)      # inscribed_radius, inflation_radius, cost_scaling_factor
REPS, PER = 8, 5
dev = "cuda:0"


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


def yard(size):
    """Outer walls two cells thick, rows of shelves (1.2 m x 12 m, aisles of 3 m) and a hundred pallets of 0.8 m."""
    cells = np.zeros((size, size), dtype=np.uint8)
    cells[:2, :] = cells[-2:, :] = cells[:, :2] = cells[:, -2:] = 254
    for y in range(100, size - 340, 300):
        for x in range(100, size - 124, 84):
            cells[y:y + 240, x:x + 24] = 254
    rng = np.random.default_rng(3)
    for x, y in rng.integers(40, size - 60, size=(100, 2)):
        cells[y:y + 16, x:x + 16] = 254
    return cells


def random_seeds(size):
    return np.where(np.random.default_rng(4).random((size, size)) < 0.03, 254, 0).astype(np.uint8)


patterns = (("empty", np.zeros((SIZE, SIZE), dtype=np.uint8)), ("yard", yard(SIZE)), ("3 % random seeds", random_seeds(SIZE)))
params = dict(README_PARAMS)
params.update(control_steps=3)
rows = []
with BatchSolver(params) as s:
    for name, cells in patterns:
        raw = torch.from_numpy(cells).to(dev)
        copy = lambda: s.set_world_map(raw, RES, 0.0, 0.0)
        inflate = lambda: s.inflate_world_map(*INFLATION)
        copy()
        inflate()
        torch.cuda.synchronize()
        after = s.get_world_map()[0]
        copy_ms = timed(copy)
        both_ms = timed(lambda: (copy(), inflate()))
        again_ms = timed(inflate)          # the inflated map inflated again: not the figure
        rows.append({"pattern": name, "seeds": int((cells == 254).sum()), "cells_changed": int((after != cells).sum()),
                     "copy_ms": copy_ms, "copy_plus_inflate_ms": both_ms, "inflate_ms": both_ms - copy_ms,
                     "inflate_over_copy": (both_ms - copy_ms) / copy_ms, "inflate_again_ms": again_ms})
        del raw
print(json.dumps({"kernel": "k_inflate_world", "world": "%d x %d cells at %g m" % (SIZE, SIZE, RES), "inflation": INFLATION,
                  "reach_cells": BatchSolver.inflation_costs(RES, *INFLATION)[1], "runs": rows}))
