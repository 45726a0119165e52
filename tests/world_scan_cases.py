"""Generators of cases that the files on the fleet's shared obstacle layer (K12 .. K14) share, and the one case the window
layers (K10) share with it.  Computed once per key, read-only.  No tests here."""
import collections
import functools

import numpy as np

from tests import footprint_gate_reference as gate_ref
from tests import scan_layer_reference as scan_ref
from tests import world_inflation_reference as inflation_ref
from tests import world_scan_layer_reference as ref
from tests.fleet_kit import RECT, inflation_for

#: the last: a width that is no multiple of 4, more than one 64-cell tile each way
WORLDS = {"96x70-5cm": (96, 70, 0.05), "40x40-10cm": (40, 40, 0.1), "130x67-2.5cm": (130, 67, 0.025)}
UPDATE_FLAGS = (ref.CLEAR | ref.MARK, 0, ref.CLEAR)   # three successive updates: a full scan, none, rays alone


def ranges_for(world):
    sx, sy, res = WORLDS[world]
    span = max(sx, sy) * res
    return dict(obstacle_max_range=0.45 * span, obstacle_min_range=3 * res, raytrace_max_range=0.4 * span,
                raytrace_min_range=2 * res)


@functools.lru_cache(maxsize=None)
def case(world, robots, max_points):
    """(cells [sy, sx], wox, woy, per update (points [robots, max_points, 2], point_counts, sensor origins [robots, 2],
    polygons [robots, 4, 2])).  Robot 0: the sensor near the middle, points far beyond every edge and corner, one not
    finite; robot 1: the sensor off the world, its outline partly off it too; the last robot's cloud is ragged.  Everything
    else at random around the sensors, many points outside the world."""
    sx, sy, res = WORLDS[world]
    rng = np.random.default_rng(1000 * sx + 10 * robots + max_points)
    cells = rng.choice(np.array([0, 0, 0, 0, 60, 150, 253, 254, 255, 255, 255], dtype=np.uint8), size=(sy, sx))
    wox, woy = (float(v) for v in rng.uniform(-5.0, 5.0, size=2))
    span = np.array([sx * res, sy * res])
    sensors = np.array([wox, woy]) + span * rng.uniform(0.25, 0.75, size=(robots, 2))
    if robots > 1:
        sensors[1] = np.array([wox, woy]) + span * (-0.05, 0.5)
    angle = rng.uniform(0.0, 2 * np.pi, size=(robots, max_points))
    radius = rng.uniform(0.0, 1.2 * span.max(), size=(robots, max_points))
    points = sensors[:, None, :] + radius[..., None] * np.stack([np.cos(angle), np.sin(angle)], -1)
    counts = np.full(robots, max_points, dtype=np.uint32)
    counts[-1] = max_points - max_points // 3
    if max_points >= 16:
        for j, (dx, dy) in enumerate(((-3, 0.1), (3, -0.1), (0.1, -3), (-0.1, 3), (-3, -3), (3, 3), (-3, 3), (3, -3))):
            points[0, j] = sensors[0] + span * (dx, dy)
        points[0, 8] = (np.nan, sensors[0, 1])
        points[0, 9] = sensors[0] + (res, 0.0)                  # nearer than obstacle_min_range
    points[:, 10 if max_points >= 16 else 0] = sensors + span * (0.2, 0.1)   # every robot marks a cell of the world
    base = np.array(RECT) * (6 * res / 0.35)                    # an outline of about 12 x 8.5 cells
    yaws = rng.uniform(-3.0, 3.0, size=robots)
    polygons = np.array([gate_ref.oriented((sensors[k, 0], sensors[k, 1], yaws[k]), base) for k in range(robots)])
    beyond = sensors[:, None, :] + 1.3 * (points - sensors[:, None, :])   # the third update's rays run through the marks
    for a in (cells, points, counts, sensors, polygons, beyond):
        a.setflags(write=False)
    return cells, wox, woy, ((points, counts, sensors), (None, None, None), (beyond, counts, sensors)), polygons


@functools.lru_cache(maxsize=None)
def expected(world, reach, robots, max_points, unknown, by_definition=False):
    """The transcription on a case: [(layer, live) per update], and the branches taken -- by definition only."""
    cells, wox, woy, updates, polygons = case(world, robots, max_points)
    res = WORLDS[world][2]
    stats = collections.Counter() if by_definition else None
    model, out = ref.WorldScanLayer(), []
    for (points, counts, sensors), flags in zip(updates, UPDATE_FLAGS):
        live = model.update(cells, res, wox, woy, *inflation_for(reach, res), points=points, sensor_origins=sensors,
                            point_counts=counts, flags=flags, clear=dict(polygons=polygons, padding=1.5 * res),
                            unknown_value=unknown, by_definition=by_definition, stats=stats, **ranges_for(world))
        out.append((model.layer.copy(), live.copy()))
    return out, stats


@functools.lru_cache(maxsize=None)
def distance_64_case():
    """193 x 66 free cells of 1/16 m (a layer pitch of 256), seeds at (64, 1) and (64, 65), R = 64: K9's and K10's shared pass
    where a seed is exactly 64 columns away across a tile border on either side, and 64 rows.  -> (world, inflated world,
    parameters, the two scan points [1, 2, 2], sensor origin [1, 2], layers, pool), the cell values asserted by hand."""
    params = inflation_for(64, 0.0625)
    table, reach = inflation_ref.table_for(0.0625, *params)
    assert reach == 64 and table[4096] >= 1                              # (or the arm could not be seen)
    world = np.zeros((66, 193), dtype=np.uint8)
    world[1, 64] = world[65, 64] = 254
    want = inflation_ref.inflate_world(world, 0.0625, *params)
    # the centres of the seeds' cells, seen from the centre of cell (64, 33): 2 m either way, inside the default ranges
    points, sensor = np.array([[(4.03125, 0.09375), (4.03125, 4.09375)]]), np.array([(4.03125, 2.09375)])
    model = scan_ref.ScanLayers()
    pool = model.update(world[None] * 0, np.zeros((1, 2)), 0.0625, *params, points=points, sensor_origins=sensor)
    assert np.argwhere(model.layers[0] == 254).tolist() == [[1, 64], [65, 64]]
    for got in (want, pool[0]):
        # 64 columns to the left and to the right of either seed: T[4096], in those two rows alone; from column 129 on: untouched
        assert got[1, 0] == got[1, 128] == got[65, 0] == got[65, 128] == table[4096] and not got[:, 129:].any()
        assert np.flatnonzero(got[:, 0]).tolist() == np.flatnonzero(got[:, 128]).tolist() == [1, 65]
        # 64 rows from the other seed: each is a seed itself and keeps 254 from there, max(254, T[4096])
        assert got[1, 64] == got[65, 64] == 254 and (got == 254).sum() == 2
    return world, want, params, points, sensor, model.layers, pool
