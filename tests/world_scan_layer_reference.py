"""Transcription of the world-scan-layer contract of include/neo_mpc.h (neo_mpc_fleet_clear, neo_mpc_update_world_scan_layer):
one obstacle layer for the whole fleet on the world map's lattice -- cleared along every robot's rays, marked at their end
points, set free under the robots' own outlines, merged into the world map with updateWithMax and inflated there.

Steps 1, 2 and 4 are the functions of tests/scan_layer_reference.py on the world's geometry -- `clear`, `mark`, `combine_into`,
`inflate_from` and their `_by_definition` forms -- imported, not copied.  Step 3, the footprint-clearing rule, is written here
from the contract's text, twice: `cleared_cell` goes cell by cell and edge by edge as the text does and counts the branches it
takes in `stats`; `cleared` works on whole arrays; tests/test_world_scan_layer.py holds the second to the first.  Every
float64 operation is a NumPy float64 operation, one rounding each, in the order the text writes them.  Helper module: no
tests in here."""
import numpy as np

from tests import scan_layer_reference as scan_ref
from tests.fleet_stamp_reference import inflation_costs

CLEAR, MARK = scan_ref.CLEAR, scan_ref.MARK
FREE, LETHAL, UNKNOWN = scan_ref.FREE, scan_ref.LETHAL, scan_ref.UNKNOWN
F = np.float64


# ------------------------------------------------------------------------------------------ step 3: the footprint-clearing rule
def cleared_cell(polygon, padding, wox, woy, wres, i, l, stats=None):
    """Whether the world cell (i, l) is set free by `polygon` [n, 2], by the contract's text."""
    polygon = np.asarray(polygon, dtype=F)
    if not np.isfinite(polygon).all():
        if stats is not None:
            stats["clear: a vertex is not finite"] += 1
        return False
    padding, wox, woy, wres = F(padding), F(wox), F(woy), F(wres)
    cx, cy = wox + (F(i) + F(0.5)) * wres, woy + (F(l) + F(0.5)) * wres
    pos, neg = True, True
    n = len(polygon)
    with np.errstate(all="ignore"):
        for e in range(n):
            a, b = polygon[e], polygon[(e + 1) % n]
            ex, ey = b[0] - a[0], b[1] - a[1]
            c = ex * (cy - a[1]) - ey * (cx - a[0])
            lim = padding * np.sqrt(ex * ex + ey * ey)
            pos = pos and bool(c >= -lim)
            neg = neg and bool(c <= lim)
    if stats is not None:
        stats["clear: every c_e >= -padding L_e" if pos else "clear: not every c_e >= -padding L_e"] += 1
        stats["clear: every c_e <= padding L_e" if neg else "clear: not every c_e <= padding L_e"] += 1
        if pos and neg:
            stats["clear: both arms"] += 1
    return pos or neg


def cleared(polygon, padding, wox, woy, wres, i, l):
    """The same for integer arrays i, l that broadcast against each other -> a bool array."""
    polygon = np.asarray(polygon, dtype=F)
    shape = np.broadcast(i, l).shape
    if not np.isfinite(polygon).all():
        return np.zeros(shape, dtype=bool)
    padding, wox, woy, wres = F(padding), F(wox), F(woy), F(wres)
    cx = wox + (np.asarray(i, dtype=F) + F(0.5)) * wres
    cy = woy + (np.asarray(l, dtype=F) + F(0.5)) * wres
    pos, neg = np.ones(shape, dtype=bool), np.ones(shape, dtype=bool)
    n = len(polygon)
    with np.errstate(all="ignore"):
        for e in range(n):
            a, b = polygon[e], polygon[(e + 1) % n]
            ex, ey = b[0] - a[0], b[1] - a[1]
            c = ex * (cy - a[1]) - ey * (cx - a[0])
            lim = padding * np.sqrt(ex * ex + ey * ey)
            pos &= c >= -lim
            neg &= c <= lim
    return pos | neg


def clear_footprints_by_definition(layer, wox, woy, wres, polygons, padding, stats=None):
    """Step 3 on the layer, in place: every cell of the world against every polygon."""
    sy, sx = layer.shape
    for polygon in polygons:
        if stats is not None and np.isfinite(polygon).all():
            lo = (np.min(polygon, 0) - (wox, woy)) / wres
            hi = (np.max(polygon, 0) - (wox, woy)) / wres
            if lo[0] < 0 or lo[1] < 0 or hi[0] > sx or hi[1] > sy:
                stats["clear: a polygon reaches beyond the world"] += 1
        for l in range(sy):
            for i in range(sx):
                if cleared_cell(polygon, padding, wox, woy, wres, i, l, stats):
                    layer[l, i] = FREE


def clear_footprints(layer, wox, woy, wres, polygons, padding):
    sy, sx = layer.shape
    i, l = np.arange(sx)[None, :], np.arange(sy)[:, None]
    for polygon in polygons:
        layer[cleared(polygon, padding, wox, woy, wres, i, l)] = FREE


# ------------------------------------------------------------------------------------------ the handle's part
class WorldScanLayer:
    """What the handle keeps next to its world map: the layer, `live`, whether `live` is valid, and what the previous update
    was made for."""

    def __init__(self):
        self.layer, self.live, self.key, self.live_valid = None, None, None, False

    def reset(self):
        self.key, self.live_valid = None, False

    def invalidate(self):
        """neo_mpc_set_world_map / neo_mpc_inflate_world_map."""
        self.live_valid = False

    def roll_source(self, world):
        return self.live if self.live_valid else world

    def update(self, world, wres, wox, woy, inscribed_radius, inflation_radius, cost_scaling_factor, points=None,
               sensor_origins=None, point_counts=None, flags=None, clear=None, obstacle_max_range=2.5, obstacle_min_range=0.0,
               raytrace_max_range=3.0, raytrace_min_range=0.0, unknown_value=255, by_definition=False, stats=None):
        """One update: returns `live`; the layer is in self.layer afterwards.  `points` [count, max_points, 2] with
        `sensor_origins` [count, 2] (and `point_counts`), or [count, sources, beams, 2] with [count, sources, 2]; `clear` = None
        or a mapping with `polygons` [count, n, 2] and `padding`."""
        world = np.asarray(world, dtype=np.uint8)
        sy, sx = world.shape
        if flags is None:
            flags = (CLEAR | MARK) if points is not None else 0
        table, reach = inflation_costs(wres, inscribed_radius, inflation_radius, cost_scaling_factor)
        key = (sx, sy, float(wres), float(wox), float(woy), int(unknown_value))
        if key != self.key:
            self.layer = np.full((sy, sx), unknown_value, dtype=np.uint8)
            if stats is not None:
                stats["reset"] += 1
        self.key = key
        layer = self.layer.copy()
        rays = []                                       # (points [n, 2], sensor origin) per robot and source
        if flags:
            points = np.asarray(points, dtype=F)
            sensors = np.asarray(sensor_origins, dtype=F)
            for k in range(points.shape[0]):
                if points.ndim == 3:
                    n = points.shape[1] if point_counts is None else min(int(point_counts[k]), points.shape[1])
                    rays.append((points[k][:n], sensors[k]))
                else:
                    rays += [(points[k, s], sensors[k, s]) for s in range(points.shape[1])]
        do_clear, do_mark = (scan_ref.clear_by_definition, scan_ref.mark_by_definition) if by_definition else (scan_ref.clear, scan_ref.mark)
        extra = (stats,) if by_definition else ()
        if flags & CLEAR:
            for pts, sensor in rays:
                do_clear(layer, (wox, woy), wres, pts, sensor, raytrace_max_range, raytrace_min_range, *extra)
        if flags & MARK:
            for pts, sensor in rays:
                do_mark(layer, (wox, woy), wres, pts, sensor, obstacle_max_range, obstacle_min_range, *extra)
        if clear is not None:
            if by_definition:
                clear_footprints_by_definition(layer, wox, woy, wres, clear["polygons"], clear["padding"], stats)
            else:
                clear_footprints(layer, wox, woy, wres, clear["polygons"], clear["padding"])
        self.layer = layer
        self.live = scan_ref.inflate_from(scan_ref.combine_into(world, layer, stats), layer, table, reach, stats)
        self.live_valid = True
        return self.live
