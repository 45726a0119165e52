"""Transcription of the scan-layer contract of include/neo_mpc.h (neo_mpc_scan_batch): a persistent obstacle layer per rolling
window -- rolled with its window, cleared along sensor rays, marked at their end points, combined into the window with
updateWithMax and inflated around its own lethal cells.

Written from the contract's text.  Every float64 operation is a NumPy float64 scalar or array operation, one rounding each,
in the order the text writes them (a division by zero gives the IEEE result, as on the device).  The cost table, the
inflation's combination rule and the squared distances to the seeds are the fleet stamp's and the world inflation's and are
imported, not copied.  Two forms of steps 1 to 3: the `*_by_definition` functions go cell by cell and ray by ray as the text
does and count the branches they take in `stats`; the others work on whole arrays; tests/test_scan_layer.py holds the second
to the first.  Helper module: no tests in here."""
import collections

import numpy as np

from tests.fleet_stamp_reference import combine as inflation_combine
from tests.fleet_stamp_reference import inflation_costs
from tests.world_inflation_reference import squared_distances

CLEAR, MARK = 1, 2
FREE, LETHAL, UNKNOWN = 0, 254, 255
F = np.float64


def cell_distance(d, res):
    with np.errstate(all="ignore"):
        return int(min(max(F(0.0), np.ceil(F(d) / F(res))), F(2147483647.0)))


def world_to_map(wx, wy, ox, oy, res, sx, sy):
    """(mx, my), or None where the contract says it fails."""
    wx, wy, ox, oy, res = F(wx), F(wy), F(ox), F(oy), F(res)
    if not (np.isfinite(wx) and np.isfinite(wy)) or wx < ox or wy < oy:
        return None
    with np.errstate(all="ignore"):
        mx, my = np.trunc((wx - ox) / res), np.trunc((wy - oy) / res)
    if not (mx < F(sx) and my < F(sy)):
        return None
    return int(mx), int(my)


# ------------------------------------------------------------------------------------------ step 1: the roll
def shift_of(origin, layer_origin, res, size):
    """The shift along one axis in cells, or None: the whole layer becomes unknown."""
    with np.errstate(all="ignore"):
        q = (F(origin) - F(layer_origin)) / F(res)
    if not np.isfinite(q) or abs(q) >= F(size):
        return None
    return int(np.rint(q))           # nearest, ties to even


def count_shift(stats, cx, cy):
    if stats is None:
        return
    if cx is None or cy is None:
        stats["shift beyond the window"] += 1
        return
    for axis, c in (("x", cx), ("y", cy)):
        stats["shift %s %s" % (axis, "+" if c > 0 else "-" if c < 0 else "0")] += 1


def roll_layer_by_definition(layer, layer_origin, origin, res, unknown, stats=None):
    sy, sx = layer.shape
    cx, cy = shift_of(origin[0], layer_origin[0], res, sx), shift_of(origin[1], layer_origin[1], res, sy)
    count_shift(stats, cx, cy)
    new = np.full_like(layer, unknown)
    if cx is None or cy is None:
        return new
    for l in range(sy):
        for i in range(sx):
            if 0 <= i + cx < sx and 0 <= l + cy < sy:
                new[l, i] = layer[l + cy, i + cx]
    return new


def roll_layer(layer, layer_origin, origin, res, unknown):
    sy, sx = layer.shape
    cx, cy = shift_of(origin[0], layer_origin[0], res, sx), shift_of(origin[1], layer_origin[1], res, sy)
    new = np.full_like(layer, unknown)
    if cx is None or cy is None:
        return new
    i0, i1, l0, l1 = max(0, -cx), min(sx, sx - cx), max(0, -cy), min(sy, sy - cy)
    if i0 < i1 and l0 < l1:
        new[l0:l1, i0:i1] = layer[l0 + cy:l1 + cy, i0 + cx:i1 + cx]
    return new


# ------------------------------------------------------------------------------------------ step 2: the line walk
def raytrace_cells(x0, y0, x1, y1, M, m):
    """The cells raytraceLine clears between the cells (x0, y0) and (x1, y1), in order."""
    Dx, Dy = x1 - x0, y1 - y0
    dist = np.sqrt(F(Dx * Dx + Dy * Dy))
    if dist < F(m):
        return []
    u0, v0 = x0, y0
    if dist > 0:
        u0, v0 = int(F(x0) + F(Dx) / dist * F(m)), int(F(y0) + F(Dy) / dist * F(m))
    dx, dy = x1 - u0, y1 - v0
    step_x, step_y = (1 if dx > 0 else -1), (1 if dy > 0 else -1)
    scale = F(1.0) if dist == 0 else min(F(1.0), F(M) / dist)
    x_major = abs(dx) >= abs(dy)
    A, B = (abs(dx), abs(dy)) if x_major else (abs(dy), abs(dx))
    n = min(M, int(scale * F(A)))
    x, y, e = u0, v0, A // 2
    cells = []
    for _ in range(n):
        cells.append((x, y))
        if x_major:
            x += step_x
        else:
            y += step_y
        e += B
        if e >= A:
            if x_major:
                y += step_y
            else:
                x += step_x
            e -= A
    cells.append((x, y))
    return cells


def clip_point(wx, wy, sx0, sy0, ox, oy, ex, ey, stats=None):
    """Steps 2.1 and 2.2 for one point."""
    wx, wy = F(wx), F(wy)
    a, b = wx - sx0, wy - sy0
    with np.errstate(all="ignore"):
        if wx < ox:
            t = (ox - sx0) / a
            wx, wy = ox, sy0 + b * t
            if stats is not None:
                stats["clip wx < ox"] += 1
        if wy < oy:
            t = (oy - sy0) / b
            wx, wy = sx0 + a * t, oy
            if stats is not None:
                stats["clip wy < oy"] += 1
        if wx > ex:
            t = (ex - sx0) / a
            wx, wy = ex - F(0.001), sy0 + b * t
            if stats is not None:
                stats["clip wx > ex"] += 1
        if wy > ey:
            t = (ey - sy0) / b
            wx, wy = sx0 + a * t, ey - F(0.001)
            if stats is not None:
                stats["clip wy > ey"] += 1
    return wx, wy


def clear_by_definition(layer, origin, res, points, sensor, raytrace_max, raytrace_min, stats=None):
    """Step 2 on one layer, in place."""
    sy, sx = layer.shape
    ox, oy, res, sx0, sy0 = F(origin[0]), F(origin[1]), F(res), F(sensor[0]), F(sensor[1])
    start = world_to_map(sx0, sy0, ox, oy, res, sx, sy)
    if start is None:
        if stats is not None and len(points):
            stats["sensor origin off the map"] += 1
        return
    ex, ey = ox + F(sx) * res, oy + F(sy) * res
    M, m = cell_distance(raytrace_max, res), cell_distance(raytrace_min, res)
    for wx, wy in points:
        if not (np.isfinite(wx) and np.isfinite(wy)):
            if stats is not None:
                stats["point not finite"] += 1
            continue
        cx, cy = clip_point(wx, wy, sx0, sy0, ox, oy, ex, ey, stats)
        end = world_to_map(cx, cy, ox, oy, res, sx, sy)
        if end is None:
            if stats is not None:
                stats["clipped point off the map"] += 1
            continue
        cells = raytrace_cells(start[0], start[1], end[0], end[1], M, m)
        if stats is not None:
            stats["ray dropped by raytrace_min_range" if not cells else "ray walked"] += 1
            stats["ray cut by raytrace_max_range"] += int(bool(cells) and cells[-1] != end)
        for x, y in cells:
            assert 0 <= x < sx and 0 <= y < sy, "the walk left the grid"
            layer[y, x] = FREE


def mark_by_definition(layer, origin, res, points, sensor, obstacle_max, obstacle_min, stats=None):
    """Step 3 on one layer, in place."""
    sy, sx = layer.shape
    sx0, sy0 = F(sensor[0]), F(sensor[1])
    for wx, wy in points:
        wx, wy = F(wx), F(wy)
        if not (np.isfinite(wx) and np.isfinite(wy)):
            continue
        with np.errstate(all="ignore"):
            s = (wx - sx0) * (wx - sx0) + (wy - sy0) * (wy - sy0)
            far, near = s >= F(obstacle_max) * F(obstacle_max), s < F(obstacle_min) * F(obstacle_min)
        cell = None if far or near else world_to_map(wx, wy, origin[0], origin[1], res, sx, sy)
        if stats is not None:
            stats["mark dropped: >= max" if far else "mark dropped: < min" if near else
                  "mark dropped: off the map" if cell is None else "marked"] += 1
            if cell is not None and world_to_map(sx0, sy0, origin[0], origin[1], res, sx, sy) is None:
                stats["marked from a sensor origin off the map"] += 1
        if cell is not None:
            layer[cell[1], cell[0]] = LETHAL


# ------------------------------------------------------------------------------------------ steps 2 and 3 on arrays
def cells_of(wx, wy, ox, oy, res, sx, sy):
    """worldToMap for arrays of points: (ok, mx, my)."""
    with np.errstate(all="ignore"):
        ok = np.isfinite(wx) & np.isfinite(wy) & ~(wx < ox) & ~(wy < oy)
        mx, my = np.trunc((wx - ox) / res), np.trunc((wy - oy) / res)
        ok &= (mx < F(sx)) & (my < F(sy))
    return ok, np.where(ok, mx, 0).astype(np.int64), np.where(ok, my, 0).astype(np.int64)


def clear(layer, origin, res, points, sensor, raytrace_max, raytrace_min):
    sy, sx = layer.shape
    ox, oy, res, sx0, sy0 = F(origin[0]), F(origin[1]), F(res), F(sensor[0]), F(sensor[1])
    start = world_to_map(sx0, sy0, ox, oy, res, sx, sy)
    points = np.asarray(points, dtype=F).reshape(-1, 2)
    if start is None or not len(points):
        return
    ex, ey = ox + F(sx) * res, oy + F(sy) * res
    M, m = cell_distance(raytrace_max, res), cell_distance(raytrace_min, res)
    wx, wy = points[:, 0].copy(), points[:, 1].copy()
    finite = np.isfinite(wx) & np.isfinite(wy)
    a, b = wx - sx0, wy - sy0
    with np.errstate(all="ignore"):
        c = wx < ox
        t = (ox - sx0) / a
        wx, wy = np.where(c, ox, wx), np.where(c, sy0 + b * t, wy)
        c = wy < oy
        t = (oy - sy0) / b
        wx, wy = np.where(c, sx0 + a * t, wx), np.where(c, oy, wy)
        c = wx > ex
        t = (ex - sx0) / a
        wx, wy = np.where(c, ex - F(0.001), wx), np.where(c, sy0 + b * t, wy)
        c = wy > ey
        t = (ey - sy0) / b
        wx, wy = np.where(c, sx0 + a * t, wx), np.where(c, ey - F(0.001), wy)
    ok, x1, y1 = cells_of(wx, wy, ox, oy, res, sx, sy)
    ok &= finite
    x1, y1 = x1[ok], y1[ok]
    x0, y0 = start
    Dx, Dy = x1 - x0, y1 - y0
    dist = np.sqrt((Dx * Dx + Dy * Dy).astype(F))
    keep = ~(dist < F(m))
    x1, y1, Dx, Dy, dist = x1[keep], y1[keep], Dx[keep], Dy[keep], dist[keep]
    with np.errstate(all="ignore"):
        u0 = np.where(dist > 0, F(x0) + Dx.astype(F) / dist * F(m), F(x0)).astype(np.int64)
        v0 = np.where(dist > 0, F(y0) + Dy.astype(F) / dist * F(m), F(y0)).astype(np.int64)
        scale = np.where(dist == 0, F(1.0), np.minimum(F(1.0), F(M) / dist))
    dx, dy = x1 - u0, y1 - v0
    step_x, step_y = np.where(dx > 0, 1, -1), np.where(dy > 0, 1, -1)
    x_major = np.abs(dx) >= np.abs(dy)
    A, B = np.where(x_major, np.abs(dx), np.abs(dy)), np.where(x_major, np.abs(dy), np.abs(dx))
    n = np.minimum(M, (scale * A.astype(F)).astype(np.int64))
    x, y, e = u0.copy(), v0.copy(), A // 2
    for t in range(int(n.max()) if len(n) else 0):
        live = t < n
        layer[y[live], x[live]] = FREE
        x = x + np.where(live & x_major, step_x, 0)
        y = y + np.where(live & ~x_major, step_y, 0)
        e = e + np.where(live, B, 0)
        turn = live & (e >= A)
        y = y + np.where(turn & x_major, step_y, 0)
        x = x + np.where(turn & ~x_major, step_x, 0)
        e = e - np.where(turn, A, 0)
    layer[y, x] = FREE


def mark(layer, origin, res, points, sensor, obstacle_max, obstacle_min):
    sy, sx = layer.shape
    points = np.asarray(points, dtype=F).reshape(-1, 2)
    wx, wy, sx0, sy0 = points[:, 0], points[:, 1], F(sensor[0]), F(sensor[1])
    with np.errstate(all="ignore"):
        s = (wx - sx0) * (wx - sx0) + (wy - sy0) * (wy - sy0)
        ok = ~(s >= F(obstacle_max) * F(obstacle_max)) & ~(s < F(obstacle_min) * F(obstacle_min))
    inside, mx, my = cells_of(wx, wy, F(origin[0]), F(origin[1]), F(res), sx, sy)
    ok &= inside
    layer[my[ok], mx[ok]] = LETHAL


# ------------------------------------------------------------------------------------------ steps 4 and 5
def combine_into(window, layer, stats=None):
    """Step 4: updateWithMax."""
    v, old = layer.astype(np.int32), window.astype(np.int32)
    take = (v != UNKNOWN) & ((old == UNKNOWN) | (old < v))
    if stats is not None:
        stats["combine: v == 255"] += int((v == UNKNOWN).sum())
        stats["combine: old == 255"] += int(((v != UNKNOWN) & (old == UNKNOWN)).sum())
        stats["combine: old < v"] += int(((v != UNKNOWN) & (old != UNKNOWN) & (old < v)).sum())
        stats["combine: old >= v"] += int(((v != UNKNOWN) & (old != UNKNOWN) & (old >= v)).sum())
    return np.where(take, v, old).astype(np.uint8)


def inflate_from(window, layer, table, reach, stats=None):
    """Step 5: the layer's lethal cells are the seeds, the window takes the costs."""
    dist2 = squared_distances(layer, reach)
    if stats is not None:
        hit = dist2 <= reach * reach
        cost = np.where(hit, table[np.where(hit, dist2, 0)], 0).astype(np.int32)
        stats["inflate: old == 255, cost >= 253"] += int((hit & (window == UNKNOWN) & (cost >= 253)).sum())
        stats["inflate: old == 255, cost < 253"] += int((hit & (window == UNKNOWN) & (cost < 253)).sum())
    return inflation_combine(window, dist2, table, reach)


# ------------------------------------------------------------------------------------------ the handle's part
class ScanLayers:
    """What the handle keeps: the layers, their origins and what the previous update was made for."""

    def __init__(self):
        self.layers, self.origins, self.key = None, None, None

    def reset(self):
        self.key = None

    def update(self, cells, origins, res, inscribed_radius, inflation_radius, cost_scaling_factor, points=None,
               sensor_origins=None, point_counts=None, flags=None, obstacle_max_range=2.5, obstacle_min_range=0.0,
               raytrace_max_range=3.0, raytrace_min_range=0.0, unknown_value=255, by_definition=False, stats=None):
        """One update on the pool `cells` [count, sy, sx] at `origins`: returns the new pool; the layers are in
        self.layers / self.origins afterwards.  Arguments as BatchSolver.update_scan_layer."""
        cells = np.asarray(cells, dtype=np.uint8)
        origins = np.asarray(origins, dtype=F)
        count, sy, sx = cells.shape
        if flags is None:
            flags = (CLEAR | MARK) if points is not None else 0
        table, reach = inflation_costs(res, inscribed_radius, inflation_radius, cost_scaling_factor)
        key = (sx, sy, float(res), count, int(unknown_value))
        if key != self.key:
            self.layers = np.full((count, sy, sx), unknown_value, dtype=np.uint8)
            self.origins = origins.copy()
            if stats is not None:
                stats["reset"] += 1
        self.key = key
        out = np.empty_like(cells)
        layers = np.empty_like(self.layers)
        for k in range(count):
            if by_definition:
                layer = roll_layer_by_definition(self.layers[k], self.origins[k], origins[k], res, unknown_value, stats)
            else:
                layer = roll_layer(self.layers[k], self.origins[k], origins[k], res, unknown_value)
            if flags:
                n = points.shape[1] if point_counts is None else min(int(point_counts[k]), points.shape[1])
                pts = np.asarray(points[k][:n], dtype=F)
                if flags & CLEAR:
                    if by_definition:
                        clear_by_definition(layer, origins[k], res, pts, sensor_origins[k], raytrace_max_range, raytrace_min_range, stats)
                    else:
                        clear(layer, origins[k], res, pts, sensor_origins[k], raytrace_max_range, raytrace_min_range)
                if flags & MARK:
                    if by_definition:
                        mark_by_definition(layer, origins[k], res, pts, sensor_origins[k], obstacle_max_range, obstacle_min_range, stats)
                    else:
                        mark(layer, origins[k], res, pts, sensor_origins[k], obstacle_max_range, obstacle_min_range)
            layers[k] = layer
            out[k] = inflate_from(combine_into(cells[k], layer, stats), layer, table, reach, stats)
        self.layers, self.origins = layers, origins.copy()
        return out
