"""Transcription of the fleet-stamp contract of include/neo_mpc.h (neo_mpc_stamp_batch): the other robots' outlines written
into each robot's window as lethal cells, with nav2's inflation ring (`InflationLayer::computeCost` and its combination rule
with `inflate_unknown` false) around them.

Written from the contract.  Every float64 `+ - * /` is one NumPy or Python operation -- IEEE float64, correctly rounded,
nothing fused -- in the order the contract writes it; everything else is integer arithmetic, so the library is held to it
by exact equality of uint8 cells.  Two forms: `stamp_window_by_definition` goes through every lattice cell within R of
the window, every robot and every pair of cells, as the text does (small windows only); `stamp_window` restricts each
robot's test to the cells around its bounding box and takes the minimum over the pairs row by row (min over dy of
dy^2 + the distance to the row's nearest stamped cell, squared) -- the same integers; tests/test_fleet_stamp.py holds the
second to the first.  Helper module: no tests in here."""
import math

import numpy as np

FAR = 1 << 20          # "no stamped cell": larger than any squared distance that matters


def inflation_costs(resolution, inscribed_radius, inflation_radius, cost_scaling_factor):
    """(T uint8 [R^2 + 1], R): T[n] is the cost of a cell whose nearest stamped cell is sqrt(n) cells away."""
    res, ins, csf = float(resolution), float(inscribed_radius), float(cost_scaling_factor)
    reach = int(math.ceil(float(inflation_radius) / res))
    table = np.zeros(reach * reach + 1, dtype=np.uint8)
    table[0] = 254
    for n in range(1, reach * reach + 1):
        dist = math.sqrt(n) * res
        if dist <= ins:
            table[n] = 253
        else:
            factor = math.exp(-csf * (dist - ins))
            table[n] = int(252 * factor)              # (uint8)(252 * factor): truncation of a value in [0, 252]
    return table, reach


def stamped(polygon, ox, oy, res, i, l):
    """Which of the lattice cells (i, l) -- integer arrays that broadcast against each other -- robot `polygon` [n, 2]
    stamps: the cell's centre is inside or on the polygon, either winding."""
    polygon = np.asarray(polygon, dtype=np.float64)
    shape = np.broadcast(i, l).shape
    if not np.isfinite(polygon).all():
        return np.zeros(shape, dtype=bool)
    cx = ox + (np.asarray(i, dtype=np.float64) + 0.5) * res
    cy = oy + (np.asarray(l, dtype=np.float64) + 0.5) * res
    pos, neg = np.ones(shape, dtype=bool), np.ones(shape, dtype=bool)
    n = len(polygon)
    with np.errstate(invalid="ignore", over="ignore"):
        for e in range(n):
            a, b = polygon[e], polygon[(e + 1) % n]
            c = (b[0] - a[0]) * (cy - a[1]) - (b[1] - a[1]) * (cx - a[0])
            pos &= c >= 0
            neg &= c <= 0
    return pos | neg


def combine(old, dist2, table, reach):
    """nav2's inflation rule on `old` (uint8 array) for the squared distances `dist2` (int array, same shape)."""
    hit = dist2 <= reach * reach
    c = table[np.where(hit, dist2, 0)].astype(np.int32)
    o = old.astype(np.int32)
    new = np.where(o == 255, np.where(c >= 253, c, 255), np.maximum(o, c))
    return np.where(hit, new, o).astype(np.uint8)


def stamp_window_by_definition(cells, origin, res, polygons, table, reach):
    """The contract, literally: every lattice cell within `reach` of the window is tested against every polygon of
    `polygons` (the OTHER robots), N is the minimum over all pairs.  For small windows."""
    size_y, size_x = cells.shape
    ox, oy, res = float(origin[0]), float(origin[1]), float(res)
    i = np.arange(-reach, size_x + reach)[None, :]
    l = np.arange(-reach, size_y + reach)[:, None]
    dist2 = np.full((size_y, size_x), FAR, dtype=np.int64)
    for polygon in polygons:
        ls, is_ = np.nonzero(stamped(polygon, ox, oy, res, i, l))
        for sl, si in zip(ls - reach, is_ - reach):
            d = (np.arange(size_x)[None, :] - si) ** 2 + (np.arange(size_y)[:, None] - sl) ** 2
            dist2 = np.minimum(dist2, d)
    return combine(cells, dist2, table, reach)


def stamp_window(cells, origin, res, polygons, table, reach):
    """The same window, faster: returns (new cells, squared distances with FAR where nothing is in reach)."""
    size_y, size_x = cells.shape
    ox, oy, res = float(origin[0]), float(origin[1]), float(res)
    width, height = size_x + 2 * reach, size_y + 2 * reach
    union = np.zeros((height, width), dtype=bool)          # lattice cells [-reach, size + reach): index + reach
    for polygon in polygons:
        polygon = np.asarray(polygon, dtype=np.float64)
        if not np.isfinite(polygon).all():
            continue
        # the cells whose centre can lie in the polygon's bounding box, two cells of slack
        q0 = (polygon.min(axis=0) - (ox, oy)) / res
        q1 = (polygon.max(axis=0) - (ox, oy)) / res
        lo = np.maximum(np.floor(q0) - 2, -reach)
        hi = np.minimum(np.floor(q1) + 2, (size_x - 1 + reach, size_y - 1 + reach))
        if lo[0] > hi[0] or lo[1] > hi[1]:
            continue
        i = np.arange(int(lo[0]), int(hi[0]) + 1)[None, :]
        l = np.arange(int(lo[1]), int(hi[1]) + 1)[:, None]
        union[int(lo[1]) + reach:int(hi[1]) + reach + 1, int(lo[0]) + reach:int(hi[0]) + reach + 1] |= \
            stamped(polygon, ox, oy, res, i, l)
    dist2 = np.full((size_y, size_x), FAR, dtype=np.int64)
    if not union.any():
        return cells.copy(), dist2
    col = np.arange(width)[None, :]
    left = np.maximum.accumulate(np.where(union, col, -FAR), axis=1)               # nearest stamped column at or left of
    right = np.minimum.accumulate(np.where(union, col, FAR)[:, ::-1], axis=1)[:, ::-1]      # ... at or right of
    along = np.minimum(col - left, right - col)[:, reach:reach + size_x].astype(np.int64)   # per lattice row, window columns
    along2 = np.where(along >= FAR // 2, FAR, along * along)
    for dy in range(-reach, reach + 1):
        rows = along2[reach + dy:reach + dy + size_y]      # lattice row l + dy for window row l
        dist2 = np.minimum(dist2, np.where(rows >= FAR, FAR, rows + dy * dy))
    return combine(cells, dist2, table, reach), dist2


def stamp_pool(cells, origins, res, polygons, inscribed_radius, inflation_radius, cost_scaling_factor, want_dist2=False):
    """The whole fleet: window k of `cells` [count, size_y, size_x] with origins[k] gets every robot but k."""
    table, reach = inflation_costs(res, inscribed_radius, inflation_radius, cost_scaling_factor)
    polygons = np.asarray(polygons, dtype=np.float64)
    out, dist = np.empty_like(cells), []
    for k in range(len(cells)):
        others = [polygons[j] for j in range(len(polygons)) if j != k]
        out[k], d = stamp_window(cells[k], origins[k], res, others, table, reach)
        dist.append(d)
    return (out, np.stack(dist)) if want_dist2 else out
