"""nav2's `FootprintCollisionChecker<Costmap2D*>::footprintCostAtPose` (Humble) with `nav2_util::LineIterator` and
`Costmap2D::worldToMap`, transcribed statement by statement in pure Python -- the executable form of the contract in
include/neo_mpc.h (neo_mpc_footprint_batch).  nav2 is not a dependency of this repository, so this transcription IS the
reference of the footprint gate (K6): it walks every edge with LineIterator's iterative num/den loop and folds the edges
in nav2's order, where the kernel uses a closed form and wave-wide reductions.  Helper module: no tests in here."""
import math

import numpy as np

LETHAL = 254


def oriented(pose, polygon):
    """footprintCostAtPose: the base-frame polygon placed at (x, y, theta), float64."""
    x, y, th = (float(v) for v in pose)
    c, s = math.cos(th), math.sin(th)
    return [(x + px * c - py * s, y + px * s + py * c) for px, py in np.asarray(polygon, dtype=np.float64)]


def world_to_map(wx, wy, size_x, size_y, resolution, origin_x, origin_y):
    """Costmap2D::worldToMap -> (mx, my), or None when the point is off the map."""
    if not (math.isfinite(wx) and math.isfinite(wy)):
        return None
    if wx < origin_x or wy < origin_y:
        return None
    mx = int((wx - origin_x) / resolution)       # static_cast<unsigned int>: truncation of a value >= 0
    my = int((wy - origin_y) / resolution)
    if mx < size_x and my < size_y:
        return mx, my
    return None


def line_cells(x0, y0, x1, y1):
    """nav2_util::LineIterator from (x0, y0) to (x1, y1): the cells it visits, end points included."""
    deltax, deltay = abs(x1 - x0), abs(y1 - y0)
    xinc1 = xinc2 = 1 if x1 >= x0 else -1
    yinc1 = yinc2 = 1 if y1 >= y0 else -1
    if deltax >= deltay:
        xinc1, yinc2 = 0, 0
        den, num, numadd, numpixels = deltax, deltax // 2, deltay, deltax
    else:
        xinc2, yinc1 = 0, 0
        den, num, numadd, numpixels = deltay, deltay // 2, deltax, deltay
    x, y, out = x0, y0, []
    for _ in range(numpixels + 1):               # isValid(): curpixel_ <= numpixels_
        out.append((x, y))
        num += numadd                            # advance()
        if num >= den:
            num -= den
            x += xinc1
            y += yinc1
        x += xinc2
        y += yinc2
    return out


def closed_form_cells(x0, y0, x1, y1):
    """The same cells as a function of the step index alone (what the kernel evaluates, one cell per lane)."""
    dx, dy = abs(x1 - x0), abs(y1 - y0)
    sx, sy = (1 if x1 >= x0 else -1), (1 if y1 >= y0 else -1)
    if dx >= dy:
        return [(x0 + sx * k, y0 + sy * ((dx // 2 + k * dy) // dx if dx else 0)) for k in range(dx + 1)]
    return [(x0 + sx * ((dy // 2 + k * dx) // dy), y0 + sy * k) for k in range(dy + 1)]


def line_cost(cells, x0, y0, x1, y1):
    """lineCost: LETHAL_OBSTACLE as soon as a cell holds it, else the largest raw value on the line."""
    cost = 0
    for x, y in line_cells(x0, y0, x1, y1):
        point = int(cells[y, x])
        if point == LETHAL:
            return LETHAL
        if cost < point:
            cost = point
    return cost


def footprint_cost(cells, resolution, origin_x, origin_y, points):
    """footprintCost: the fold over the outline's edges, in nav2's order."""
    size_y, size_x = cells.shape
    first = world_to_map(points[0][0], points[0][1], size_x, size_y, resolution, origin_x, origin_y)
    if first is None:
        return LETHAL
    cost = 0
    x0, y0 = first
    for j in range(len(points) - 1):
        nxt = world_to_map(points[j + 1][0], points[j + 1][1], size_x, size_y, resolution, origin_x, origin_y)
        if nxt is None:
            return LETHAL
        cost = max(cost, line_cost(cells, x0, y0, nxt[0], nxt[1]))
        x0, y0 = nxt
        if cost == LETHAL:
            return cost
    return max(cost, line_cost(cells, x0, y0, first[0], first[1]))   # the closing edge


def gate(cells, resolution, origins, poses, polygons, map_indices=None):
    """The gate for a batch.  cells [size_y, size_x] with origins = (origin_x, origin_y), or a pool
    cells [maps, size_y, size_x] with origins [maps, 2] and `map_indices`; polygons [points, 2] shared or
    [count, points, 2].  Returns float64 costs [count] on nav2's 0..255 scale."""
    cells, poses, polygons = np.asarray(cells), np.asarray(poses, dtype=np.float64), np.asarray(polygons, dtype=np.float64)
    origins = np.asarray(origins, dtype=np.float64)
    out = np.zeros(len(poses))
    for i, pose in enumerate(poses):
        k = None if cells.ndim == 2 else int(map_indices[i])
        grid, (ox, oy) = (cells, origins) if k is None else (cells[k], origins[k])
        poly = polygons if polygons.ndim == 2 else polygons[i]
        out[i] = footprint_cost(grid, resolution, float(ox), float(oy), oriented(pose, poly))
    return out


def vertex_margin(resolution, origins, poses, polygons, map_indices=None):
    """Smallest distance, in cells, of any oriented vertex of any robot from a cell edge: a vertex that close to an edge
    may land in either cell depending on the last bit of sin / cos, so the exact-equality tests ask for inputs that keep
    every vertex clear of the edges."""
    poses, polygons = np.asarray(poses, dtype=np.float64), np.asarray(polygons, dtype=np.float64)
    origins = np.asarray(origins, dtype=np.float64)
    worst = np.inf
    for i, pose in enumerate(poses):
        ox, oy = origins if origins.ndim == 1 else origins[int(map_indices[i])]
        poly = polygons if polygons.ndim == 2 else polygons[i]
        for X, Y in oriented(pose, poly):
            for q in ((X - ox) / resolution, (Y - oy) / resolution):
                worst = min(worst, abs(q - round(q)))
    return worst
