"""Probes of the solver's view of the costmap, cell by cell (tests/test_costmap_cells.py).

With control_steps = 1 and u = 0 the objective (py:204-269; k_objective in neo_mpc_kernels.hip, orc_objective in
oracle/mpc_oracle.c) moves nowhere -- the increments of py:235-236 are 0 * cos * dt - 0 * sin * dt, exact zeros -- and looks up
exactly the cell of `cur_xy`.  With the carrot, the goal and the velocity at zero and identity quaternions every other term of
the objective is an exact zero as well: the value IS the costmap term of that one cell, 1000 for a lethal cell (or the outside
of the map), w_costmap * (occupancy / 100)^2 otherwise.  One request per target cell then reads the map as the solver sees it:
the interior, the border K3 wrote around it (costmap.h map_raw reads it from memory) and the cells beyond, which the bounds
test makes lethal.

Nothing here touches the device: the requests, the patterned maps, the model of K3's load paths and the robots of the reach-tile
test are plain NumPy; the reference is oracle/c_oracle.objective_batch.
"""
import numpy as np

from neo_mpc_planner2_amd import abi, synthetic
from oracle import mpc_oracle

#: raw cell values with pairwise different occupancies (costmap.h raw_occupancy: 0, 1, 98, 99, 100, 23, 50, 77) -- so with
#: pairwise different costmap terms.  255 (occupancy -1) squares to the term of raw 1 ... 3 and stays out: the round trips of
#: random bytes carry it.
PATTERN = (0, 1, 252, 253, 254, 60, 130, 200)
#: how far a move of the probe to another cell must change the reference objective, relative: the comparison's tolerance is
#: 1e-12, so a wrong cell on the device cannot hide in it
DISCRIMINATES = 1e-6


def occupancy(raw):
    """costmap.h raw_occupancy / mpc_oracle.c orc_occupancy for an array of raw values"""
    return mpc_oracle.nav2_occupancy_table()[np.asarray(raw, dtype=np.int64)]


def pattern_map(size_x, size_y, shift=0):
    """uint8 [size_y, size_x] of PATTERN[(3 mx + 7 my + shift) % 8]: a step along x moves the index by 3, one along y by 7,
    neither a multiple of 8 -- every cell's occupancy differs from that of its four neighbours"""
    mx, my = np.meshgrid(np.arange(size_x), np.arange(size_y))
    return np.array(PATTERN, dtype=np.uint8)[(3 * mx + 7 * my + shift) % len(PATTERN)]


def parity_map(size_x, size_y, axis):
    """uint8 [size_y, size_x]: raw 0 in the even and 253 in the odd columns (axis 0) or rows (axis 1): a cell differs from both
    neighbours along the axis, and both values differ from the lethal outside"""
    mx, my = np.meshgrid(np.arange(size_x), np.arange(size_y))
    return np.where((mx if axis == 0 else my) % 2 == 0, 0, 253).astype(np.uint8)


def probe_params(**over):
    """the README's parameters at control_steps 1"""
    return mpc_oracle.make_params(control_steps=1, **over)


def cell_of(w, origin, resolution):
    """the reference's world -> cell, floor((w - origin) / resolution), in float64"""
    return np.floor((np.asarray(w, dtype=np.float64) - origin) / resolution)


def cell_centres(origin, resolution, cells):
    """origin + (m + 0.5) * resolution for the cell indices `cells`, each checked in float64 to floor back to its cell; one that
    does not (the sum rounds by more than half a cell only where an ulp of the position is of a cell's size) is nudged towards
    its cell's centre"""
    m = np.asarray(cells, dtype=np.float64)
    w = origin + (m + 0.5) * resolution
    for _ in range(4):
        q = (w - origin) / resolution
        bad = np.floor(q) != m
        if not bad.any():
            return w
        w = np.where(bad, w + (m + 0.5 - q) * resolution, w)
    raise AssertionError("no float64 position lands in cells %s at origin %r, resolution %r" % (m[bad][:4], origin, resolution))


def requests(x, y, map_index=0):
    """one request per position: everything but `cur_xy` (and the map of a pool) at rest"""
    x, y = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
    p = np.zeros(x.size, dtype=abi.PROBLEM_DTYPE)
    p["cur_xy"][:, 0] = x.ravel()
    p["cur_xy"][:, 1] = y.ravel()
    for q in ("cur_q", "carrot_q", "goal_q"):
        p[q][:, 3] = 1.0
    p["control_interval"] = 1.0 / 30.0
    p["delta_t"] = 1.0 / 30.0
    p["map_index"] = map_index
    return p


def at_rest(problems):
    """the controls of the probes: none"""
    return np.zeros((len(problems), 3))


def cell_requests(mx, my, resolution, origin_x, origin_y, map_index=0):
    """requests at the centres of the cells (mx[i], my[i])"""
    mx, my = np.asarray(mx), np.asarray(my)
    ux, ix = np.unique(mx, return_inverse=True)
    uy, iy = np.unique(my, return_inverse=True)
    return requests(cell_centres(origin_x, resolution, ux)[ix], cell_centres(origin_y, resolution, uy)[iy], map_index)


def window(size_x, size_y, border, margin=2):
    """(mx, my) of every cell of [-border - margin, size + border + margin) on both axes: the map, its border and beyond"""
    mx, my = np.meshgrid(np.arange(-border - margin, size_x + border + margin),
                         np.arange(-border - margin, size_y + border + margin))
    return mx.ravel(), my.ravel()


def reference(params, cmap, problems):
    """the reference objective of the probes on cmap = (cells, resolution, origin_x, origin_y)"""
    from oracle import c_oracle
    return c_oracle.objective_batch(params, cmap, problems, at_rest(problems))


def moved(problems, dx, dy, resolution):
    """the same requests `dx`, `dy` cells further"""
    p = problems.copy()
    p["cur_xy"][:, 0] += dx * resolution
    p["cur_xy"][:, 1] += dy * resolution
    return p


def gap(f0, f1):
    """relative difference of two objective values (0 where both are 0)"""
    scale = np.maximum(np.abs(f0), np.abs(f1))
    return np.abs(f1 - f0) / np.where(scale > 0.0, scale, 1.0)


def neighbour_gap(params, cmap, problems, dx, dy):
    """by how much, relative, the reference objective of every probe changes when the probe moves (dx, dy) cells"""
    return gap(reference(params, cmap, problems), reference(params, cmap, moved(problems, dx, dy, cmap[1])))


# ------------------------------------------------------------------ K3's load paths
def ingest_paths(size_x):
    """Which branches of costmap_ingest.h ingest_chunk the in-map rows of a map `size_x` cells wide reach, restated from its
    conditions: a set of "8-byte", "dwords", ("straddle", valid dwords) and "bytes".  Chunks start at multiples of 16 (both
    borders are multiples of 16); the chunks of the border alone keep the fill value and are no path of their own."""
    paths = set()
    for mx0 in range(0, size_x, 16):
        if mx0 + 16 <= size_x and size_x % 8 == 0:
            paths.add("8-byte")
        elif mx0 + 16 <= size_x and size_x % 4 == 0:
            paths.add("dwords")
        elif size_x % 4 == 0:
            paths.add(("straddle", (size_x - mx0) >> 2))
        else:
            paths.add("bytes")
    return paths


def pitch(size_x, border):
    """row pitch of the padded device map (neo_mpc_capi.cpp PaddedMap)"""
    return (size_x + 2 * border + 127) & ~127


# ------------------------------------------------------------------ cell boundaries
#: cells of the kernel's switch (costmap.h cell_of redoes the division within 1e-6 cells of an integer) and steps either side
BOUNDARY_OFFSETS = (1e-7, -1e-7, 2e-6, -2e-6)
BOUNDARY_ULPS = (1, -1, 2, -2)
FAR = (1e10, -1e10, 1e15, -1e15)


def boundary_positions(origin, resolution, k):
    """positions around the lower edge of cell k: origin + k * resolution exactly, 1 and 2 float64 steps either side, and
    1e-7 and 2e-6 cells either side"""
    e = origin + k * resolution
    out = [e]
    for n in BOUNDARY_ULPS:
        w = e
        for _ in range(abs(n)):
            w = np.nextafter(w, np.inf if n > 0 else -np.inf)
        out.append(w)
    out += [origin + (k + d) * resolution for d in BOUNDARY_OFFSETS]
    return np.array(out)


# ------------------------------------------------------------------ robots of the reach-tile test
def edge_robot_cells(size_x, size_y, reach, step=2):
    """The robots' cells (mx, my), unique: a grid over the whole map; rings 1, reach // 2 and reach + 2 cells outside it; and
    the cells exactly reach - 1, reach and reach + 1 cells from each edge -- where the tile's first or last row or column is the
    last outside the map, the first inside, and the one after."""
    gx, gy = list(range(0, size_x, step)), list(range(0, size_y, step))
    ex = sorted({reach - 1, reach, reach + 1, size_x - reach - 2, size_x - reach - 1, size_x - reach})
    ey = sorted({reach - 1, reach, reach + 1, size_y - reach - 2, size_y - reach - 1, size_y - reach})
    cells = {(x, y) for x in gx for y in gy}
    cells |= {(x, y) for x in ex for y in gy + ey} | {(x, y) for x in gx for y in ey}
    for d in (1, max(2, reach // 2), reach + 2):
        xs = sorted(set(range(-d, size_x + d, 3)) | {size_x + d - 1})
        ys = sorted(set(range(-d, size_y + d, 3)) | {size_y + d - 1})
        cells |= {(x, y) for x in xs for y in (-d, size_y + d - 1)} | {(x, y) for x in (-d, size_x + d - 1) for y in ys}
    cells = np.array(sorted(cells))
    return cells[:, 0], cells[:, 1]


def robot_requests(mx, my, resolution, origin_x, origin_y, seed, map_index=0):
    """Requests as synthetic.make_problems draws them (yaw, carrot, goal, velocity), the robots somewhere inside the cells
    (mx[i], my[i]) -- checked in float64 like the probes."""
    rng = np.random.default_rng(seed)
    p = synthetic.make_problems(len(mx), 100, seed=seed, resolution=resolution)
    for axis, (m, origin) in enumerate(((mx, origin_x), (my, origin_y))):
        w = origin + (np.asarray(m) + rng.uniform(0.05, 0.95, size=len(m))) * resolution
        assert (cell_of(w, origin, resolution) == m).all()
        p["cur_xy"][:, axis] = w
    p["map_index"] = map_index
    return p
