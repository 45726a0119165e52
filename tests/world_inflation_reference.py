"""Transcription of the world-inflation contract of include/neo_mpc.h (neo_mpc_inflate_world_map): nav2's inflation layer
applied to the master grid a fleet's rolling windows are cut from.

Written from the contract's text.  The seeds are the cells equal to 254; N is the smallest squared cell distance to a seed,
an integer; the cost table and the combination rule are the fleet stamp's and are imported from
tests/fleet_stamp_reference.py, not copied.  Nothing but the table is floating point, so the library is held to this by
exact equality of uint8 cells.  Two forms: `inflate_by_definition` takes, for every cell, the minimum over every seed, as
the text does (small maps only); `inflate` takes the distance to the nearest seed of each row first and then the minimum
over dy of dy^2 + that distance squared, rows further than R away left out -- the same integers wherever N <= R^2, which is
all the combination looks at; tests/test_world_inflation.py holds the second to the first.  Helper module: no tests in here."""
import numpy as np

from tests.fleet_stamp_reference import FAR, combine, inflation_costs

SEED = 254


def table_for(resolution, inscribed_radius, inflation_radius, cost_scaling_factor):
    """(T, R) at the WORLD map's resolution."""
    return inflation_costs(resolution, inscribed_radius, inflation_radius, cost_scaling_factor)


def inflate_by_definition(cells, table, reach):
    """The contract, literally: for every cell the minimum over every seed."""
    cells = np.asarray(cells, dtype=np.uint8)
    size_y, size_x = cells.shape
    dist2 = np.full((size_y, size_x), FAR, dtype=np.int64)
    i, l = np.arange(size_x)[None, :], np.arange(size_y)[:, None]
    for sl, si in zip(*np.nonzero(cells == SEED)):
        dist2 = np.minimum(dist2, (i - si) ** 2 + (l - sl) ** 2)
    return combine(cells, dist2, table, reach)


def squared_distances(cells, reach):
    """N per cell, exact wherever N <= reach^2 and FAR or larger than reach^2 elsewhere."""
    cells = np.asarray(cells, dtype=np.uint8)
    size_y, size_x = cells.shape
    seeds = cells == SEED
    dist2 = np.full((size_y, size_x), FAR, dtype=np.int64)
    if not seeds.any():
        return dist2
    col = np.arange(size_x)[None, :]
    left = np.maximum.accumulate(np.where(seeds, col, -FAR), axis=1)                       # nearest seed at or left of
    right = np.minimum.accumulate(np.where(seeds, col, FAR)[:, ::-1], axis=1)[:, ::-1]     # ... at or right of
    along = np.minimum(col - left, right - col).astype(np.int64)
    along2 = np.where(along >= FAR // 2, FAR, along * along)
    for dy in range(-reach, reach + 1):
        lo, hi = max(0, -dy), min(size_y, size_y - dy)          # rows l with 0 <= l + dy < size_y
        if lo >= hi:
            continue
        rows = along2[lo + dy:hi + dy]
        dist2[lo:hi] = np.minimum(dist2[lo:hi], np.where(rows >= FAR, FAR, rows + dy * dy))
    return dist2


def inflate(cells, table, reach):
    """The same map, faster: row-wise nearest seed, then the minimum over dy."""
    cells = np.asarray(cells, dtype=np.uint8)
    return combine(cells, squared_distances(cells, reach), table, reach)


def inflate_world(cells, resolution, inscribed_radius, inflation_radius, cost_scaling_factor):
    """What neo_mpc_inflate_world_map leaves of a world map `cells` [WSY, WSX] at `resolution`."""
    table, reach = table_for(resolution, inscribed_radius, inflation_radius, cost_scaling_factor)
    return inflate(cells, table, reach)
