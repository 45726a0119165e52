"""Transcription of step 3b of the world-scan-layer contract of include/neo_mpc.h (neo_mpc_set_world_scan_denoise): the speckle
filter between the layer and its composition.  Integers only.

The group-size decision is written three times.  `small_by_flood_fill` goes by the definition -- a group is a connected
component of occupied cells -- with a stack, and counts the branches it takes in `stats`; `small_by_label` lets
scipy.ndimage.label find the components; `small_by_bounded_ball` is the form the device uses: the occupied cells within G - 1
neighbour steps of a cell number at least G exactly when its group does, and they lie within G - 1 cells of it, so the cell is
judged from the (2 G - 1)^2 window around it alone.  tests/test_world_scan_denoise.py holds the three to each other.

`DenoisedWorldScanLayer` puts the step into the handle's part: tests/world_scan_layer_reference.py's WorldScanLayer for the
layer, then D, then `live` composed from D by the scan layer's own `combine_into` and `inflate_from`.  Helper module: no tests
in here."""
import numpy as np

from tests import scan_layer_reference as scan_ref
from tests import world_scan_layer_reference as world_ref
from tests.fleet_stamp_reference import inflation_costs

FREE, LETHAL = scan_ref.FREE, scan_ref.LETHAL
MAX_GROUP = 16


def neighbours(connectivity):
    """The (di, dl) of a cell's neighbours."""
    assert connectivity in (4, 8), connectivity
    return [(di, dl) for dl in (-1, 0, 1) for di in (-1, 0, 1)
            if (di, dl) != (0, 0) and (connectivity == 8 or abs(di) + abs(dl) == 1)]


def occupied(layer, world):
    return (np.asarray(layer) == LETHAL) | (np.asarray(world) == LETHAL)


def group_sizes_by_flood_fill(occ, connectivity, stats=None):
    """int array like `occ`: the number of cells of every occupied cell's group, 0 elsewhere."""
    sy, sx = occ.shape
    sizes = np.zeros(occ.shape, dtype=np.int64)
    seen = np.zeros(occ.shape, dtype=bool)
    steps = neighbours(connectivity)
    for l0 in range(sy):
        for i0 in range(sx):
            if not occ[l0, i0] or seen[l0, i0]:
                continue
            seen[l0, i0] = True
            group, stack = [], [(i0, l0)]
            while stack:
                i, l = stack.pop()
                group.append((i, l))
                for di, dl in steps:
                    a, b = i + di, l + dl
                    if not (0 <= a < sx and 0 <= b < sy):
                        if stats is not None:
                            stats["denoise: a neighbour outside the world"] += 1
                    elif not occ[b, a]:
                        if stats is not None:
                            stats["denoise: a neighbour that is not occupied"] += 1
                    elif seen[b, a]:
                        if stats is not None:
                            stats["denoise: a neighbour already in the group"] += 1
                    else:
                        if stats is not None:
                            stats["denoise: a neighbour joins the group"] += 1
                        seen[b, a] = True
                        stack.append((a, b))
            if stats is not None:
                stats["denoise: a group of one" if len(group) == 1 else "denoise: a group of several"] += 1
            for i, l in group:
                sizes[l, i] = len(group)
    return sizes


def group_sizes_by_label(occ, connectivity):
    from scipy import ndimage
    structure = np.ones((3, 3), dtype=int) if connectivity == 8 else np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    labels, n = ndimage.label(occ, structure=structure)
    counts = np.bincount(labels.ravel(), minlength=n + 1)
    counts[0] = 0
    return counts[labels].astype(np.int64)


def ball_count(occ, i, l, group, connectivity):
    """|B_{G-1}| of the occupied cell (i, l), stopping where the device stops: the occupied cells within G - 1 neighbour
    steps, through occupied cells, counted inside the (2 G - 1)^2 window and nowhere else."""
    sy, sx = occ.shape
    h = group - 1
    steps = neighbours(connectivity)
    ball = {(i, l)}
    for _ in range(h):
        grown = set(ball)
        for a, b in ball:
            for di, dl in steps:
                c, d = a + di, b + dl
                if 0 <= c < sx and 0 <= d < sy and abs(c - i) <= h and abs(d - l) <= h and occ[d, c]:
                    grown.add((c, d))
        if len(grown) >= group or len(grown) == len(ball):
            ball = grown
            break
        ball = grown
    return len(ball)


def small_by_flood_fill(occ, group, connectivity, stats=None):
    """bool array: the occupied cells whose group has fewer than `group` cells."""
    return occ & (group_sizes_by_flood_fill(occ, connectivity, stats) < group)


def small_by_label(occ, group, connectivity):
    return occ & (group_sizes_by_label(occ, connectivity) < group)


def small_by_bounded_ball(occ, group, connectivity):
    out = np.zeros(occ.shape, dtype=bool)
    for l, i in np.argwhere(occ):
        out[l, i] = ball_count(occ, int(i), int(l), group, connectivity) < group
    return out


def denoise(layer, world, group, connectivity, small=small_by_label):
    """D of the contract: the layer, with 0 where a mark over a world cell that is not 254 belongs to a group of fewer than
    `group` cells.  group 0 or 1: the layer."""
    assert 0 <= group <= MAX_GROUP and connectivity in (4, 8)
    layer, world = np.asarray(layer, dtype=np.uint8), np.asarray(world, dtype=np.uint8)
    out = layer.copy()
    if group >= 2:
        out[small(occupied(layer, world), group, connectivity) & (layer == LETHAL) & (world != LETHAL)] = FREE
    return out


class DenoisedWorldScanLayer(world_ref.WorldScanLayer):
    """The handle's part with the filter's setting: `layer`, `denoised` (D) and `live` after every update."""

    def __init__(self, group=0, connectivity=8):
        super().__init__()
        self.denoised = None
        self.set_denoise(group, connectivity)

    def set_denoise(self, group, connectivity=8):
        assert 0 <= group <= MAX_GROUP and connectivity in (4, 8)
        self.group, self.connectivity = (group if group >= 2 else 0), connectivity

    def update(self, world, wres, wox, woy, inscribed_radius, inflation_radius, cost_scaling_factor, **kw):
        live = super().update(world, wres, wox, woy, inscribed_radius, inflation_radius, cost_scaling_factor, **kw)
        self.denoised = denoise(self.layer, world, self.group, self.connectivity)
        if self.group >= 2:
            table, reach = inflation_costs(wres, inscribed_radius, inflation_radius, cost_scaling_factor)
            live = scan_ref.inflate_from(scan_ref.combine_into(np.asarray(world, dtype=np.uint8), self.denoised), self.denoised,
                                         table, reach)
            self.live = live
        return live
