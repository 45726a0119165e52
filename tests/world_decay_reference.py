"""Transcription of step 2b of the world-scan-layer contract of include/neo_mpc.h (neo_mpc_set_world_scan_decay): old marks of
the fleet's shared obstacle layer expire, their age counted in scan updates.  Integers only, every difference modulo 2^32.

The rule is written twice.  `step_by_definition` goes cell by cell with Python integers reduced modulo 2^32 where the text
subtracts, and counts the branches it takes in `stats`; `step` works on whole uint32 arrays.
tests/test_world_scan_decay.py holds the second to the first.

`DecayingWorldScanLayer` puts the step into the handle's part, between the marks and the footprint clearing of
tests/world_scan_layer_reference.py's update, with tests/world_denoise_reference.py's filter and composition behind it: after
every update `layer`, `ages()`, `denoised` (D) and `live`.  Helper module: no tests in here."""
import numpy as np

from tests import scan_layer_reference as scan_ref
from tests import world_denoise_reference as denoise_ref
from tests import world_scan_layer_reference as world_ref

FREE, LETHAL = scan_ref.FREE, scan_ref.LETHAL
CLEAR, MARK = scan_ref.CLEAR, scan_ref.MARK
NO_AGE = 0xFFFFFFFF
WRAP = 1 << 32


def step_by_definition(layer, stamp, clock, marked, max_age, unknown, scan, stats=None):
    """One update's part of the rule, in place, cell by cell: `layer` uint8 as the marks of this update left it, `stamp` the
    stamps, `clock` the clock before the update, `marked` the cells this update's marks wrote, `scan` whether it is a scan
    update -> the clock after it."""
    assert max_age > 0
    sy, sx = layer.shape
    if scan:
        clock = (clock + 1) % WRAP
        if stats is not None:
            stats["decay: a scan update advances the clock"] += 1
            if clock == 0:
                stats["decay: the clock wraps"] += 1
    elif stats is not None:
        stats["decay: an update that is no scan update"] += 1
    for l in range(sy):
        for i in range(sx):
            if scan and marked[l, i]:
                stamp[l, i] = clock
                if stats is not None:
                    stats["decay: a mark is stamped"] += 1
            if layer[l, i] != LETHAL:
                continue                                # (its stamp is not read)
            age = (clock - int(stamp[l, i])) % WRAP
            if age >= max_age:
                layer[l, i] = unknown
                if stats is not None:
                    stats["decay: a mark expires"] += 1
            elif stats is not None:
                stats["decay: a mark is young enough"] += 1
                if clock < int(stamp[l, i]):
                    stats["decay: an age across the wrap"] += 1
    return clock


def step(layer, stamp, clock, marked, max_age, unknown, scan):
    """The same on arrays, in place -> the clock after the update."""
    assert max_age > 0 and stamp.dtype == np.uint32
    clock = np.uint32(clock)
    with np.errstate(over="ignore"):
        if scan:
            clock = clock + np.uint32(1)
            stamp[marked] = clock
        old = (layer == LETHAL) & ((clock - stamp) >= np.uint32(max_age))
    layer[old] = unknown
    return int(clock)


def ages(layer, stamp, clock):
    """What neo_mpc_get_world_scan_ages returns: clock - stamp under a mark, NO_AGE elsewhere."""
    with np.errstate(over="ignore"):
        got = np.uint32(clock) - stamp
    return np.where(layer == LETHAL, got, np.uint32(NO_AGE)).astype(np.uint32)


class DecayingWorldScanLayer(denoise_ref.DenoisedWorldScanLayer):
    """The handle's part with both settings.  An update is the update of the classes below in two halves -- the rays and the
    marks, then, behind this step, the footprint clearing, the filter and the composition -- so nothing of them is copied."""

    def __init__(self, max_age=0, group=0, connectivity=8, clock=0, by_definition=False):
        super().__init__(group, connectivity)
        self.max_age, self.clock, self.stamp, self.decaying = int(max_age), int(clock) % WRAP, None, False
        self.by_definition = by_definition

    def set_decay(self, max_age):
        assert 0 <= max_age < WRAP
        self.max_age = int(max_age)

    def ages(self):
        assert self.decaying, "the last update ran without decay"
        return ages(self.layer, self.stamp, self.clock)

    def update(self, world, wres, wox, woy, inscribed_radius, inflation_radius, cost_scaling_factor, points=None, flags=None,
               clear=None, **kw):
        if self.max_age == 0:
            self.decaying = False
            return super().update(world, wres, wox, woy, inscribed_radius, inflation_radius, cost_scaling_factor, points=points,
                                  flags=flags, clear=clear, **kw)
        if flags is None:
            flags = (CLEAR | MARK) if points is not None else 0
        unknown = kw.get("unknown_value", 255)
        rays = {k: v for k, v in kw.items() if k in ("sensor_origins", "point_counts")}
        # steps 1 and 2 (the composition of this half is thrown away)
        super().update(world, wres, wox, woy, 0.0, 0.0, 1.0, points=points, flags=flags, clear=None, **kw)
        layer = self.layer.copy()
        scan = bool(flags & MARK) and points is not None and len(points) > 0
        marked = np.zeros(layer.shape, dtype=bool)
        if scan:
            # where this update's marks fell: the marks alone, on a layer of their own
            alone = world_ref.WorldScanLayer()
            alone.update(np.zeros_like(world), wres, wox, woy, 0.0, 0.0, 1.0, points=points, flags=MARK, clear=None,
                         **{k: v for k, v in kw.items() if k not in ("by_definition", "stats")})
            marked = alone.layer == LETHAL
        # step 2b.  The first update with decay on: the marks that are there count as made by the last scan update before it
        if not self.decaying or self.stamp is None or self.stamp.shape != layer.shape:
            self.stamp = np.full(layer.shape, self.clock, dtype=np.uint32)
        form = step_by_definition if self.by_definition else step
        self.clock = form(layer, self.stamp, self.clock, marked, self.max_age, unknown, scan)
        self.layer = layer
        self.decaying = True
        # steps 3, 3b and 4 on the layer as decay left it
        kw = {k: v for k, v in kw.items() if k not in rays}
        return super().update(world, wres, wox, woy, inscribed_radius, inflation_radius, cost_scaling_factor, points=None, flags=0,
                              clear=clear, **kw)
