"""Transcription of the laser-projection contract of include/neo_mpc.h (neo_mpc_laser_batch): LaserScan ranges of several
scanners a robot projected into global-frame hit points and sensor origins, and the scan layer's update over all of them --
every clear of every scanner, then every mark.

Written from the contract's text.  The projection is pure Python floats, beam by beam: every + - * / is one IEEE float64
operation in the order the text writes them, cos and sin are libm's (math.cos, math.sin -- the library's table is built with
the same libm).  The multi-source update is composed from tests/scan_layer_reference.py, imported unchanged: roll, then
`clear` per source, then `mark` per source, then combine and inflate.  Helper module: no tests in here."""
import math
import struct

import numpy as np

from tests import scan_layer_reference as scan_ref
from tests.fleet_stamp_reference import inflation_costs

INF_IS_VALID = 1
SCANNER_FIELDS = ("mount_x", "mount_y", "mount_yaw", "angle_min", "angle_increment", "range_min", "range_max")
NAN = float("nan")


def widen(r):
    """(double) of a float32 range as it is on the wire."""
    return struct.unpack("<f", struct.pack("<f", r))[0]


def beam_table(scanner, beams):
    """Step 4: [(cos a, sin a)] of every beam, a = mount_yaw + (angle_min + i * angle_increment)."""
    out = []
    for i in range(beams):
        a = scanner["mount_yaw"] + (scanner["angle_min"] + float(i) * scanner["angle_increment"])
        out.append((math.cos(a), math.sin(a)))
    return out


def valid_range(scanner, r):
    """Steps 1 and 2: the range the beam is projected at, or None where the beam is not valid."""
    if r == math.inf and scanner.get("flags", 0) & INF_IS_VALID:
        r = scanner["range_max"] - 1e-4
    if r >= scanner["range_min"] and r < scanner["range_max"]:       # (NaN fails both comparisons)
        return r
    return None


def to_global(pose, bx, by, sincos=None):
    """Steps 6 and 7.  `sincos`: (S, C) of the pose's yaw, libm's by default."""
    x, y, yaw = pose
    S, C = (math.sin(yaw), math.cos(yaw)) if sincos is None else sincos
    return (x + bx * C) - by * S, (y + bx * S) + by * C


def project(ranges, poses, scanners):
    """ranges [count][sources][beams], poses [count][3], scanners: a list of dicts -> (points float64 [count, sources, beams, 2]
    with (NaN, NaN) for a beam that is not valid, origins float64 [count, sources, 2], base-frame points in the same shape as
    points -- what the tolerance of a comparison is made of)."""
    count, sources, beams = len(ranges), len(scanners), len(ranges[0][0])
    points = np.full((count, sources, beams, 2), NAN)
    base = np.full((count, sources, beams, 2), NAN)
    origins = np.zeros((count, sources, 2))
    tables = [beam_table(sc, beams) for sc in scanners]
    for k in range(count):
        pose = tuple(float(v) for v in poses[k])
        for s, sc in enumerate(scanners):
            origins[k, s] = to_global(pose, sc["mount_x"], sc["mount_y"])
            for i in range(beams):
                r = valid_range(sc, widen(float(ranges[k][s][i])))
                if r is None:
                    continue
                c, sn = tables[s][i]
                bx, by = sc["mount_x"] + r * c, sc["mount_y"] + r * sn
                base[k, s, i] = (bx, by)
                points[k, s, i] = to_global(pose, bx, by)
    return points, origins, base


class LaserScanLayers(scan_ref.ScanLayers):
    """The handle's layers, updated from the points of several sources a robot."""

    def update_sources(self, cells, origins, res, inscribed_radius, inflation_radius, cost_scaling_factor, points,
                       sensor_origins, flags=scan_ref.CLEAR | scan_ref.MARK, obstacle_max_range=2.5, obstacle_min_range=0.0,
                       raytrace_max_range=3.0, raytrace_min_range=0.0, unknown_value=255):
        """One multi-source update on the pool `cells` [count, sy, sx]: points [count, sources, beams, 2], sensor_origins
        [count, sources, 2].  Returns the new pool; the layers are in self.layers / self.origins afterwards."""
        cells = np.asarray(cells, dtype=np.uint8)
        origins = np.asarray(origins, dtype=np.float64)
        count, sy, sx = cells.shape
        sources = points.shape[1]
        table, reach = inflation_costs(res, inscribed_radius, inflation_radius, cost_scaling_factor)
        key = (sx, sy, float(res), count, int(unknown_value))
        if key != self.key:
            self.layers = np.full((count, sy, sx), unknown_value, dtype=np.uint8)
            self.origins = origins.copy()
        self.key = key
        out = np.empty_like(cells)
        layers = np.empty_like(self.layers)
        for k in range(count):
            layer = scan_ref.roll_layer(self.layers[k], self.origins[k], origins[k], res, unknown_value)
            if flags & scan_ref.CLEAR:
                for s in range(sources):
                    scan_ref.clear(layer, origins[k], res, points[k, s], sensor_origins[k, s], raytrace_max_range, raytrace_min_range)
            if flags & scan_ref.MARK:
                for s in range(sources):
                    scan_ref.mark(layer, origins[k], res, points[k, s], sensor_origins[k, s], obstacle_max_range, obstacle_min_range)
            layers[k] = layer
            out[k] = scan_ref.inflate_from(scan_ref.combine_into(cells[k], layer), layer, table, reach)
        self.layers, self.origins = layers, origins.copy()
        return out
