"""Pure-Python transcription of the rolling-window contract of include/neo_mpc.h (neo_mpc_window_batch): nav2's
`LayeredCostmap::updateMap` -> `Costmap2D::updateOrigin` for the window's origin and the rolling-window branch of
`StaticLayer::updateCosts` (`mapToWorld` of the window, `worldToMap` on the static map) for its cells.

Written from the contract, cell by cell, not from the kernel: no index tables, no separability.  All arithmetic is on
Python floats -- IEEE float64, one correctly rounded operation per `+ - * /`, nothing fused -- in the order the contract
writes it, so the library is held to it by exact equality."""
import math

import numpy as np


def move_axis(x, o, size, res):
    """The new origin coordinate of a window of `size` cells whose robot stands at `x`."""
    x, o, res = float(x), float(o), float(res)
    s = (size - 1 + 0.5) * res              # getSizeInMetersX
    n = x - s / 2
    q = (n - o) / res
    c = int(q) if math.isfinite(q) and abs(q) < 2.0 ** 31 else 0     # static_cast<int>: toward zero
    return o + c * res


def move_origin(origin, xy, size_x, size_y, res):
    return move_axis(xy[0], origin[0], size_x, res), move_axis(xy[1], origin[1], size_y, res)


def world_cell(w, wo, wres, wsize):
    """worldToMap along one axis: the world map's cell index of coordinate `w`, None where it refuses."""
    if w < wo:
        return None
    q = (w - wo) / wres
    if not q < wsize:
        return None
    return int(q)


def fill_window(world, wres, wox, woy, origin, size_x, size_y, res, outside_value=255, dtype=np.uint8):
    """The cells [size_y, size_x] of a window with `origin`, sampled from `world` (uint8 [WSY, WSX])."""
    wsy, wsx = world.shape
    wres, wox, woy, res = float(wres), float(wox), float(woy), float(res)
    ox, oy = float(origin[0]), float(origin[1])
    out = np.empty((size_y, size_x), dtype=dtype)
    for j in range(size_y):
        for i in range(size_x):
            wx = ox + (i + 0.5) * res       # mapToWorld
            wy = oy + (j + 0.5) * res
            mx = world_cell(wx, wox, wres, wsx)
            my = world_cell(wy, woy, wres, wsy)
            out[j, i] = outside_value if mx is None or my is None else world[my, mx]
    return out


def roll(world, wres, wox, woy, origins, size_x, size_y, res, poses=None, outside_value=255, fill=True):
    """One roll of `len(origins)` windows.  Returns (new origins float64 [count, 2], cells uint8 [count, size_y, size_x]
    -- None with fill=False).  `poses` [count, >= 2] or None (the windows stay where they are)."""
    origins = np.array(origins, dtype=np.float64).reshape(-1, 2)
    if poses is not None:
        for k in range(len(origins)):
            origins[k] = move_origin(origins[k], poses[k], size_x, size_y, res)
    if not fill:
        return origins, None
    cells = np.stack([fill_window(world, wres, wox, woy, origins[k], size_x, size_y, res, outside_value)
                      for k in range(len(origins))])
    return origins, cells
