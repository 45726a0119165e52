"""The wall model of the stage-wise direction (csrc/costmap.h edge_stickiness) reads up to three cells of the reach tile and
their term-table words.  Its serial form reads the stage's own cell, decides from the position inside the cell whether an
axis has an edge in its zone, and only then -- behind a lane-divergent branch -- reads that axis' neighbour.  The static-tile
kernels choose the neighbour FIRST (`lo ? m - 1 : m + 1`: the high neighbour where neither side is in the zone), read the
three cells together, and let the same branches consume the copies.  That is only allowed where both forms give the same
BITS for every position and every neighbourhood, and where the cell read for nothing lies inside the tile.

Both forms are written out here in float64 with NumPy scalars, the tail that turns the two axes' weights into the stage
record's five entries and the hop vector included, and held against each other on a 5 x 5 tile with free, graded, inscribed
(253) and lethal (254) cells: every interior cell as the stage's own, the in-cell offsets on a grid that holds exactly 0, the
zone boundaries (wall, sticky, hop range) and 1 - those, both axes at once, for a hop range above and one below the wall zone.
The tile reader refuses an index outside the tile, so a pre-read that left it would fail the test."""
import itertools

import numpy as np

D = np.float64
# csrc/solver_rules.h
STICKY, WALL, STICKY_DIST, WALL_DIST, HOP_MARGIN = D(100.0), D(1e4), D(0.02), D(0.1), D(0.01)
RES, DT, WT = D(0.05), D(0.2), D(0.5)
HOP_DROP = D(1e-4)

TILE = np.array([[0, 0, 40, 254, 254],
                 [0, 120, 253, 254, 0],
                 [60, 0, 0, 200, 254],
                 [254, 253, 90, 0, 0],
                 [254, 254, 0, 10, 253]], dtype=np.uint8)     # [y][x]


def raw_occupancy(raw):
    raw = int(raw)
    return 0 if raw == 0 else 99 if raw == 253 else 100 if raw == 254 else -1 if raw == 255 else 1 + (97 * (raw - 1)) // 251


TERM = np.array([D(0.5) * D(raw_occupancy(r)) / D(100.0) for r in range(256)], dtype=np.float64)


class Reader:
    """The tile as the kernel sees it: a read outside it is an error, every read is counted."""

    def __init__(self):
        self.reads = 0

    def __call__(self, mx, my):
        assert 0 <= mx < TILE.shape[1] and 0 <= my < TILE.shape[0], (mx, my)
        self.reads += 1
        return int(TILE[my, mx])


def _axis(lo, dist, raw_here, raw_n, here, there, hop_range, drop):
    """One axis of the wall model behind its `if (lo || hi)`: -> rho, pb, hop?, the new best drop, the hop's world component."""
    rho, pb, hop, hw = D(0.0), D(0.0), False, D(0.0)
    wall = raw_n == 254 and raw_here != 254
    if wall:
        if dist < WALL_DIST:
            rho = WALL * D(2.0) * WT
            pb = ((WALL_DIST - dist) if lo else (dist - WALL_DIST)) * RES
    elif dist < STICKY_DIST and there > here:
        rho = STICKY * D(2.0) * WT
    if dist < hop_range and here - there > drop:
        drop = here - there
        hop = True
        hw = (D(-1.0) if lo else D(1.0)) * (dist + HOP_MARGIN) * RES
    return rho, pb, hop, drop, hw


def _tail(rx, ry, pbx, pby, hop, hwx, hwy, c0, s0, cs, sn):
    wxx = rx * c0 * c0 + ry * s0 * s0
    wxy = rx * c0 * -s0 + ry * s0 * c0
    wyy = rx * s0 * s0 + ry * c0 * c0
    lx = -(rx * pbx * c0 + ry * pby * s0)
    ly = -(rx * pbx * -s0 + ry * pby * c0)
    hop_x = hop_y = np.float32(0.0)
    if hop:
        hrx, hry, idt = c0 * hwx + s0 * hwy, -s0 * hwx + c0 * hwy, D(1.0) / DT
        hop_x = np.float32((cs * hrx + sn * hry) * idt)
        hop_y = np.float32((-sn * hrx + cs * hry) * idt)
    return np.array([wxx, wxy, wyy, lx, ly]), bool(hop), np.array([hop_x, hop_y], dtype=np.float32)


def _axes(mx, my, fx, fy, hop_range, raw_here, here, neighbour_x, neighbour_y, frame):
    """What both forms share behind their reads; neighbour_x / neighbour_y: (lo) -> (raw, term) of that axis' neighbour."""
    zone = max(WALL_DIST, hop_range)
    xlo, xhi, ylo, yhi = fx < zone, D(1.0) - fx < zone, fy < zone, D(1.0) - fy < zone
    rx = ry = pbx = pby = hwx = hwy = D(0.0)
    drop, hop = HOP_DROP, False
    if xlo or xhi:
        raw_n, there = neighbour_x(xlo)
        rx, pbx, h, drop, hw = _axis(xlo, fx if xlo else D(1.0) - fx, raw_here, raw_n, here, there, hop_range, drop)
        if h:
            hop, hwx, hwy = True, hw, D(0.0)
    if ylo or yhi:
        raw_n, there = neighbour_y(ylo)
        ry, pby, h, _, hw = _axis(ylo, fy if ylo else D(1.0) - fy, raw_here, raw_n, here, there, hop_range, drop)
        if h:
            hop, hwx, hwy = True, D(0.0), hw
    return _tail(rx, ry, pbx, pby, hop, hwx, hwy, *frame)


def serial_form(read, mx, my, fx, fy, hop_range, frame):
    raw_here = read(mx, my)
    here = TERM[raw_here]

    def nx(lo):
        r = read(mx - 1 if lo else mx + 1, my)
        return r, TERM[r]

    def ny(lo):
        r = read(mx, my - 1 if lo else my + 1)
        return r, TERM[r]
    return _axes(mx, my, fx, fy, hop_range, raw_here, here, nx, ny, frame)


def choose_first_form(read, mx, my, fx, fy, hop_range, frame):
    zone = max(WALL_DIST, hop_range)
    nmx = mx - 1 if fx < zone else mx + 1          # (neither side in the zone: the high neighbour, read for nothing)
    nmy = my - 1 if fy < zone else my + 1
    raw_here, raw_nx, raw_ny = read(mx, my), read(nmx, my), read(mx, nmy)      # three bytes, one wait
    here, there_x, there_y = TERM[raw_here], TERM[raw_nx], TERM[raw_ny]        # three table words, one wait
    return _axes(mx, my, fx, fy, hop_range, raw_here, here, lambda lo: (raw_nx, there_x), lambda lo: (raw_ny, there_y), frame)


def _offsets(hop_range):
    edges = [D(0.0), STICKY_DIST, WALL_DIST, hop_range, HOP_MARGIN]
    vals = set()
    for e in edges:
        for v in (e, D(1.0) - e):
            vals.update([v, np.nextafter(v, D(0.0)), np.nextafter(v, D(1.0))])
    vals.update([D(0.5), D(0.3), D(0.77)])
    return sorted(v for v in vals if D(0.0) <= v < D(1.0))


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64 if x.dtype == np.float64 else np.uint32)


def _frames():
    for psi0, th in ((0.0, 0.0), (0.7, -0.4), (2.9, 1.3)):
        yield D(np.cos(psi0)), D(np.sin(psi0)), D(np.cos(th)), D(np.sin(th))


def test_tile_holds_every_kind_of_cell():
    kinds = set(TILE.ravel().tolist())
    assert 0 in kinds and 253 in kinds and 254 in kinds and any(0 < k < 253 for k in kinds)


def test_choose_first_equals_serial_bit_for_bit():
    cases = axes_both = hops = walls = sticky = 0
    for hop_range in (D(0.25), D(0.04)):      # (above and below the wall zone: min(0.25, 0.05 m/s dt / resolution))
        offs = _offsets(hop_range)
        zone = max(WALL_DIST, hop_range)
        for frame in _frames():
            for (mx, my), (fx, fy) in itertools.product(itertools.product(range(1, 4), repeat=2), itertools.product(offs, repeat=2)):
                ra, rb = Reader(), Reader()
                wa, ha, va = serial_form(ra, mx, my, fx, fy, hop_range, frame)
                wb, hb, vb = choose_first_form(rb, mx, my, fx, fy, hop_range, frame)
                assert np.array_equal(_bits(wa), _bits(wb)) and ha == hb and np.array_equal(_bits(va), _bits(vb)), (mx, my, fx, fy)
                assert rb.reads == 3 and ra.reads <= 3
                cases += 1
                both = (fx < zone or 1.0 - fx < zone) and (fy < zone or 1.0 - fy < zone)
                axes_both += both
                hops += ha
                walls += bool(np.abs(wa[3:]).max() > 0)
                sticky += bool(np.abs(wa[:3]).max() > 0)
    # the grid reaches every arm: both axes at once, hops, wall stand-offs, sticky edges
    assert cases > 5000 and axes_both > 1000 and hops > 100 and walls > 100 and sticky > walls
