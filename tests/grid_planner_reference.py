"""The grid planner's contract (include/neo_mpc.h, neo_mpc_replan_batch) transcribed in plain Python -- nav2's planners are no
dependency of this repository and use float potentials, so this transcription IS the reference of K16 (k_replan).  The
potential is a heap Dijkstra from the goal over the reversed moves (the kernel relaxes to the same fixpoint: a shortest-path
cost is unique), the path the walk down that potential under the tie rule; every decision is an `if` on Python ints, the
poses are one float64 multiply and one float64 add each.  Helper module: no tests in here."""
import heapq

import numpy as np

from neo_mpc_planner2_amd import abi
from tests import footprint_gate_reference as fref

#: direction k -> (dx, dy): E, NE, N, NW, W, SW, S, SE (y grows to the north)
MOVES = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))
#: the header's table: k * pi / 4, from k = 5 on (k - 8) * pi / 4
YAW = (0.0, 0.7853981633974483, 1.5707963267948966, 2.356194490192345, 3.141592653589793,
       -2.356194490192345, -1.5707963267948966, -0.7853981633974483)


def window_origin(s, g, size, window):
    """One axis: clamp((s + g) / 2 - W / 2, 0, max(size - W, 0)), integer division."""
    return min(max((s + g) // 2 - window // 2, 0), max(size - window, 0))


class Search:
    """One robot's search window on `cells`: which cells are traversable, what a move costs, the potential."""

    def __init__(self, cells, s, g, window, max_cost, unknown_cost, neutral_cost):
        self.cells, self.s, self.g = cells, s, g
        self.size_y, self.size_x = cells.shape
        self.window, self.max_cost, self.unknown_cost, self.neutral_cost = window, max_cost, unknown_cost, neutral_cost
        self.x0 = window_origin(s[0], g[0], self.size_x, window)
        self.y0 = window_origin(s[1], g[1], self.size_y, window)

    def inside(self, c):
        return (self.x0 <= c[0] < min(self.x0 + self.window, self.size_x) and
                self.y0 <= c[1] < min(self.y0 + self.window, self.size_y))

    def traversable(self, c):
        """By the cell's value alone; everything outside the window is not."""
        if not self.inside(c):
            return False
        v = int(self.cells[c[1], c[0]])
        if v == 255:
            return self.unknown_cost > 0
        return v < self.max_cost

    def cost(self, c):
        v = int(self.cells[c[1], c[0]])
        return self.unknown_cost if v == 255 else v

    def allowed(self, a, k):
        """The move from `a` in direction k: its target traversable and, for a diagonal, both cells it passes between."""
        dx, dy = MOVES[k]
        if not self.traversable((a[0] + dx, a[1] + dy)):
            return False
        if k % 2 == 1 and not (self.traversable((a[0] + dx, a[1])) and self.traversable((a[0], a[1] + dy))):
            return False
        return True

    def step(self, a, k):
        b = (a[0] + MOVES[k][0], a[1] + MOVES[k][1])
        return (14 if k % 2 == 1 else 10) * (self.neutral_cost + self.cost(b))

    def leaves(self, a):
        """Whether moves start at `a`: a traversable cell, or the start cell whatever it holds."""
        return a == self.s or self.traversable(a)

    def potential(self):
        """{cell: G}: Dijkstra from the goal over the reversed moves."""
        G = {self.g: 0}
        heap = [(0, self.g)]
        while heap:
            d, b = heapq.heappop(heap)
            if d > G[b]:
                continue
            if not self.traversable(b):        # (the start cell where it is a wall: moves leave it, none enters it)
                continue
            for k in range(8):
                a = (b[0] - MOVES[k][0], b[1] - MOVES[k][1])
                if not self.inside(a) or not self.leaves(a) or not self.allowed(a, k):
                    continue
                cand = self.step(a, k) + d
                if cand < G.get(a, 1 << 32):
                    G[a] = cand
                    heapq.heappush(heap, (cand, a))
        return G

    def walk(self, G):
        """From the start to the allowed neighbour of least step + G, the lowest k on a tie, until the goal."""
        path, a = [self.s], self.s
        while a != self.g:
            best, nxt = None, None
            for k in range(8):
                b = (a[0] + MOVES[k][0], a[1] + MOVES[k][1])
                if b in G and self.allowed(a, k):
                    cand = self.step(a, k) + G[b]
                    if best is None or cand < best:
                        best, nxt = cand, b
            assert best == G[a] and len(path) < self.window * self.window
            a = nxt
            path.append(a)
        return path


def poses_of(path, res, ox, oy):
    """Cell centres, one rounded multiply and one rounded add each; the yaw of the move that leaves the cell, the last pose
    that of the one before it, a lone cell 0."""
    out = []
    for j, (mx, my) in enumerate(path):
        if j + 1 < len(path):
            k = MOVES.index((path[j + 1][0] - mx, path[j + 1][1] - my))
        elif j > 0:
            k = MOVES.index((mx - path[j - 1][0], my - path[j - 1][1]))
        else:
            k = 0
        out.append((ox + (mx + 0.5) * res, oy + (my + 0.5) * res, YAW[k]))
    return out


def replan_one(cells, res, ox, oy, start, goal, window, max_cost, unknown_cost, neutral_cost, max_path_cells):
    """One robot that was asked -> ((status, length, cost, window_x0, window_y0), the whole path's cells, the search or None)."""
    size_y, size_x = cells.shape
    s = fref.world_to_map(float(start[0]), float(start[1]), size_x, size_y, res, ox, oy)
    g = fref.world_to_map(float(goal[0]), float(goal[1]), size_x, size_y, res, ox, oy)
    if s is None or g is None:
        return (3, 0, 0, 0, 0), [], None
    q = Search(cells, s, g, window, max_cost, unknown_cost, neutral_cost)
    if not (q.inside(s) and q.inside(g)):
        return (3, 0, 0, q.x0, q.y0), [], q
    if s == g:                                  # the robot stands on its goal: the start cell's value is never looked at
        return (0, 1, 0, q.x0, q.y0), [s], q
    if not q.traversable(g):
        return (2, 0, 0, q.x0, q.y0), [], q
    G = q.potential()
    if s not in G:
        return (1, 0, 0, q.x0, q.y0), [], q
    path = q.walk(G)
    return (5 if len(path) > max_path_cells else 0, len(path), G[s], q.x0, q.y0), path, q


def replan_plans(cells, res, ox, oy, starts, goals, window, checks=None, max_cost=253, unknown_cost=0, neutral_cost=50,
                 max_path_cells=None, path_cells=None, path_poses=None):
    """The batch -> (records abi.REPLAN_DTYPE [count], path_cells int32 [count, max_path_cells, 2], path_poses float64
    [count, max_path_cells, 3]).  `path_cells` / `path_poses`: what the output arrays hold before the call (zeros without);
    entries beyond a path stay as they are."""
    cells = np.asarray(cells)
    starts = np.asarray(starts, dtype=np.float64).reshape(-1, 2)
    goals = np.asarray(goals, dtype=np.float64).reshape(-1, 2)
    count = len(starts)
    stride = window * window if max_path_cells is None else int(max_path_cells)
    out = np.zeros(count, dtype=abi.REPLAN_DTYPE)
    out_cells = np.zeros((count, stride, 2), dtype=np.int32) if path_cells is None else np.array(path_cells, dtype=np.int32)
    out_poses = np.zeros((count, stride, 3), dtype=np.float64) if path_poses is None else np.array(path_poses, dtype=np.float64)
    for i in range(count):
        if checks is not None and int(checks[i]["status"]) != 1:
            out[i] = (4, 0, 0, 0, 0, 0)
            continue
        r, path, _ = replan_one(cells, float(res), float(ox), float(oy), starts[i], goals[i], int(window), int(max_cost),
                                int(unknown_cost), int(neutral_cost), stride)
        out[i] = r + (0,)
        n = min(len(path), stride)
        if n:
            out_cells[i, :n] = path[:n]
            out_poses[i, :n] = poses_of(path, float(res), float(ox), float(oy))[:n]
    return out, out_cells, out_poses


def record(status, length=0, cost=0, window_x0=0, window_y0=0):
    """One expected record, written out by hand in a test."""
    return (status, length, cost, window_x0, window_y0, 0)
