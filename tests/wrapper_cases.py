"""Named, deterministic edge cases for the wrapper kernel K2 (py:365-403): tests/test_wrapper_edges.py.

Every case is a small batch at one parameter set: a 40 x 40 map at 0.05 m that is free except where the case puts cells (or a
pool of three such maps), the records, their states and warm starts, and one or more CALLS (solutions + success flags) made
on the same state records in a row.  Stages are put on CELL CENTRES: the controls are computed backwards from the cells the
rollout is to visit, so that every filtered position is 0.025 m from the nearest cell edge and a last-bit difference in a
sine cannot move a stage into another cell (`check` asserts 1e-9 m with the reference alone).
"""
import math

import numpy as np

from neo_mpc_planner2_amd import abi, synthetic
from oracle import mpc_oracle as orc
from tests import wrapper_reference as ref

SIZE, RES = 40, 0.05
ORIGIN = (-1.0, -1.0)
MARGIN = 1e-9          # a thousand times the 1e-12 m K2's path is granted (test_predicted_path_matches_reference_local_plan)
MAX_RECORDS = 256


class Call:
    """One postprocess call: the injected solutions and success flags (None: all succeeded), per-record overrides of
    request fields for this call ({field: array})."""

    def __init__(self, solutions, success=None, **fields):
        self.solutions = np.ascontiguousarray(solutions, dtype=np.float64)
        self.success = None if success is None else np.ascontiguousarray(success, dtype=np.int32)
        self.fields = fields


class Case:
    def __init__(self, name, params, maps, problems, states, warm, calls, want_path=True, pooled=False, expect=(), names=None):
        self.name, self.params, self.pooled, self.want_path = name, params, pooled, want_path
        self.maps = maps                        # list of (cells, resolution, origin_x, origin_y)
        self.problems, self.states, self.warm, self.calls = problems, states, warm, calls
        self.expect = tuple(expect)             # branches at least one record has to take (check)
        self.names = names or ["%d" % i for i in range(len(problems))]
        assert len(problems) == len(states) == len(warm) == len(self.names) <= MAX_RECORDS
        assert pooled or len(maps) == 1

    def __repr__(self):
        return self.name

    @property
    def n(self):
        return int(self.params["control_steps"])

    def map_of(self, problems):
        """Which map a record looks at: its map_index clamped into the pool (costmap pool contract), map 0 without a pool."""
        if not self.pooled:
            return np.zeros(len(problems), dtype=int)
        return np.clip(problems["map_index"], 0, len(self.maps) - 1).astype(int)

    def oracle_maps(self):
        return [orc.Costmap(*m) for m in self.maps]

    def problems_of(self, call):
        p = self.problems.copy()
        for k, v in call.fields.items():
            p[k] = v
        return p

    def reference_run(self):
        """The calls made in a row on the reference: [(problems, expected of wrapper_reference.step_batch)]."""
        st, wm = self.states.copy(), self.warm.copy()
        out = []
        for call in self.calls:
            p = self.problems_of(call)
            e = ref.step_batch(self.params, self.oracle_maps(), self.map_of(p), p, st, wm, call.solutions, call.success)
            st, wm = e["states"], e["warm"]
            out.append((p, e))
        return out


# ---------------------------------------------------------------------------------------------------------- pieces
def free_map(origin=ORIGIN):
    return [np.zeros((SIZE, SIZE), dtype=np.uint8), RES, origin[0], origin[1]]


def centre(mx, my, origin=ORIGIN):
    return (origin[0] + (mx + 0.5) * RES, origin[1] + (my + 0.5) * RES)


def params_for(n, **over):
    return orc.make_params(**dict(dict(control_steps=n, prediction_horizon=0.8, low_pass_gain=0.5), **over))


def controls_through(start, yaw0, cells, wz, dt, origin=ORIGIN):
    """The controls whose global-frame rollout (py:320-327) from `start` (a cell) and `yaw0` visits the centres of `cells`;
    stage k turns with wz[k]."""
    x = np.zeros(3 * len(cells))
    (px, py), yaw = centre(*start, origin=origin), yaw0
    for k, cell in enumerate(cells):
        tx, ty = (cell if isinstance(cell[0], float) else centre(*cell, origin=origin))
        yaw += wz[k] * dt
        dx, dy, c, s = tx - px, ty - py, math.cos(yaw), math.sin(yaw)
        x[3 * k:3 * k + 3] = ((dx * c + dy * s) / dt, (-dx * s + dy * c) / dt, wz[k])
        px, py = tx, ty
    return x


def turns(n):
    return [0.4 * (-1) ** k + 0.1 for k in range(n)]


def make_problem(start, yaw, origin=ORIGIN, **fields):
    p = np.zeros(1, dtype=abi.PROBLEM_DTYPE)
    p["cur_xy"] = centre(*start, origin=origin)
    p["cur_q"] = synthetic.yaw_quat(yaw)
    p["carrot_xy"], p["carrot_q"] = (0.4, 0.1), synthetic.yaw_quat(0.2)
    p["goal_xyz"], p["goal_q"] = (0.5, -0.25, 0.0), synthetic.yaw_quat(-0.6)
    p["control_interval"] = p["delta_t"] = 1.0 / 30.0
    for k, v in fields.items():
        p[k] = v
    return p


def make_state(problem, last=(0.0, 0.0, 0.0), wait=0.0, collision=0, fp=0, has_goal=1, old_goal=None):
    s = np.zeros(1, dtype=abi.STATE_DTYPE)
    s["last_control"], s["waiting_time"], s["collision"], s["collision_footprint"] = last, wait, collision, fp
    s["has_old_goal"] = has_goal
    s["old_goal"] = np.concatenate([problem["goal_xyz"][0], problem["goal_q"][0]]) if old_goal is None else old_goal
    # (what the previous tick left behind: the kernel has to overwrite it)
    s["has_prev_u0"], s["prev_u0"] = 1, (0.125, -0.25, 0.5)
    return s


class _Batch:
    """Records collected one by one."""

    def __init__(self, n):
        self.n, self.names, self.p, self.s, self.w, self.x, self.ok = n, [], [], [], [], [], []

    def add(self, name, problem, state, x, ok=1, warm=None):
        self.names.append(name)
        self.p.append(problem)
        self.s.append(state)
        self.w.append(np.full(3 * self.n, 0.0625) if warm is None else np.asarray(warm, dtype=np.float64))
        self.x.append(np.asarray(x, dtype=np.float64))
        self.ok.append(int(ok))

    def case(self, name, params, maps, success="all", **kw):
        calls = kw.pop("calls", None)
        if calls is None:
            calls = [Call(np.array(self.x), None if success == "all" else np.array(self.ok))]
        return Case(name, params, maps, np.concatenate(self.p), np.concatenate(self.s), np.array(self.w), calls, names=self.names, **kw)


# ---------------------------------------------------------------------------------------------------------- one stage hits
STAGE_COUNTS = (1, 2, 3, 8, 32, 63, 64)
_TRACK_ROW, _START, _LETHAL_START = 2, (2, 2), (3, 2)


def _track(n):
    """Stage k's cell on the shared track: 32 cells of one row, then 32 of the next."""
    return [(4 + k % 32, _TRACK_ROW + k // 32) for k in range(n)]


def one_stage_hits(n):
    """rollout_global spreads the stages over lanes and masks with lane < n: stage i ALONE on a lethal cell, for the first, the
    last and a middle stage and the raw values either side of the latch's threshold; nothing but the robot's own cell
    lethal; nothing but the cell one step BEHIND the last stage lethal (a rollout one stage too long would hit it)."""
    params, dt, yaw0 = params_for(n), 0.8 / n, 0.7
    m = free_map()
    b = _Batch(n)
    row = 6
    for stage in sorted({0, n - 1, n // 2}):
        for raw in (254, 252, 253, 255):
            cells = _track(n)
            cells[stage] = (cells[stage][0], row)            # the detour: a row no other record visits
            m[0][row, cells[stage][0]] = raw
            x = controls_through(_START, yaw0, cells, turns(n), dt)
            p = make_problem(_START, yaw0)
            b.add("stage %d raw %d" % (stage, raw), p, make_state(p, last=x[:3]), x)
            row += 1
    m[0][_LETHAL_START[1], _LETHAL_START[0]] = 254
    x = controls_through(_LETHAL_START, yaw0, _track(n), turns(n), dt)
    p = make_problem(_LETHAL_START, yaw0)
    b.add("start cell lethal", p, make_state(p, last=x[:3]), x)
    t = [_START] + _track(n)
    beyond = (2 * t[-1][0] - t[-2][0], 2 * t[-1][1] - t[-2][1])
    assert beyond not in t and m[0][beyond[1], beyond[0]] == 0
    m[0][beyond[1], beyond[0]] = 254
    x = controls_through(_START, yaw0, _track(n), turns(n)[:-1] + [0.0], dt)   # (straight on behind the last stage: no turn in it)
    p = make_problem(_START, yaw0)
    b.add("lethal behind the last stage", p, make_state(p, last=x[:3]), x)
    return b.case("one stage hits, n=%d" % n, params, [tuple(m)], expect=("hit at stage 0", "hit at the last stage", "moves"))


# ---------------------------------------------------------------------------------------------------------- map edges
BORDER_STEPS = (1, 16, 17, 64, 65)    # cells outside the map: next to it, around the paddings the device keeps (16 a pool, 64 one map)


def _edge_records(b, n, dt, origin=ORIGIN, **fields):
    yaw0, start = -2.1, (20, 20)
    for stage in (0, n - 1):
        for axis in (0, 1):
            outside = [-k for k in BORDER_STEPS] + [SIZE - 1 + k for k in BORDER_STEPS]
            for c in outside + [0, SIZE - 1]:
                cells = [(20, 20 + (k % 2)) for k in range(n)]
                cells[stage] = (c, 21) if axis == 0 else (21, c)
                x = controls_through(start, yaw0, cells, turns(n), dt, origin=origin)
                p = make_problem(start, yaw0, origin=origin, **fields)
                b.add("stage %d in cell %s %d" % (stage, "xy"[axis], c), p, make_state(p, last=x[:3]), x)


def map_edges():
    n = 3
    b = _Batch(n)
    _edge_records(b, n, 0.8 / n)
    return b.case("map edges", params_for(n), [tuple(free_map())], expect=("hit at stage 0", "hit at the last stage", "moves"))


def far_stage():
    """A stage 1e7 m away (in x, in y, either sign): outside every map.  The far stage is the second of three, so the first
    block -- the only one the low-pass touches -- stays small; no path is asked for (a coordinate of 1e7 m has an ulp of
    1.9e-9 m: the path's 1e-12 m says nothing there)."""
    n, dt, yaw0, start = 3, 0.8 / 3, 0.9, (20, 20)
    b = _Batch(n)
    for axis in (0, 1):
        for far in (1e7, -1e7):
            c = list(centre(20, 20))
            c[axis] = centre(int(far / RES), int(far / RES))[axis]
            x = controls_through(start, yaw0, [(21, 20), tuple(c), tuple(c)], turns(n), dt)
            p = make_problem(start, yaw0)
            b.add("%s = %g m" % ("xy"[axis], far), p, make_state(p, last=x[:3]), x)
    return b.case("far stage", params_for(n), [tuple(free_map())], want_path=False, expect=("hit in the middle",))


# ---------------------------------------------------------------------------------------------------------- low-pass decides
def low_pass_decides(n, gain):
    """last_control far from the solution's first block.  Stage 0 of the UNFILTERED rollout stands on cell A, of the FILTERED
    one on cell B (the turn rates are equal, so the later stages are the same moves from there); A lethal in one record, B in
    the other.  At gain 1 the two rollouts are one; at gain 0 the first block is last_control alone."""
    params, dt, yaw0, start = params_for(n, low_pass_gain=gain), 0.8 / n, 1.9, (10, 10)
    m = free_map()
    b = _Batch(n)
    for k, (name, lethal_is_filtered) in enumerate((("unfiltered crosses", False), ("filtered crosses", True))):
        row = 10 + 8 * k
        a_cell, b_cell = (16, row), (10, row + 3)
        tail = [(1, 0), (1, 1)][:n - 1]
        xa = controls_through((10, row), yaw0, [a_cell] + [(a_cell[0] + i + dx, a_cell[1] + dy) for i, (dx, dy) in enumerate(tail)], turns(n), dt)
        xb = controls_through((10, row), yaw0, [b_cell] + [(b_cell[0] + i + dx, b_cell[1] + dy) for i, (dx, dy) in enumerate(tail)], turns(n), dt)
        x = xa.copy()                                       # the solution: through A
        if gain == 1.0:
            last = (3.0, -2.0, 1.5)                         # (ignored: the filtered block is the solution's)
            lethal = a_cell if lethal_is_filtered else None
        else:
            # filtered = gain * x + (1 - gain) * last = xb's first block  (same turn rate: last[2] = x[2])
            last = tuple((xb[i] - gain * x[i]) / (1.0 - gain) for i in range(3))
            lethal = b_cell if lethal_is_filtered else a_cell
        if lethal is not None:
            m[0][lethal[1], lethal[0]] = 254
        p = make_problem((10, row), yaw0)
        b.add(name, p, make_state(p, last=last), x)
        if gain != 1.0:      # the two rollouts disagree about the latch, by the reference's own collision_check
            cm, q = orc.Costmap(*m), ref.util.oracle_problem(p[0])
            xf = np.concatenate([xb[:3], x[3:]])
            assert orc.collision_check(x, q, params, cm) != lethal_is_filtered and orc.collision_check(xf, q, params, cm) == lethal_is_filtered
    return b.case("low-pass decides, n=%d gain=%g" % (n, gain), params, [tuple(m)], expect=("hit at stage 0", "moves"))


# ---------------------------------------------------------------------------------------------------------- wait and latch
def one_ulp_below_three():
    w = float(np.nextafter(3.0, 0.0))
    assert w == 2.9999999999999996 and w + 0.0 < 3.0
    return w


def wait_and_latch():
    n, dt, yaw0, start = 3, 0.8 / 3, 0.4, (10, 10)
    params = params_for(n)
    m = free_map()
    m[0][20, 12] = 254
    b = _Batch(n)
    free = controls_through(start, yaw0, [(11, 10), (12, 10), (12, 11)], turns(n), dt)
    hit = controls_through(start, yaw0, [(11, 10), (12, 20), (12, 11)], turns(n), dt)

    def add(name, x, wait, delta_t, collision=1, fcost=0.0):
        p = make_problem(start, yaw0, delta_t=delta_t, footprint_cost=fcost)
        b.add(name, p, make_state(p, last=x[:3], wait=wait, collision=collision), x)
    add("latched, below 3.0", free, 1.0, 0.5)
    add("latched, exactly 3.0", free, 2.5, 0.5)
    add("latched, one ulp below 3.0", free, one_ulp_below_three(), 0.0)
    add("latched, above 3.0 in one call", free, 0.2, 3.0)
    add("hit on the tick the wait reaches 3.0", hit, 2.5, 0.5, collision=0)
    add("latched and hit on the tick the wait reaches 3.0", hit, 2.5, 0.5)
    add("fresh hit", hit, 0.0, 0.1, collision=0)
    add("latched, delta_t 0", free, 1.25, 0.0)
    add("not latched, wait left alone", free, 1.25, 0.5, collision=0)
    add("footprint stop counts the wait", free, 1.0, 0.5, collision=0, fcost=1.0)
    add("footprint stop clears the latch at 3.0", free, 2.5, 0.5, fcost=1.0)
    add("footprint cost 0.99 does not stop", free, 1.0, 0.5, collision=0, fcost=0.99)
    return b.case("wait and latch", params, [tuple(m)],
                  expect=("release", "latched stop without a hit", "hit in the middle", "moves"))


def footprint_stop_is_not_latched():
    """footprint_cost 1.0, then 0.99 on the next call: the robot moves again at once (py:343-347 assigns, py:338-341 latches)."""
    n, dt, yaw0, start = 3, 0.8 / 3, 0.4, (10, 10)
    x = controls_through(start, yaw0, [(11, 10), (12, 10), (12, 11)], turns(n), dt)
    b = _Batch(n)
    p = make_problem(start, yaw0, delta_t=0.5)
    b.add("robot", p, make_state(p, last=x[:3], wait=0.5), x)
    calls = [Call([x], footprint_cost=np.array([1.0])), Call([x], footprint_cost=np.array([0.99]))]
    return b.case("footprint stop is not latched", params_for(n), [tuple(free_map())], calls=calls, expect=("moves",))


def wait_chain():
    """32 calls at delta_t 0.1 on one latched record: the wait is the running sum 0.1 + 0.1 + ... in that order (twenty-nine
    additions give 2.9000000000000012, thirty give 3.0000000000000013: the thirtieth call releases, 30 * 0.1 formed any other
    way need not), the calls after it move.  The second record is hit afresh on call 10 and waits from there."""
    n, dt, yaw0, start = 3, 0.8 / 3, 0.4, (10, 10)
    m = free_map()
    m[0][20, 12] = 254
    free = controls_through(start, yaw0, [(11, 10), (12, 10), (12, 11)], turns(n), dt)
    hit = controls_through(start, yaw0, [(11, 10), (12, 20), (12, 11)], turns(n), dt)
    b = _Batch(n)
    p = make_problem(start, yaw0, delta_t=0.1)
    b.add("latched from the start", p, make_state(p, last=free[:3], collision=1), free)
    b.add("hit on call 10", p.copy(), make_state(p, last=free[:3], collision=0), free)
    calls = [Call([free, hit if k == 10 else free]) for k in range(32)]
    return b.case("wait chain", params_for(n), [tuple(m)], calls=calls, expect=("release", "latched stop without a hit", "moves"))


# ---------------------------------------------------------------------------------------------------------- clamp
CLAMP_ACC = (2.5, 1.75, 3.0)
CLAMP_INTERVALS = (0.0, 1.0 / 30.0, 0.1)


def clamp():
    """Gain 1: the filtered block IS the solution's, so it can be put exactly on last +- acc * ci (the reference's own two
    roundings), one ulp inside and one ulp outside; far outside as well."""
    n = 3
    params = params_for(n, low_pass_gain=1.0, acc_x_limit=CLAMP_ACC[0], acc_y_limit=CLAMP_ACC[1], acc_theta_limit=CLAMP_ACC[2])
    last = (0.11, -0.07, 0.05)
    base = np.array([0.12, -0.06, 0.04, 0.05, 0.02, -0.1, -0.03, 0.04, 0.2])   # (moves of centimetres on a free map)
    b = _Batch(n)
    for ci in CLAMP_INTERVALS:
        for axis in range(3):
            for side in (1.0, -1.0):
                bound = last[axis] + side * CLAMP_ACC[axis] * ci
                away = side * np.inf
                for name, v in (("on", bound), ("one ulp inside", np.nextafter(bound, -away)),
                                ("one ulp outside", np.nextafter(bound, away)), ("far outside", bound + side * 0.75)):
                    x = base.copy()
                    x[axis] = v
                    # (the start is no cell centre here: a third of a cell from the edges)
                    p = make_problem((10, 10), 0.3, control_interval=ci)
                    p["cur_xy"] += (RES / 6, -RES / 6)
                    b.add("ci %.4f axis %d side %+d %s" % (ci, axis, side, name), p, make_state(p, last=last), x)
    return b.case("clamp", params, [tuple(free_map())], expect=tuple("clamp %s axis %d" % (s, a) for s in ("above", "below") for a in range(3)))


# ---------------------------------------------------------------------------------------------------------- goal record
def goal_record():
    n, dt, yaw0, start = 3, 0.8 / 3, -0.8, (10, 10)
    x = controls_through(start, yaw0, [(11, 10), (12, 10), (12, 11)], turns(n), dt)
    last = tuple(x[:3] + (0.3, -0.2, 0.1))
    b = _Batch(n)

    def add(name, old_goal=None, has_goal=1, collision=0, **fields):
        p = make_problem(start, yaw0, delta_t=0.25, **fields)
        b.add(name, p, make_state(p, last=last, wait=1.5, collision=collision, has_goal=has_goal, old_goal=old_goal), x)
        return p
    p0 = add("same goal")
    goal = np.concatenate([p0["goal_xyz"][0], p0["goal_q"][0]])
    for k in range(7):
        g = goal.copy()
        g[k] += 1e-9
        add("component %d differs by 1e-9" % k, old_goal=g, collision=k % 2)
    add("has_old_goal 0, equal numbers", has_goal=0)
    add("has_old_goal 0, latched", has_goal=0, collision=1)
    add("has_old_goal 2 counts as set", has_goal=2)
    add("-0.0 against 0.0", old_goal=np.where(goal == 0.0, -0.0, goal))
    z = goal.copy()
    z[2] = np.nan
    add("NaN goal z", old_goal=z, goal_xyz=(z[0], z[1], np.nan))         # (equal bytes on both sides: still a new goal)
    add("NaN goal quaternion x, latched", collision=1, goal_q=(np.nan,) + tuple(goal[4:]))
    calls = [Call(np.array(b.x)), Call(np.array(b.x))]                     # twice: the NaN goals reset every call
    return b.case("goal record", params_for(n), [tuple(free_map())], calls=calls, expect=("reset", "moves", "latched stop without a hit"))


# ---------------------------------------------------------------------------------------------------------- failed solve
def failed_solve(n):
    rng = np.random.default_rng(500 + n)
    params = params_for(n, low_pass_gain=0.3)
    b = _Batch(n)
    for i in range(12):
        x = rng.uniform(-0.01, 0.01, size=3 * n) / n      # (millimetres of travel: the start's cell, a third of a cell from its edges)
        x[2::3] = rng.uniform(-0.7, 0.7, size=n)
        p = make_problem((10 + i, 12), 0.1 * i - 0.5, control_interval=10.0)
        p["cur_xy"] += (RES / 6, RES / 6)
        last = tuple(x[:3] + rng.uniform(-0.01, 0.01, size=3))
        b.add("record %d %s" % (i, "failed" if i % 3 == 1 else "solved"), p, make_state(p, last=last), x, ok=0 if i % 3 == 1 else 1,
              warm=rng.uniform(-1, 1, size=3 * n))
    mixed = Call(np.array(b.x), np.array(b.ok))
    flipped = Call(np.array(b.x)[::-1].copy(), 1 - np.array(b.ok))
    return b.case("failed solve, n=%d" % n, params, [tuple(free_map())], calls=[mixed, flipped, Call(np.array(b.x), None)],
                  expect=("un-shifted warm start", "moves"))


# ---------------------------------------------------------------------------------------------------------- skip and pool
POOL_ORIGINS = ((-1.0, -1.0), (3.5, -7.25), (-12.0, 0.65))


def skip_and_pool(count):
    """Three maps with origins of their own; record i looks at map_index[i] (out-of-range indices are clamped into the pool).
    The lethal cell a record's stage 1 stands on is there in ONE map only: the record hits iff that is its own.  Every
    third row is skipped (two in a row among them)."""
    n, dt, yaw0 = 3, 0.8 / 3, 2.5
    maps = [free_map(o) for o in POOL_ORIGINS]
    for k, m in enumerate(maps):
        m[0][15, 12 + k] = 254                          # cell (12 + k, 15) in map k alone
    index = [0, 1, 2, -1, 3, 100, -2 ** 31, 2 ** 31 - 1]
    b = _Batch(n)
    for i in range(count):
        mi = index[i % len(index)]
        own = min(max(mi, 0), 2)
        origin = POOL_ORIGINS[own]
        target = (i // 3) % 3                            # whose lethal cell the rollout visits
        x = controls_through((10, 10), yaw0, [(11, 10), (12 + target, 15), (12, 11)], turns(n), dt, origin=origin)
        skip = 1 if (i % 3 == 1 or i % 7 == 2) and count > 1 else 0
        p = make_problem((10, 10), yaw0, origin=origin, map_index=mi, skip=skip)
        b.add("record %d map_index %d visits %d%s" % (i, mi, target, " skipped" if skip else ""), p,
              make_state(p, last=x[:3], wait=0.75), x, warm=np.arange(3 * n) + 0.5 + i)
    return b.case("skip and pool, %d records" % count, params_for(n), [tuple(m) for m in maps], pooled=True,
                  expect=("hit in the middle", "moves", "skipped") if count > 1 else ("hit in the middle",))


def pool_edges():
    """The map-edge records against the second map of a pool: its origin, its padding."""
    n = 3
    maps = [free_map(o) for o in POOL_ORIGINS]
    b = _Batch(n)
    _edge_records(b, n, 0.8 / n, origin=POOL_ORIGINS[1], map_index=1)
    return b.case("pool edges", params_for(n), [tuple(m) for m in maps], pooled=True,
                  expect=("hit at stage 0", "hit at the last stage", "moves"))


def all_cases():
    cases = [one_stage_hits(n) for n in STAGE_COUNTS]
    cases += [map_edges(), far_stage()]
    cases += [low_pass_decides(n, g) for n in (1, 3) for g in (0.0, 0.3, 1.0)]
    cases += [wait_and_latch(), footprint_stop_is_not_latched(), wait_chain(), clamp(), goal_record()]
    cases += [failed_solve(n) for n in (1, 3, 8)]
    cases += [skip_and_pool(1), skip_and_pool(65), pool_edges()]
    return cases


# ---------------------------------------------------------------------------------------------------------- preconditions
def branches(case, run):
    """The names of the branches the reference takes somewhere in `run` (Case.reference_run)."""
    n, seen = case.n, set()
    for p, e in run:
        for i, r in enumerate(e["records"]):
            if r is None:
                seen.add("skipped")
                continue
            h = r["hit_stage"]
            if h == 0:
                seen.add("hit at stage 0")
            if h == n - 1:
                seen.add("hit at the last stage")
            if 0 < h < n - 1:
                seen.add("hit in the middle")
            if r["released"]:
                seen.add("release")
            if r["stopped"] and h < 0 and r["collision"]:
                seen.add("latched stop without a hit")
            if r["reset"]:
                seen.add("reset")
            if not r["stopped"]:
                seen.add("moves")
                for a in range(3):
                    if r["vel"][a] < r["filtered_x"][a]:
                        seen.add("clamp above axis %d" % a)
                    if r["vel"][a] > r["filtered_x"][a]:
                        seen.add("clamp below axis %d" % a)
            if not r["has_prev_u0"]:
                seen.add("un-shifted warm start")
    return seen


def check(case, run):
    """The builder's own preconditions, with the reference alone: every filtered position of every record at least MARGIN
    from a cell edge, every branch the case names taken by at least one record."""
    for p, e in run:
        live = ~e["skipped"]
        worst = e["edge_distance"][live].min() if live.any() else np.inf
        assert worst >= MARGIN, (case.name, worst, [case.names[i] for i in np.nonzero((e["edge_distance"] < MARGIN).any(axis=1))[0]])
    missing = set(case.expect) - branches(case, run)
    assert not missing, (case.name, sorted(missing))


# ---------------------------------------------------------------------------------------------------------- fused K2
FUSED_ROWS = ((3, 0), (3, 1), (3, 3), (8, 0), (8, 1), (8, 2), (32, 0), (32, 1),     # test_kernel_gradient_matches_reference_fd_gradient's
              (1, 0), (64, 0), (3, 2))                                              # ... and (1, AUTO), (64, AUTO), (3, NEWTON)
FUSED_COUNT, FUSED_MAP = 256, 200
FUSED_SPEED_CAP = 4.0     # |last_control| stays of order one: the 1e-14 of the comparisons is an absolute bound


def fused_batch(n, method, max_iterations=None):
    """256 robots on synthetic.make_costmap(200) in states a solve seldom meets: a third latched with waits around 3.0, a
    quarter with a goal that changed in one component, a few footprint costs of 1.0, gain 0.3 and -- where a speed of
    FUSED_SPEED_CAP gets there -- last_control aimed at the nearest lethal cell, so that the filtered first block drives
    into it whatever the search answers.  Returns (params, cmap, problems, states, warm)."""
    params = orc.make_params(control_steps=n, method=method, low_pass_gain=0.3)
    if max_iterations is not None:
        params["max_iterations"] = max_iterations
    cmap = synthetic.make_costmap(FUSED_MAP)
    probs = synthetic.make_problems(FUSED_COUNT, FUSED_MAP, seed=900 + n)
    st, warm = synthetic.make_states(probs, n)
    rng = np.random.default_rng(7000 + 10 * n + method)
    cells, res, ox, oy = cmap
    ly, lx = np.nonzero(cells == 254)
    lethal = np.stack([ox + (lx + 0.5) * res, oy + (ly + 0.5) * res], axis=1)
    dt = params["prediction_horizon"] / n
    for i in range(FUSED_COUNT):
        d = lethal - probs["cur_xy"][i]
        d = d[np.argmin((d * d).sum(axis=1))] * rng.uniform(0.9, 1.2)
        q = probs["cur_q"][i]
        yaw = orc.yaw_from_quaternion(*q)
        c, s = math.cos(yaw), math.sin(yaw)
        v = np.array([d[0] * c + d[1] * s, -d[0] * s + d[1] * c]) / (0.7 * dt)
        if np.hypot(*v) <= FUSED_SPEED_CAP and i % 2 == 0:
            st["last_control"][i] = (v[0], v[1], 0.0)
        if i % 3 == 0:
            st["collision"][i] = 1
            third = 3.0 - 1.0 / 30.0
            st["waiting_time"][i] = (1.0, third, np.nextafter(third, 0.0), np.nextafter(third, 4.0), 2.99, 2.9, 3.0 - 2.0 / 30.0)[(i // 3) % 7]
        if i % 4 == 1:
            st["old_goal"][i][rng.integers(7)] += 1e-9
        if i % 37 == 5:
            probs["footprint_cost"][i] = 1.0
    return params, cmap, probs, st, warm
