"""The map fence across streams: one side of a write / read pair is HELD BACK on its stream by a bounded device-side
delay, the other side is enqueued afterwards on another stream (or through a host entry point, which works on the null
stream), and the test looks at which map the reader saw.  With the fence of csrc/neo_mpc_capi.cpp (`MapFence`, the
world map's `world_ready` event) the answer is fixed; without it the side that is not held runs at once and the answer is
the opposite one -- a deterministic wrong result, not a race won by luck.  Only the ORDER is under test: every expected
value is the library's own answer to the same calls made one at a time with a synchronisation behind each (kernel
correctness against the references is the other test files' job), and every comparison is exact.

What include/neo_mpc.h promises and these scenarios hold it to:
  1  read after write: a held ingest, pool ingest, roll or stamp -- the reader on another stream sees the NEW map;
  2  write after read: a held solve or gate sees the OLD map whatever writer follows it on another stream;
  3  write after write: two writers on two streams leave what they leave one after the other;
  4  a chain over four streams;
  5  the world map's copy against the rolls that read it;
  6  the host-side tables (the per-step costmap terms, a host pool's origins): they are rewritten only after every launch
     that may still read them has ENDED, also a reader that a later write on another stream has already cleared
     (docs/NOTEBOOK.md A.10's hole: scenario 6b).

Two conditions keep a scenario from passing for the wrong reason; both are asserted in every scenario and a miss FAILS
with "inconclusive":
  (1) the delay was still running right after the scenario's last asynchronous call (just before a host call that has
      to block -- and it has ended when that call returns);
  (2) the streams really run side by side: a trivial operation enqueued on each stream that is not held ends while the
      delay is running (two streams may share one of the runtime's hardware queues; further fresh streams are tried, at
      most eight).  The stream neo_mpc_solve_batch_begin works on is the library's own: it is put to the same test with
      a short delay before the scenario starts.

The delay: torch.cuda._sleep, its cycle count calibrated once per module with an event pair (a chain of matrix products
sized by the same calibration where _sleep does nothing).  It always ends by itself.  Its length: the host needs
0.08 ms to enqueue the slowest scenario without a delay (measured on an MI355X after a warm-up; every test prints
its own figure); 20 times that is below the floor of 50 ms, so D = 50 ms.  Every scenario asserts that 20 times the enqueue
time it measured itself is no more than D, and that the delay it ran under lasted no more than the ceiling of 500 ms.
"""
import ctypes as C
import functools
import time
from collections import namedtuple

import numpy as np
import pytest

from neo_mpc_planner2_amd import _lib, abi, synthetic
from tests import util

pytestmark = pytest.mark.gpu

HOLD_MS = 50.0            # D; every scenario asserts 20 x its own enqueue time <= D and that the delay ran <= MAX_HOLD_MS
MAX_HOLD_MS = 500.0
PROBE_HOLD_MS = 20.0      # the short delay streams are chosen with
SIDE_BY_SIDE_MS = 50.0    # condition 2: how long the operation on the other stream may take to end
DEV = "cuda:0"
RES = 0.05
COUNT = 256               # robots per solve or gate
SINGLE = 200              # the single map: 200 x 200 cells, origin (-5, -5)
SINGLE_GEOM = (RES, -5.0, -5.0)
POOL, WIN_X, WIN_Y = 8, 64, 48
WORLD = 256               # the world map: 256 x 256 cells at (0, 0)
WORLD_GEOM = (RES, 0.0, 0.0)
STAMP = (0.3, 0.0, 1.0)   # inscribed_radius, inflation_radius (no ring), cost_scaling_factor
RECT = np.asarray(synthetic.RECT_FOOTPRINT, dtype=np.float64)


# ------------------------------------------------------------------------------------------ inputs, made once
def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def single_maps():
    a = synthetic.make_costmap(SINGLE, seed=1)[0]
    return dict(free=_frozen(np.zeros((SINGLE, SINGLE), dtype=np.uint8)), lethal=_frozen(np.full((SINGLE, SINGLE), 254, dtype=np.uint8)),
                mid=_frozen(np.full((SINGLE, SINGLE), 100, dtype=np.uint8)), a=_frozen(a), b=_frozen(synthetic.make_costmap(SINGLE, seed=2)[0]),
                a1=_frozen(np.maximum(a, 1)))          # (no free cell: a gate on it never answers 0)


@functools.lru_cache(maxsize=None)
def pool_maps():
    cut = lambda seed: np.stack([synthetic.make_costmap(WIN_X, seed=seed + k, n_discs=3)[0][:WIN_Y] for k in range(POOL)])
    shape = (POOL, WIN_Y, WIN_X)
    return dict(free=_frozen(np.zeros(shape, dtype=np.uint8)), lethal=_frozen(np.full(shape, 254, dtype=np.uint8)),
                mid=_frozen(np.full(shape, 100, dtype=np.uint8)), a=_frozen(cut(10)), b=_frozen(cut(20)))


@functools.lru_cache(maxsize=None)
def world_maps():
    shape = (WORLD, WORLD)
    return dict(free=_frozen(np.zeros(shape, dtype=np.uint8)), lethal=_frozen(np.full(shape, 254, dtype=np.uint8)),
                a=_frozen(synthetic.make_costmap(WORLD, seed=3)[0]), b=_frozen(synthetic.make_costmap(WORLD, seed=4)[0]))


#: the windows' origins: on the world's cell lattice, every window wholly inside the world; and the pool's other origins (6c, 6d)
POOL_ORIGINS = _frozen(np.array([(0.6 + k, 1.0 + k) for k in range(POOL)], dtype=np.float64))
OTHER_ORIGINS = _frozen(POOL_ORIGINS + 0.35)


@functools.lru_cache(maxsize=None)
def stamp_polygons():
    """Robot j as a rectangle a little larger than window j + 1: every window is covered by a robot that is not its own,
    so one stamp turns an all-free pool into an all-lethal one."""
    out = np.zeros((POOL, 4, 2))
    for j in range(POOL):
        x0, y0 = POOL_ORIGINS[(j + 1) % POOL] - 0.1
        x1, y1 = POOL_ORIGINS[(j + 1) % POOL] + (WIN_X * RES + 0.1, WIN_Y * RES + 0.1)
        out[j] = ((x0, y0), (x1, y0), (x1, y1), (x0, y1))
    return _frozen(out)


@functools.lru_cache(maxsize=None)
def small_stamp_polygons():
    """Robot j as a square of 1 m in the middle of window j + 1: a stamp leaves most of every window as it found it."""
    out = np.zeros((POOL, 4, 2))
    for j in range(POOL):
        cx, cy = POOL_ORIGINS[(j + 1) % POOL] + (WIN_X * RES / 2, WIN_Y * RES / 2)
        out[j] = ((cx - 0.5, cy - 0.5), (cx + 0.5, cy - 0.5), (cx + 0.5, cy + 0.5), (cx - 0.5, cy + 0.5))
    return _frozen(out)


@functools.lru_cache(maxsize=None)
def robots(pool, count=COUNT, seed=5):
    """(request records, gate poses [count, 3], map indices or None): every robot well inside its map -- with a pool inside
    its window at both sets of origins."""
    probs = synthetic.make_problems(count, SINGLE if not pool else WIN_X, seed=seed)
    rng = np.random.default_rng(seed + 100)
    idx = None
    if pool:
        idx = (np.arange(count) % POOL).astype(np.int32)
        probs["cur_xy"] = POOL_ORIGINS[idx] + rng.uniform((0.9, 0.9), (2.3, 1.5), size=(count, 2))
        probs["map_index"] = idx
    poses = np.concatenate([probs["cur_xy"], rng.uniform(-np.pi, np.pi, size=(count, 1))], 1)
    return _frozen(probs), _frozen(poses), None if idx is None else _frozen(idx)


# ------------------------------------------------------------------------------------------ the delay
@functools.lru_cache(maxsize=None)
def _delay():
    """-> enqueue(ms) on torch's current stream, calibrated once."""
    import torch

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    if hasattr(torch.cuda, "_sleep"):
        torch.cuda._sleep(1000)
        torch.cuda.synchronize()
        cycles = 2_000_000
        for _ in range(3):
            ms = timed(lambda: torch.cuda._sleep(cycles))
            if ms >= 1.0:
                per_ms = cycles / ms
                print("delay: torch.cuda._sleep, %.0f cycles per ms" % per_ms)
                return lambda want: torch.cuda._sleep(int(want * per_ms))
            cycles *= 16
    # _sleep does nothing here: a chain of matrix products, each ordered behind the last by the stream
    x = torch.ones((1024, 1024), device=DEV)
    y = torch.empty_like(x)
    torch.mm(x, x, out=y)
    torch.cuda.synchronize()
    per_op = timed(lambda: [torch.mm(x, x, out=y) for _ in range(64)]) / 64
    print("delay: a chain of matrix products, %.3f ms each" % per_op)
    return lambda want: [torch.mm(x, x, out=y) for _ in range(int(want / per_op) + 1)]


def hold(stream, ms=HOLD_MS):
    """A bounded spin on `stream` -> the event recorded behind it (`.began`: the event in front of it)."""
    import torch
    with torch.cuda.stream(stream):
        began = torch.cuda.Event(enable_timing=True)
        began.record(stream)
        _delay()(ms)
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(stream)
    ev.began = began
    return ev


def _ends_within(event, ms):
    deadline = time.perf_counter() + ms / 1e3
    while not event.query():
        if time.perf_counter() > deadline:
            return False
    return True


# ------------------------------------------------------------------------------------------ one handle and its arrays
#: one call of a scenario: on the held stream "H", on another stream of the caller's ("A", "B", "C"), or through a host
#: entry point (None: the library works on the null stream).  `blocks`: a host call that may only return when the held
#: work has ended
Step = namedtuple("Step", "stream call blocks", defaults=(False,))


class Rig:
    """One handle, and every array a scenario touches: all of them exist before the delay starts."""

    def __init__(self, pool, **params):
        import torch
        from neo_mpc_planner2_amd.solver import BatchSolver
        self.torch = torch
        self.pool = pool
        self.params = util.orc.make_params(**params)
        assert self.params["control_steps"] == 3
        self.s = BatchSolver(self.params)
        self.probs, self.poses, self.idx = robots(pool)
        self._tensors = {}
        self.dev_out, self.host_out = {}, {}
        self._restore = []           # (tensor or array, its pristine copy)
        self._pinned = []
        self.d_fp, self.d_poses = self.t(RECT), self.t(self.poses)
        self.d_idx = self.t(self.idx) if pool else None
        self.d_origins = torch.from_numpy(POOL_ORIGINS.copy()).to(DEV) if pool else None
        self.probe = torch.zeros(16, device=DEV)
        self.probe.add_(1)
        torch.cuda.synchronize()

    def close(self):
        self.torch.cuda.synchronize()
        self.s.close()
        for a in self._pinned:
            _lib.load().neo_mpc_unpin_host_memory(C.c_void_p(a.ctypes.data))

    def t(self, array):
        """The device copy of a module-level input (made on first use: in a serial pass, never under the delay)."""
        key = id(array)
        if key not in self._tensors:
            self._tensors[key] = (array, self.torch.from_numpy(np.array(array)).to(DEV))
        return self._tensors[key][1]

    def reset(self):
        for live, pristine in self._restore:
            if isinstance(live, np.ndarray):
                live[...] = pristine
            else:
                live.copy_(pristine)
        for out in self.dev_out.values():
            out.zero_()
        self.host_out.clear()
        self.torch.cuda.synchronize()

    def outputs(self):
        self.torch.cuda.synchronize()
        out = {k: v.copy() for k, v in self.host_out.items()}
        for k, v in self.dev_out.items():
            a = v.cpu().numpy()
            out[k] = a.view(abi.COMMAND_DTYPE).reshape(-1) if a.dtype == np.uint8 else a
        return out

    # -- readers: each returns the steps that write the output `name`
    def solve_device(self, name, stream, timed=False):
        from neo_mpc_planner2_amd.solver import DeviceBatch
        torch = self.torch
        st, warm = synthetic.make_states(self.probs, 3)
        db = DeviceBatch(self.probs, st, warm, DEV, want_solution=False)
        self._restore += [(db.states, db.states.clone()), (db.warm, db.warm.clone())]
        self.dev_out[name] = db.commands
        events = None
        if timed:
            events = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            for e in events:
                e.record()
        return [Step(stream, lambda: self.s.solve_device(db.problems, db.states, db.warm, db.commands, events=events))]

    def gate_device(self, name, stream):
        costs = self.torch.zeros(COUNT, dtype=self.torch.float64, device=DEV)
        self.dev_out[name] = costs
        return [Step(stream, lambda: self.s.footprint_gate_device(self.d_fp, costs, poses=self.d_poses, map_indices=self.d_idx))]

    def readback(self, name, stream=None):
        def call():
            self.host_out[name], self.host_out[name + " origins"] = self.s.get_costmap_pool()
        return [Step(None, call, True)]

    def solve_host(self, name, count):
        probs = robots(self.pool, count, seed=7)[0]
        st0, warm0 = synthetic.make_states(probs, 3)

        def call():
            self.host_out[name] = self.s.solve(probs, st0.copy(), warm0.copy())[0].copy()
        return [Step(None, call, True)]

    def solve_begin_wait(self, name):
        st, warm = synthetic.make_states(self.probs, 3)
        arrays = [self.probs.copy(), st, warm, np.zeros(COUNT, dtype=abi.COMMAND_DTYPE), np.zeros((COUNT, 9))]
        for a in arrays:
            assert _lib.load().neo_mpc_pin_host_memory(C.c_void_p(a.ctypes.data), a.nbytes) == 0, _lib.load().neo_mpc_last_error()
            self._pinned.append(a)
            self._restore.append((a, a.copy()))
        ticket = []

        def begin():
            ticket.append(self.s.solve_begin(arrays[0], arrays[1], arrays[2], out=(arrays[3], arrays[4])))

        def wait():
            self.host_out[name] = self.s.solve_wait(ticket.pop())[0].copy()
        return [Step(None, begin), Step(None, wait, True)]

    def postprocess(self, name):
        st0, warm0 = synthetic.make_states(self.probs, 3)
        x = np.random.default_rng(11).uniform(-0.3, 0.3, size=(COUNT, 9))

        def call():
            self.host_out[name] = self.s.postprocess(self.probs, st0.copy(), warm0.copy(), x).copy()
        return [Step(None, call, True)]

    def objective(self, name):
        u = np.random.default_rng(12).uniform(-0.3, 0.3, size=(COUNT, 9))

        def call():
            self.host_out[name] = self.s.objective(self.probs, u)
        return [Step(None, call, True)]

    def gate_host(self, name):
        def call():
            self.host_out[name] = self.s.footprint_gate(RECT, poses=self.poses, map_indices=self.idx)
        return [Step(None, call, True)]

    def reader(self, kind, name, stream):
        if kind == "solve_device":
            return self.solve_device(name, stream)
        if kind == "solve_device_timed":
            return self.solve_device(name, stream, timed=True)
        if kind == "gate_device":
            return self.gate_device(name, stream)
        if kind == "get_costmap_pool":
            return self.readback(name)
        if kind == "solve-staged-700":
            return self.solve_host(name, 700)
        if kind == "solve-latency-48":
            return self.solve_host(name, 48)
        return {"solve_begin-wait": self.solve_begin_wait, "postprocess": self.postprocess, "objective": self.objective,
                "footprint_gate": self.gate_host}[kind](name)

    # -- writers
    def writer(self, kind, old, new):
        """-> (install: the old map, made with synchronous calls; write: the device entry point on torch's current stream;
        write_host: the host entry point) for one of the four kinds of write.  `old` / `new` name the maps (of the world for
        a roll; a stamp turns `old` all lethal)."""
        s = self.s
        if kind == "ingest":
            maps = single_maps()
            return (lambda: s.set_costmap(self.t(maps[old]), *SINGLE_GEOM), lambda: s.set_costmap(self.t(maps[new]), *SINGLE_GEOM),
                    lambda: s.set_costmap(maps[new], *SINGLE_GEOM))
        maps = pool_maps()
        install = lambda: s.set_costmap_pool(self.t(maps[old]), RES, self.d_origins)
        if kind == "pool":
            return (install, lambda: s.set_costmap_pool(self.t(maps[new]), RES, self.d_origins),
                    lambda: s.set_costmap_pool(maps[new], RES, POOL_ORIGINS))
        if kind == "stamp":
            return (install, lambda: s.stamp_fleet(*STAMP, polygons=self.t(stamp_polygons())),
                    lambda: s.stamp_fleet(*STAMP, polygons=stamp_polygons()))
        assert kind == "roll"
        worlds = world_maps()

        def install_rolled():
            s.set_world_map(worlds[old], *WORLD_GEOM)
            self.roll()
            s.set_world_map(worlds[new], *WORLD_GEOM)      # (the host variant waits for the roll)
        return install_rolled, self.roll, lambda: s.roll_costmap_pool(WIN_X, WIN_Y, RES, POOL_ORIGINS.copy())

    def roll(self):
        self.s.roll_costmap_pool(WIN_X, WIN_Y, RES, self.d_origins)


@pytest.fixture
def rig():
    made = []

    def make(pool, **params):
        made.append(Rig(pool, **params))
        return made[-1]
    yield make
    for r in made:
        r.close()


# ------------------------------------------------------------------------------------------ the runner
def _poke(rig, stream):
    """A trivial operation on `stream` -> the event behind it."""
    torch = rig.torch
    with torch.cuda.stream(stream):
        rig.probe.add_(1)
        ev = torch.cuda.Event()
        ev.record(stream)
    return ev


def _side_by_side(rig, held, poke):
    """Does what `poke` enqueues (-> an event behind it, or None after a host wait of its own) end while a short delay
    is running on `held`?"""
    ev = hold(held, PROBE_HOLD_MS)
    behind = poke()
    ok = (behind is None or _ends_within(behind, SIDE_BY_SIDE_MS)) and not ev.query()
    ev.synchronize()
    rig.torch.cuda.synchronize()
    return ok


def _choose_streams(rig, names, uses_null, own_stream_probe):
    torch = rig.torch
    null = torch.cuda.default_stream()
    for _ in range(8):
        held = torch.cuda.Stream()
        if uses_null and not _side_by_side(rig, held, lambda: _poke(rig, null)):
            continue
        if own_stream_probe is not None and not _side_by_side(rig, held, own_stream_probe):
            continue
        break
    else:
        pytest.fail("inconclusive: no stream found that runs side by side with the stream(s) the library works on")
    streams, tried = {"H": held}, 0
    for name in names:
        while name not in streams:
            if tried == 8:
                pytest.fail("inconclusive: eight fresh streams, none runs side by side with the held one")
            tried += 1
            fresh = torch.cuda.Stream()
            if all(fresh.cuda_stream != s.cuda_stream for s in streams.values()) and \
                    _side_by_side(rig, held, lambda: _poke(rig, fresh)):
                streams[name] = fresh
    streams[None] = null
    return streams


def _each_differs(x, y):
    if x.dtype.fields:     # records: every record
        x, y = (v.view(np.uint8).reshape(len(v), -1) for v in (x, y))
        return bool((x != y).any(axis=1).all())
    return bool((x != y).all())


def run(rig, prepare, steps, differ, own_stream_probe=None, check=None):
    """`prepare()` brings handle and arrays to the scenario's start with synchronous calls (and may leave outputs of its
    own: what the other order would give).  `steps` run twice one at a time, a synchronisation behind each -- the first
    pass allocates every buffer, stamp table and stream slot, both yield the expected outputs -- and then once with the
    first of them held back.  `differ`: (output, output, "each" | "any") -- the pairs that must differ, in every robot or
    cell or as arrays, for the scenario to prove anything; `check(outputs)`: what else the serial answers have to show."""
    torch = rig.torch
    assert steps[0].stream == "H"
    names = sorted({s.stream for s in steps if s.stream not in ("H", None)})
    uses_null = any(s.stream is None for s in steps)
    prepare()
    torch.cuda.synchronize()
    streams = _choose_streams(rig, names, uses_null, own_stream_probe)

    def call(step):
        with torch.cuda.stream(streams[step.stream]):
            step.call()

    serial = []
    for _ in range(2):
        rig.reset()
        prepare()
        torch.cuda.synchronize()
        enqueue = 0.0
        for step in steps:
            t0 = time.perf_counter()
            call(step)
            if not step.blocks:
                enqueue += time.perf_counter() - t0
            torch.cuda.synchronize()
        serial.append(rig.outputs())
    want = serial[1]
    print("host time to enqueue the asynchronous calls, no delay: %.3f ms" % (1e3 * enqueue))
    assert 20 * 1e3 * enqueue <= HOLD_MS, "inconclusive: D = %g ms is less than 20 x the %.3f ms the host needs to enqueue" % (HOLD_MS, 1e3 * enqueue)
    assert sorted(serial[0]) == sorted(want) and all(np.array_equal(serial[0][k], want[k]) for k in want), "the serial answers differ"
    for x, y, how in differ:
        assert (_each_differs(want[x], want[y]) if how == "each" else want[x].tobytes() != want[y].tobytes()), \
            "%r and %r do not differ (%s): the scenario would prove nothing" % (x, y, how)
    if check is not None:
        check(want)

    rig.reset()
    prepare()
    torch.cuda.synchronize()
    first_block = next((k for k, s in enumerate(steps) if s.blocks), len(steps))
    held = hold(streams["H"])
    try:
        for name in names + ([None] if uses_null else []):      # condition 2, under the delay the scenario runs under
            behind = _poke(rig, streams[name])
            assert _ends_within(behind, SIDE_BY_SIDE_MS) and not held.query(), \
                "inconclusive: stream %r does not run side by side with the held one" % (name,)
        for k, step in enumerate(steps):
            if k == first_block:                                 # condition 1
                assert not held.query(), "inconclusive: the delay had ended before the last asynchronous call was made"
            call(step)
            if step.blocks:
                assert held.query(), "host call %d returned while the held work was still running" % k
        if first_block == len(steps):
            assert not held.query(), "inconclusive: the delay had ended before the last asynchronous call was made"
    finally:
        torch.cuda.synchronize()
    got = rig.outputs()
    assert held.query()
    ran = held.began.elapsed_time(held)
    assert ran <= MAX_HOLD_MS, "the delay ran %.0f ms: the calibration is off" % ran
    assert sorted(got) == sorted(want)
    wrong = [k for k in sorted(want) if not np.array_equal(got[k], want[k])]
    assert not wrong, "not what the same calls give one after the other: %s" % ", ".join(wrong)


#: which pair of maps tells a reader's answers apart: all-free against all-lethal (a gate answers 0 against 254, every cell
#: and every record differs) -- two seeded costmaps for the solves
def _maps_for(reader):
    return ("a", "b", "any") if reader.startswith("solve") else ("free", "lethal", "each")


# ------------------------------------------------------------------------------------------ 1: read after write
WRITERS = ("ingest", "pool", "roll", "stamp")
DEVICE_ENTRY = {"ingest": "set_costmap_device", "pool": "set_costmap_pool_device", "roll": "roll_costmap_pool_device",
                "stamp": "stamp_fleet_device"}
HOST_ENTRY = {"ingest": "set_costmap", "pool": "set_costmap_pool", "roll": "roll_costmap_pool", "stamp": "stamp_fleet"}
FURTHER_READERS = ("solve-staged-700", "solve-latency-48", "solve_begin-wait", "solve_device_timed", "postprocess", "objective",
                   "footprint_gate")
RAW = [(w, r) for w in WRITERS for r in ("solve_device", "gate_device", "get_costmap_pool")] + [("ingest", r) for r in FURTHER_READERS]


@pytest.mark.parametrize("writer,reader", RAW, ids=["%s-%s" % (DEVICE_ENTRY[w], r) for w, r in RAW])
def test_1_a_reader_on_another_stream_sees_the_held_write(rig, writer, reader):
    r = rig(pool=writer != "ingest")
    old, new, how = _maps_for(reader)
    install, write, _ = r.writer(writer, old, new)
    before = r.reader(reader, "old map", "A")
    after = r.reader(reader, "new map", "A")

    def prepare():
        install()
        for step in before:
            step.call()
        r.torch.cuda.synchronize()

    probe = None
    if reader == "solve_begin-wait":
        def probe():
            for step in before:
                step.call()
    run(r, prepare, [Step("H", write)] + after, [("old map", "new map", how)], probe)


# ------------------------------------------------------------------------------------------ 2: write after read
WAR = [(r, w, host) for r in ("solve_device", "gate_device") for host in (False, True) for w in WRITERS]
#: the host writers that return only when their kernel has run (or wait for an idle map first); neo_mpc_set_costmap alone
#: leaves its ingest to the null stream
HOST_WRITER_BLOCKS = {"ingest": False, "pool": True, "roll": True, "stamp": True}


@pytest.mark.parametrize("reader,writer,host", WAR, ids=["%s-%s" % (r, (HOST_ENTRY if h else DEVICE_ENTRY)[w]) for r, w, h in WAR])
def test_2_a_held_reader_sees_the_map_from_before_the_write(rig, reader, writer, host):
    r = rig(pool=writer != "ingest")
    old, new, how = _maps_for(reader)
    install, write, write_host = r.writer(writer, old, new)
    steps = r.reader(reader, "held reader", "H")
    steps += [Step(None, write_host, HOST_WRITER_BLOCKS[writer])] if host else [Step("A", write)]
    steps += r.reader(reader, "reader behind the write", "B")
    run(r, install, steps, [("held reader", "reader behind the write", how)])


# ------------------------------------------------------------------------------------------ 3: write after write
@pytest.mark.parametrize("pair", ["ingest-ingest", "roll-ingest", "pool_ingest-stamp", "roll-stamp"])
def test_3_two_writers_on_two_streams_leave_what_they_leave_in_turn(rig, pair):
    """X is held, Y follows on another stream; the read-back is Y applied to X's map.  In the other order X would have
    had the last word: the read-back behind X alone, which prepare() leaves for the comparison.  The stamp covers the
    middle of each window only: the read-back carries the stamp AND X's cells around it (0), none of the map before X
    (100) -- the stamp modified X and nothing else."""
    first, second = pair.split("-")
    r = rig(pool=pair != "ingest-ingest")
    s = r.s
    if pair == "ingest-ingest":
        start, _, _ = r.writer("ingest", "mid", "mid")
        _, x, _ = r.writer("ingest", "mid", "free")
        _, y, _ = r.writer("ingest", "mid", "lethal")
    else:
        start, _, _ = r.writer("pool", "mid", "mid")
        if first == "roll":
            s.set_world_map(world_maps()["free"], *WORLD_GEOM)
            x = r.roll
        else:
            _, x, _ = r.writer("pool", "mid", "free")
        y = r.writer("pool", "mid", "lethal")[1] if second == "ingest" else \
            (lambda: s.stamp_fleet(*STAMP, polygons=r.t(small_stamp_polygons())))
    alone = r.readback("X alone")[0]

    def prepare():
        start()
        x()
        alone.call()
        start()
    check = None
    if second == "stamp":
        def check(want):
            cells = want["X then Y"]
            assert all((w == 254).any() and (w == 0).any() for w in cells) and set(np.unique(cells)) == {0, 254}
    run(r, prepare, [Step("H", x), Step("A", y)] + r.readback("X then Y"),
        [("X alone", "X then Y", "any" if second == "stamp" else "each")], check=check)


# ------------------------------------------------------------------------------------------ 4: a chain
def test_4_a_chain_over_four_streams(rig):
    """Held ingest A on S1, solve on S2, ingest B on S3, gate on S4: the solve sees A, the gate sees B.  (The map before A is
    all lethal, A a seeded costmap without a free cell, B all free: a gate answers 254, 1 or more, 0.)"""
    r = rig(pool=False)
    start, _, _ = r.writer("ingest", "lethal", "lethal")
    _, a, _ = r.writer("ingest", "lethal", "a1")
    _, b, _ = r.writer("ingest", "lethal", "free")
    others = r.solve_device("solve, map before", "A") + r.gate_device("gate, map before", "A") + [Step("A", a)] + \
        r.gate_device("gate, A", "A") + [Step("A", b)] + r.solve_device("solve, B", "A")

    def prepare():
        start()
        for step in others:
            step.call()
        r.torch.cuda.synchronize()
        start()
    steps = [Step("H", a)] + r.solve_device("solve", "A") + [Step("B", b)] + r.gate_device("gate", "C")
    run(r, prepare, steps, [("solve", "solve, map before", "any"), ("solve", "solve, B", "any"),
                            ("gate", "gate, map before", "each"), ("gate", "gate, A", "each")])


# ------------------------------------------------------------------------------------------ 5: the world map
def _world(r, name, host=False):
    cells = world_maps()[name]
    return (lambda: r.s.set_world_map(cells, *WORLD_GEOM)) if host else (lambda: r.s.set_world_map(r.t(cells), *WORLD_GEOM))


def _other_world_first(r, gate_name, cells_name):
    """prepare() of 5b and 5d: what roll and gate give on the NEW world, then the old world in its place and the pool
    as that roll left it."""
    gate, back = r.gate_device(gate_name, "A")[0], r.readback(cells_name)[0]

    def prepare():
        _world(r, "lethal", host=True)()
        r.roll()
        gate.call()
        back.call()
        _world(r, "free", host=True)()
    return prepare


def test_5a_a_roll_waits_for_the_held_copy_of_the_world_map(rig):
    r = rig(pool=True)
    back = r.readback("old world")[0]

    def prepare():
        _world(r, "free", host=True)()
        r.roll()
        back.call()
    run(r, prepare, [Step("H", _world(r, "lethal")), Step("A", r.roll)] + r.readback("new world"), [("old world", "new world", "each")])


@pytest.mark.parametrize("copy", ["set_world_map_device", "set_world_map"])
def test_5b_the_copy_waits_for_the_held_roll(rig, copy):
    r = rig(pool=True)
    host = copy == "set_world_map"
    steps = [Step("H", r.roll)] + r.gate_device("gate", "H") + [Step(None if host else "A", _world(r, "lethal", host), host)] + \
        r.readback("cells")
    run(r, _other_world_first(r, "gate, new world", "cells, new world"), steps,
        [("gate", "gate, new world", "each"), ("cells", "cells, new world", "each")])


def test_5c_two_copies_on_two_streams_and_the_roll_gets_the_second(rig):
    """Copy X is held on S1, copy Y follows on S2, the roll on S1 again: behind X in its stream, and behind Y by the copy's
    event alone."""
    r = rig(pool=True)
    back = r.readback("X")[0]

    def prepare():
        _world(r, "free", host=True)()
        r.roll()
        back.call()
        _world(r, "a", host=True)()
    run(r, prepare, [Step("H", _world(r, "free")), Step("A", _world(r, "lethal")), Step("H", r.roll)] + r.readback("Y"),
        [("X", "Y", "each")])


@pytest.mark.parametrize("copy", ["set_world_map_device", "set_world_map"])
def test_5d_the_copy_waits_for_the_held_roll_behind_an_ingest_too(rig, copy):
    """As 5b with a pool ingest of the same geometry between the roll and the copy: the map is no longer a rolled one when
    the copy is asked for, and the roll that reads the old copy has not started."""
    r = rig(pool=True)
    host = copy == "set_world_map"
    _, ingest, _ = r.writer("pool", "mid", "mid")
    steps = [Step("H", r.roll)] + r.gate_device("gate", "H") + [Step("A", ingest), Step(None if host else "B", _world(r, "lethal", host), host)]
    run(r, _other_world_first(r, "gate, new world", "cells, new world"), steps, [("gate", "gate, new world", "each")])


# ------------------------------------------------------------------------------------------ 6: the host-side tables
W_COSTMAP = (util.orc.make_params()["w_costmap"], 0.2)      # (both below w_trans / 4: the same search direction)


@pytest.mark.parametrize("case", ["a-set_params", "b-set_params-behind-a-write-that-cleared-the-reader", "c-set_costmap_pool",
                                  "d-roll_costmap_pool"])
def test_6_host_side_tables_are_rewritten_when_the_held_solve_has_ended(rig, case):
    """A solve is held on stream A; the host call that rewrites the term table (a, b) or the pool's origins and cells (c, d)
    returns only when that solve has ended, the solve's commands are the old table's / pool's and a solve behind it gives
    the new one's.  In (b) an ingest of the same cells on another stream has cleared the solve from the fence's pending
    readers before the table is rewritten."""
    case = case[0]
    r = rig(pool=case in "cd")
    s = r.s
    if case in "ab":
        install, same_again, _ = r.writer("ingest", "a", "a")

        def prepare():
            s.set_params(w_costmap=W_COSTMAP[0])
            install()
        rewrite = [Step("B", same_again)] if case == "b" else []
        rewrite += [Step(None, lambda: s.set_params(w_costmap=W_COSTMAP[1]), True)]
    elif case == "c":
        maps = pool_maps()
        prepare = lambda: s.set_costmap_pool(maps["a"], RES, POOL_ORIGINS)
        rewrite = [Step(None, lambda: s.set_costmap_pool(maps["b"], RES, OTHER_ORIGINS), True)]
    else:
        s.set_world_map(world_maps()["a"], *WORLD_GEOM)
        prepare = lambda: s.roll_costmap_pool(WIN_X, WIN_Y, RES, POOL_ORIGINS.copy())
        rewrite = [Step(None, lambda: s.roll_costmap_pool(WIN_X, WIN_Y, RES, OTHER_ORIGINS.copy()), True)]
    steps = r.solve_device("held solve", "H") + rewrite + r.solve_device("solve behind", "A")
    run(r, prepare, steps, [("held solve", "solve behind", "any")])
