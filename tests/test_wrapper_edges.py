"""The wrapper kernel (K2: everything of optimizer() behind the solve, py:365-403) at its edges, against the line-cited
reference `oracle/mpc_oracle.py::optimizer_step` (tests/wrapper_reference.py is the adaptor, tests/wrapper_cases.py the cases).

  * CPU: every case through the C mirror (`c_oracle.postprocess_batch`), bit for bit; the cases' own preconditions; the fused
    wrapper behind the mirror's solve.
  * GPU: every case through `BatchSolver.postprocess` (k_postprocess) on pageable arrays and on page-locked ones -- K2 on its
    own always stages its batch, page-locked arrays turn the copies into DMA transfers; the in-place path exists for the fused
    K2 only and is taken once in the fused test.
  * GPU and CPU: K2 fused behind every row of K1's dispatch table, from states a solve seldom meets, against the adaptor applied
    to the solution the solve returned.

What is exact and what is not: the decisions (collision, collision_footprint, has_old_goal, has_prev_u0, the RESET / STOPPED /
SKIPPED bits), waiting_time (additions only), prev_u0 (a copy), old_goal (by value), every zero of a stopped command and the
bytes of a skipped row are compared exactly.  vel, last_control and the warm start are within 1e-14 absolute (FMA contraction
in the low-pass and in the clamp's bound is the only freedom; the same bound as test_postprocess_kernel_reproduces_reference_
episodes), the path within 1e-12.  The one-ulp clamp records ("clamp": `... on`, `... one ulp inside`, `... one ulp outside`)
are the ones a contracted bound can move by an ulp of 0.1 (1.4e-17): the 1e-14 covers both admissible bounds, nothing else is
granted to them.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from neo_mpc_planner2_amd import abi
from oracle import c_oracle
from oracle import mpc_oracle as orc
from tests import wrapper_cases as wc
from tests import wrapper_reference as ref

CASES = wc.all_cases()
CASE_IDS = [c.name.replace(", ", "-").replace("=", "").replace(" ", "_") for c in CASES]
KEPT_BITS = abi.FLAG_RESET | abi.FLAG_STOPPED | abi.FLAG_SKIPPED      # (FLAG_WALL_IN_REACH is K1's set-up's to decide)


@functools.lru_cache(maxsize=None)
def reference_run(index):
    """The reference's answers for a case: computed once, shared by every test, never written to."""
    return CASES[index].reference_run()


# ------------------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("index", range(len(CASES)), ids=CASE_IDS)
def test_case_preconditions_hold_on_the_reference(index):
    case = CASES[index]
    assert len(case.problems) <= wc.MAX_RECORDS and all(m[0].shape == (wc.SIZE, wc.SIZE) and m[1] == wc.RES for m in case.maps)
    wc.check(case, reference_run(index))


def test_every_named_branch_is_taken_somewhere():
    seen = set()
    for k, case in enumerate(CASES):
        seen |= wc.branches(case, reference_run(k))
    want = {"hit at stage 0", "hit at the last stage", "hit in the middle", "release", "latched stop without a hit", "reset", "moves",
            "skipped", "un-shifted warm start"} | {"clamp %s axis %d" % (s, a) for s in ("above", "below") for a in range(3)}
    assert want <= seen, sorted(want - seen)
    assert {c.n for c in CASES} >= set(wc.STAGE_COUNTS)


def test_the_wait_one_ulp_below_three_is_below():
    """The wait `one ulp below 3.0` is 2.9999999999999996; thirty additions of 0.1 overshoot 3.0 (3.0000000000000013), which is
    why the 32-call chain releases on its thirtieth call -- the reference's own sum decides, in the reference's order."""
    w = 0.0
    for _ in range(30):
        w += 0.1
    assert w == 3.0000000000000013 and wc.one_ulp_below_three() == 2.9999999999999996
    run = reference_run(CASE_IDS.index("wait_chain"))
    latched = [int(e["states"]["collision"][0]) for _, e in run]
    assert latched == [1] * 29 + [0] * 3 and run[28][1]["states"]["waiting_time"][0] == 2.9000000000000012
    assert [int(e["states"]["collision"][1]) for _, e in run] == [0] * 10 + [1] * 22


def _mirror_call(case, problems, states, warm, call):
    """One call on the C mirror, states / warm updated in place.  The mirror knows one map: a pool goes through map by map."""
    count, n = len(problems), case.n
    commands, path = np.zeros(count, dtype=abi.COMMAND_DTYPE), np.zeros((count, n, 3))
    which = case.map_of(problems)
    for k, m in enumerate(case.maps):
        rows = np.nonzero(which == k)[0]
        if not len(rows):
            continue
        st, wm = states[rows].copy(), warm[rows].copy()
        ok = None if call.success is None else call.success[rows]
        cm, _, pt = c_oracle.postprocess_batch(case.params, m, problems[rows].copy(), st, wm, call.solutions[rows].copy(), ok, want_path=True)
        states[rows], warm[rows], commands[rows], path[rows] = st, wm, cm, pt
    return commands, path


@pytest.mark.parametrize("index", range(len(CASES)), ids=CASE_IDS)
def test_mirror_wrapper_is_the_reference_bit_for_bit(index):
    case = CASES[index]
    st, wm = case.states.copy(), case.warm.copy()
    for k, (call, (problems, want)) in enumerate(zip(case.calls, reference_run(index))):
        st_in, wm_in = st.copy(), wm.copy()
        cm, path = _mirror_call(case, problems, st, wm, call)
        where = (case.name, "call %d" % k)
        assert cm["vel"].tobytes() == want["vel"].tobytes(), where + (_first(case, cm["vel"], want["vel"]),)
        assert ((cm["flags"] & KEPT_BITS) == want["flags"]).all(), where + (_first(case, cm["flags"] & KEPT_BITS, want["flags"]),)
        assert wm.tobytes() == want["warm"].tobytes(), where + (_first(case, wm, want["warm"]),)
        for f in abi.STATE_DTYPE.names:
            assert st[f].tobytes() == want["states"][f].tobytes(), where + (f, _first(case, st[f], want["states"][f]))
        assert np.abs(path - want["path"]).max() <= 1e-12
        sk = want["skipped"]
        assert st[sk].tobytes() == st_in[sk].tobytes() and wm[sk].tobytes() == wm_in[sk].tobytes() and not path[sk].any()


def _first(case, got, want):
    """The first record that differs, by name."""
    bad = [i for i in range(len(want)) if np.asarray(got[i]).tobytes() != np.asarray(want[i]).tobytes()]
    return (case.names[bad[0]], got[bad[0]], want[bad[0]]) if bad else None


# ------------------------------------------------------------------------------------------------------------ K2 alone
def assert_wrapper_outputs(where, names, vel, flags, states, warm, want, path=None, decided=None):
    """Command, state and warm start against wrapper_reference.step_batch's `want`: the exact / 1e-14 / 1e-12 split of this
    file's header.  `decided` (fused test): the records whose decision fields are compared."""
    live = ~want["skipped"]
    dec = live if decided is None else (live & decided)
    ws = want["states"]

    def name(mask):
        return where + ([names[i] for i in np.nonzero(mask)[0][:4]],)
    for f in ("collision", "waiting_time"):
        assert (states[f][dec] == ws[f][dec]).all(), name(dec & (states[f] != ws[f])) + (f,)
    for f in ("collision_footprint", "has_old_goal", "has_prev_u0"):
        assert (states[f][live] == ws[f][live]).all(), name(live & (states[f] != ws[f])) + (f,)
    assert (states["prev_u0"][live] == ws["prev_u0"][live]).all(), name(live & (states["prev_u0"] != ws["prev_u0"]).any(axis=1))
    assert np.array_equal(states["old_goal"][live], ws["old_goal"][live], equal_nan=True), where
    got_bits = flags & KEPT_BITS
    stop = abi.FLAG_STOPPED
    assert ((got_bits & ~stop) == (want["flags"] & ~stop)).all(), name((got_bits & ~stop) != (want["flags"] & ~stop))
    assert ((got_bits & stop)[dec] == (want["flags"] & stop)[dec]).all(), name(dec & ((got_bits & stop) != (want["flags"] & stop)))
    stopped = dec & ((want["flags"] & stop) != 0)
    assert (vel[stopped] == 0.0).all() and (states["last_control"][stopped] == 0.0).all(), name(stopped & (vel != 0.0).any(axis=1))
    assert np.abs(vel[dec] - want["vel"][dec]).max(initial=0.0) <= 1e-14, name(dec & (np.abs(vel - want["vel"]).max(axis=1) > 1e-14))
    dl = np.abs(states["last_control"] - ws["last_control"]).max(axis=1)
    assert dl[dec].max(initial=0.0) <= 1e-14, name(dec & (dl > 1e-14))
    dw = np.abs(warm - want["warm"]).max(axis=1)
    assert dw[live].max(initial=0.0) <= 1e-14, name(live & (dw > 1e-14))
    if path is not None:
        dp = np.abs(path - want["path"]).reshape(len(path), -1).max(axis=1)
        assert dp.max(initial=0.0) <= 1e-12, name(dp > 1e-12)


class _Arena:
    """Page-locked host arrays: one page-aligned block, registered once (small arrays of their own would share pages)."""

    def __init__(self, lib, nbytes):
        self.lib = lib
        self.raw = np.zeros(nbytes + 8192, dtype=np.uint8)
        self.base = (-self.raw.ctypes.data) % 4096
        self.size = (nbytes + 4095) // 4096 * 4096
        self.used = 0
        assert lib.neo_mpc_pin_host_memory(C.c_void_p(self.raw.ctypes.data + self.base), self.size) == 0, lib.neo_mpc_last_error()

    def like(self, a):
        a = np.ascontiguousarray(a)
        off = self.base + self.used
        self.used += (a.nbytes + 255) // 256 * 256
        assert self.used <= self.size
        out = self.raw[off:off + a.nbytes].view(a.dtype).reshape(a.shape)
        out[...] = a
        return out

    def release(self):
        assert self.lib.neo_mpc_unpin_host_memory(C.c_void_p(self.raw.ctypes.data + self.base)) == 0


def _solver_for(case):
    from neo_mpc_planner2_amd import solver
    s = solver.BatchSolver(case.params)
    if case.pooled:
        s.set_costmap_pool(np.stack([m[0] for m in case.maps]), wc.RES, np.array([[m[2], m[3]] for m in case.maps]))
    else:
        s.set_costmap(*case.maps[0])
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("page_locked", [False, True], ids=["pageable", "page-locked"])
@pytest.mark.parametrize("index", range(len(CASES)), ids=CASE_IDS)
def test_postprocess_kernel_at_the_wrappers_edges(index, page_locked):
    """k_postprocess on every case; a case's calls are made in a row on the kernel's OWN state and warm start."""
    from neo_mpc_planner2_amd import _lib
    case, n = CASES[index], CASES[index].n
    count = len(case.problems)
    st, wm = case.states.copy(), case.warm.copy()
    arena = None
    with _solver_for(case) as s:
        try:
            if page_locked:
                lib = _lib.load()
                arena = _Arena(lib, 4096 + count * (256 + 128 + 48 + 4 * 24 * n + 256 * 8))
                st, wm = arena.like(st), arena.like(wm)
                p_prob, p_cmd = arena.like(case.problems), arena.like(np.zeros(count, dtype=abi.COMMAND_DTYPE))
                p_sol, p_path = arena.like(np.zeros((count, 3 * n))), arena.like(np.zeros((count, n, 3)))
            for k, (call, (problems, want)) in enumerate(zip(case.calls, reference_run(index))):
                st_in, wm_in = st.copy(), wm.copy()
                if page_locked:
                    p_prob[...], p_sol[...], p_cmd[...], p_path[...] = problems, call.solutions, np.zeros(1, dtype=abi.COMMAND_DTYPE), 7.0
                    b = abi.batch_struct(p_prob, st, wm, p_cmd, p_sol, p_path if case.want_path else None)
                    ok = None if call.success is None else C.c_void_p(call.success.ctypes.data)
                    _lib.check(lib.neo_mpc_postprocess_batch(s._handle, C.byref(b), ok))
                    cm, path, sol = p_cmd.copy(), (p_path.copy() if case.want_path else None), p_sol
                else:
                    sol = call.solutions.copy()
                    out = s.postprocess(problems, st, wm, sol, call.success, want_path=case.want_path)
                    cm, path = out if case.want_path else (out, None)
                where = (case.name, "call %d" % k)
                assert_wrapper_outputs(where, case.names, cm["vel"], cm["flags"], st, wm, want, path)
                # skipped rows: state and warm start byte for byte, a zero command with the flag alone, a zero path row; and
                # the injected solution comes back as it went in, skipped or not
                sk = want["skipped"]
                zero = np.zeros(1, dtype=abi.COMMAND_DTYPE)
                zero["flags"] = abi.FLAG_SKIPPED
                assert st[sk].tobytes() == st_in[sk].tobytes() and wm[sk].tobytes() == wm_in[sk].tobytes(), where
                assert cm[sk].tobytes() == zero.tobytes() * int(sk.sum()), where
                assert path is None or not path[sk].any(), where
                assert sol.tobytes() == call.solutions.tobytes(), where
                assert (cm["status"][~sk] == (0 if call.success is None else 1 - call.success[~sk])).all(), where
        finally:
            if arena is not None:
                arena.release()


# ------------------------------------------------------------------------------------------------------------ fused K2
def check_fused_wrapper(solve, n, method, in_place=None, may_leave_out=wc.FUSED_COUNT // 100):
    """`solve(params, cmap, problems, states, warm) -> (commands, solution)`, states / warm updated in place: once as is, once
    with max_iterations = 1 (most searches end un-converged: the un-shifted hand-back).  Whatever the search answered, the
    command, the state and the warm start are the reference wrapper's at THAT solution with ok = (status == 0)."""
    for cap in (None, 1):
        params, cmap, probs, st0, warm0 = wc.fused_batch(n, method, cap)
        st, warm = st0.copy(), warm0.copy()
        cm, x = solve(params, cmap, probs, st, warm)
        assert np.isfinite(x).all()
        ok = cm["status"] == 0
        want = ref.step_batch(params, [orc.Costmap(*cmap)], np.zeros(len(probs), dtype=int), probs, st0, warm0, x, ok)
        # a stage the reference puts within 1e-9 m of a cell edge decides nothing here (the mirror's own solutions have none)
        decided = want["edge_distance"].min(axis=1) >= wc.MARGIN
        assert (~decided).sum() <= may_leave_out, (~decided).sum()
        where = ("control_steps %d method %d max_iterations %s" % (n, method, cap),)
        names = ["robot %d" % i for i in range(len(probs))]
        assert_wrapper_outputs(where, names, cm["vel"], cm["flags"], st, warm, want, decided=decided)
        # teeth
        recs = want["records"]
        fresh = sum(1 for i, r in enumerate(recs) if decided[i] and r["hit_stage"] >= 0 and not st0["collision"][i])
        assert fresh >= 1 and sum(r["released"] for r in recs) >= 1 and sum(r["reset"] for r in recs) >= 1, where
        if cap == 1:
            assert (~ok).sum() >= 1 and (st["has_prev_u0"][~ok] == 0).all(), where
        print("fused K2 %s: %d fresh hits, %d releases, %d resets, %d un-shifted, %d left out"
              % (where[0], fresh, sum(r["released"] for r in recs), sum(r["reset"] for r in recs), (~ok).sum(), (~decided).sum()))
        if cap is None and in_place is not None:
            in_place(params, cmap, probs, st0, warm0, cm, x, st, warm)


@pytest.mark.parametrize("n,method", wc.FUSED_ROWS)
def test_fused_wrapper_behind_the_mirrors_solve(n, method):
    def solve(params, cmap, probs, st, warm):
        cm, x, _ = c_oracle.solve_batch(params, cmap, probs, st, warm)
        return cm, x
    check_fused_wrapper(solve, n, method, may_leave_out=0)      # (none of the mirror's solutions comes that close to an edge)


@pytest.mark.gpu
@pytest.mark.parametrize("n,method", wc.FUSED_ROWS)
def test_fused_wrapper_behind_every_row_of_the_dispatch_table(n, method):
    """solve_finish behind each search kernel: K2 reads its state, the true yaw and the footprint cost out of LDS the searches
    carve up differently per row.  (3, AUTO) once more on page-locked arrays worked on in place: bit for bit the same."""
    from neo_mpc_planner2_amd import _lib, solver
    lib = _lib.load()

    def solve(params, cmap, probs, st, warm):
        with solver.BatchSolver(params) as s:
            s.set_costmap(*cmap)
            return s.solve(probs, st, warm)

    def in_place(params, cmap, probs, st0, warm0, cm, x, st, warm):
        count = len(probs)
        arena = _Arena(lib, 4096 + count * (256 + 128 + 48 + 2 * 24 * n + 256 * 6))
        try:
            arrays = [arena.like(a) for a in (probs, st0, warm0, np.zeros(count, dtype=abi.COMMAND_DTYPE), np.zeros((count, 3 * n)))]
            with solver.BatchSolver(params) as s:
                s.set_costmap(*cmap)
                b = abi.batch_struct(*arrays)
                _lib.check(lib.neo_mpc_solve_batch(s._handle, C.byref(b)))
            assert arrays[3].tobytes() == cm.tobytes() and arrays[4].tobytes() == x.tobytes()
            assert arrays[1].tobytes() == st.tobytes() and arrays[2].tobytes() == warm.tobytes()
        finally:
            arena.release()
    check_fused_wrapper(solve, n, method, in_place if (n, method) == (3, 0) else None)
