"""Carrot (look-ahead) selection -- SURVEY §8f row 2: the step before the solver
(src/NeoMpcPlanner.cpp:83-104 plan pruning, 157-171 look-ahead distance, 173-189 look-ahead
point, 221-232 slow_down_ state machine).  The C++ plugin cannot be built here (nav2/tf2 absent),
so the oracle restatement (oracle/mpc_oracle.c part 3) is checked against an independent,
literal NumPy transcription of those lines (tests/carrot_reference.py), and the HIP kernel against the oracle and,
on the constructed edge cases further down, against the transcription itself."""
import math

import numpy as np
import pytest

from neo_mpc_planner2_amd import abi, synthetic
from oracle import c_oracle
from tests import carrot_reference as cref
from tests.carrot_reference import transcription
from tests.fleet_kit import gpu

LP = dict(lookahead_dist_min=0.4, lookahead_dist_max=0.8, lookahead_dist_close_to_goal=0.3,
          max_transform_dist=5.0)


def _inputs(count, seed):
    poses, offsets, robots = synthetic.make_plans(count, seed=seed, min_len=8, max_len=300)
    rng = np.random.default_rng(seed + 1)
    slow = rng.integers(0, 2, size=count).astype(np.int32)
    fcost = rng.choice([0.0, 150.0, 201.0, 253.0, 255.0], size=count)
    return poses, offsets, robots, slow, fcost


def test_oracle_restatement_matches_literal_transcription():
    poses, offsets, robots, slow, fcost = _inputs(300, seed=5)
    # edge cases: robot far from everything (status 2), robot at the goal (closer_to_goal)
    robots[0, :2] += 100.0
    robots[1, :2] = poses[offsets[2] - 1, :2]
    slow_in = slow.copy()
    car = c_oracle.select_carrots(poses, offsets, robots, slow, fcost, **LP)
    assert car["status"][0] == 2 and car["closer_to_goal"][1] == 1
    for i in range(len(robots)):
        t = transcription(poses[offsets[i]:offsets[i + 1]], robots[i], slow_in[i], fcost[i], LP)
        assert car["status"][i] == t["status"]
        if t["status"] in (1, 2):
            continue
        assert (car["begin"][i], car["end"][i]) == (t["begin"], t["end"])
        assert bool(car["closer_to_goal"][i]) == t["closer"] and car["lookahead_dist"][i] == t["la"]
        assert np.allclose(car["xy"][i], t["xy"], rtol=0, atol=1e-12)
        yaw = math.atan2(2 * car["q"][i][3] * car["q"][i][2], 1 - 2 * car["q"][i][2] ** 2)
        assert abs(yaw - t["yaw"]) <= 1e-12
        assert car["slow_down"][i] == t["slow"] == slow[i]


def test_oracle_empty_plan_and_problem_write():
    poses, offsets, robots, slow, fcost = _inputs(4, seed=9)
    offsets2 = np.concatenate([offsets[:2], offsets[1:]]).astype(np.uint32)   # robot 1 gets an empty plan
    robots2 = np.concatenate([robots[:1], robots[:1], robots[1:]])
    slow2 = np.ones(5, dtype=np.int32)
    probs = synthetic.make_problems(5, 200, seed=1)
    before = probs["carrot_xy"].copy()
    car = c_oracle.select_carrots(poses, offsets2, robots2, slow2, None, problems=probs, **LP)
    assert car["status"][1] == 1 and (probs["carrot_xy"][1] == before[1]).all()
    ok = car["status"] == 0
    assert (probs["carrot_xy"][ok] == car["xy"][ok]).all() and (probs["carrot_q"][ok] == car["q"][ok]).all()
    # every throw in front of the service call (cpp:70, 131, 235) means "no request this tick": the record says so
    assert (probs["skip"] == (car["status"] != 0)).all() and (probs["switch_opt"][ok] == car["closer_to_goal"][ok]).all()


def test_footprint_cost_255_makes_no_request():
    """cpp:234-236: a footprint cost of 255 throws AFTER the slow_down_ update and BEFORE the optimizer request: carrot
    status 3, the request record is marked `skip`, and the solver (here: the CPU mirror) leaves that robot's state, warm
    start and command alone."""
    from oracle import mpc_oracle as orc
    poses, offsets, robots, slow, fcost = _inputs(64, seed=31)
    fcost[::4] = 255.0
    probs = synthetic.make_problems(64, 500, seed=4)
    car = c_oracle.select_carrots(poses, offsets, robots, slow, fcost, problems=probs, **LP)
    thrown = fcost == 255.0
    assert ((car["status"] == 3) == (thrown & (car["status"] != 2) & (car["status"] != 1))).all() and (car["status"] == 3).any()
    assert (probs["skip"] == (car["status"] != 0)).all()
    cmap = synthetic.make_costmap(500, seed=0)
    st, warm = synthetic.make_states(probs, 3)
    warm[:] = 0.01
    st0, warm0 = st.copy(), warm.copy()
    cm, _, _ = c_oracle.solve_batch(orc.make_params(), cmap, probs, st, warm)
    sk = probs["skip"] != 0
    assert (cm["flags"][sk] == abi.FLAG_SKIPPED).all() and ((cm["flags"][~sk] & abi.FLAG_SKIPPED) == 0).all()
    assert st[sk].tobytes() == st0[sk].tobytes() and (warm[sk] == warm0[sk]).all() and (cm["vel"][sk] == 0.0).all()
    assert (cm["iterations"][sk] == 0).all() and (cm["cost"][sk] == 0.0).all()
    assert st[~sk].tobytes() != st0[~sk].tobytes()


@pytest.mark.gpu
def test_carrot_kernel_matches_oracle():
    from neo_mpc_planner2_amd.solver import BatchSolver
    poses, offsets, robots, slow, fcost = _inputs(4096, seed=11)
    robots[0, :2] += 100.0
    slow_g, slow_c = slow.copy(), slow.copy()
    pg = synthetic.make_problems(4096, 200, seed=2)
    pc = pg.copy()
    want = c_oracle.select_carrots(poses, offsets, robots, slow_c, fcost, problems=pc, **LP)
    with BatchSolver({}) as s:
        got = s.select_carrots(poses, offsets, robots, slow_g, fcost, problems=pg, **LP)
    for f in ("begin", "end", "closer_to_goal", "slow_down", "status", "lookahead_dist"):
        assert (got[f] == want[f]).all(), f
    assert (slow_g == slow_c).all()
    assert np.allclose(got["xy"], want["xy"], rtol=0, atol=1e-12)
    assert np.allclose(got["q"], want["q"], rtol=0, atol=1e-12)
    assert np.allclose(pg["carrot_xy"], pc["carrot_xy"], rtol=0, atol=1e-12)
    assert np.allclose(pg["carrot_q"], pc["carrot_q"], rtol=0, atol=1e-12)
    assert (got["status"] == 0).sum() >= 3000 and (got["status"] == 3).sum() >= 500
    assert (pg["skip"] == pc["skip"]).all() and (pg["switch_opt"] == pc["switch_opt"]).all() and (pg["skip"] != 0).sum() >= 500


@pytest.mark.gpu
def test_carrots_feed_the_solver_on_device():
    """device-resident chain K4 -> K1: carrots are written straight into the request records."""
    import torch
    from neo_mpc_planner2_amd.solver import BatchSolver, DeviceBatch
    from oracle import mpc_oracle as orc
    count = 1024
    poses, offsets, robots, slow, fcost = _inputs(count, seed=21)
    cmap = synthetic.make_costmap(500, seed=0)
    probs = synthetic.make_problems(count, 500, seed=3)
    st, warm = synthetic.make_states(probs, 3)
    # reference chain on the host: oracle carrots, then the GPU solver through host buffers
    pc, sc = probs.copy(), slow.copy()
    c_oracle.select_carrots(poses, offsets, robots, sc, fcost, problems=pc, **LP)
    with BatchSolver(orc.make_params()) as s:
        s.set_costmap(*cmap)
        want, _ = s.solve(pc, st.copy(), warm.copy())
        dev = "cuda:0"
        db = DeviceBatch(probs, st, warm, dev)
        d_poses, d_off, d_rob, d_slow, d_fc = gpu(poses), gpu(offsets.view(np.int32)), gpu(robots), gpu(slow), gpu(fcost)
        d_car = torch.zeros((count, abi.CARROT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        lp = abi.NeoMpcLookaheadParams(LP["lookahead_dist_min"], LP["lookahead_dist_max"],
                                       LP["lookahead_dist_close_to_goal"], LP["max_transform_dist"])
        s.select_carrots_device(lp, d_poses, d_off, d_rob, d_slow, d_car, d_fc, problems=db.problems)
        s.solve_device(db.problems, db.states, db.warm, db.commands)
        torch.cuda.synchronize()
        got = db.commands_host()
    dv = np.abs(got["vel"] - want["vel"]).max(axis=1)
    # the carrots agree to an ulp; the Newton path's finite-difference Hessian amplifies that a little
    assert (dv <= 1e-6).mean() >= 0.98 and (dv <= 1e-3).mean() >= 0.995


@pytest.mark.gpu
def test_skipped_instances_are_left_alone_by_the_solver():
    """neo_mpc_problem.skip (set by K4 with carrot status 3, cpp:234-236): K1 and K2 leave the robot's state record and warm
    start alone and answer zero twist + NEO_MPC_FLAG_SKIPPED (zero rows in the optional outputs) -- on the staged path, the
    small latency path and the in-place (page-locked) path; the other instances come out exactly as without any skip."""
    import ctypes as C
    from neo_mpc_planner2_amd import _lib
    from neo_mpc_planner2_amd.solver import BatchSolver
    from oracle import mpc_oracle as orc
    lib = _lib.load()
    cmap = synthetic.make_costmap(500, seed=0)
    for count in (48, 700):                      # latency path / staged path
        probs = synthetic.make_problems(count, 500, seed=6)
        st0, warm0 = synthetic.make_states(probs, 3)
        warm0[:] = 0.02
        with BatchSolver(orc.make_params()) as s:
            s.set_costmap(*cmap)
            st_a, warm_a = st0.copy(), warm0.copy()
            ref, xref = s.solve(probs, st_a, warm_a)
            sk = np.zeros(count, dtype=bool)
            sk[::3] = True
            p2 = probs.copy()
            p2["skip"] = sk
            st_b, warm_b = st0.copy(), warm0.copy()
            cmds = np.zeros(count, dtype=abi.COMMAND_DTYPE)
            cmds["vel"] = 7.0
            sol = np.full((count, 9), 5.0)
            s.solve(p2, st_b, warm_b, out=(cmds, sol))
            assert (cmds["flags"][sk] == abi.FLAG_SKIPPED).all() and (cmds["vel"][sk] == 0.0).all() and (sol[sk] == 0.0).all()
            assert (cmds["iterations"][sk] == 0).all() and (cmds["status"][sk] == 0).all() and (cmds["cost"][sk] == 0.0).all()
            assert st_b[sk].tobytes() == st0[sk].tobytes() and (warm_b[sk] == warm0[sk]).all()
            assert cmds[~sk].tobytes() == ref[~sk].tobytes() and (sol[~sk] == xref[~sk]).all()
            assert st_b[~sk].tobytes() == st_a[~sk].tobytes() and (warm_b[~sk] == warm_a[~sk]).all()
            # K2 alone
            st_c, warm_c = st0.copy(), warm0.copy()
            c2 = s.postprocess(p2, st_c, warm_c, xref)
            assert (c2["flags"][sk] == abi.FLAG_SKIPPED).all() and st_c[sk].tobytes() == st0[sk].tobytes()
            if count > 64:   # in place on page-locked arrays
                arrays = [np.ascontiguousarray(p2).copy(), st0.copy(), warm0.copy(), cmds.copy(), sol.copy()]
                arrays[3]["vel"] = 7.0
                arrays[3]["flags"] = 0
                arrays[4][:] = 5.0
                for a in arrays:
                    assert lib.neo_mpc_pin_host_memory(C.c_void_p(a.ctypes.data), a.nbytes) == 0
                try:
                    b = abi.batch_struct(*arrays)
                    _lib.check(lib.neo_mpc_solve_batch(s._handle, C.byref(b)))
                    assert arrays[3].tobytes() == cmds.tobytes() and (arrays[4] == sol).all()
                    assert arrays[1].tobytes() == st_b.tobytes() and (arrays[2] == warm_b).all()
                finally:
                    for a in arrays:
                        assert lib.neo_mpc_unpin_host_memory(C.c_void_p(a.ctypes.data)) == 0


@pytest.mark.gpu
def test_skip_fields_other_than_0_or_1_are_refused_on_host_batches():
    """neo_mpc_problem.skip was reserved[0] in ABI 1 and that header never asked for zeroed reserved bytes: garbage there
    must not take robots out of a tick silently.  Host batches are scanned (NEO_MPC_ERR_INVALID_ARGUMENT, nothing
    touched); the device entry points act on skip == 1 alone -- any other value is solved like 0."""
    import torch
    from neo_mpc_planner2_amd import _lib
    from neo_mpc_planner2_amd.solver import BatchSolver, DeviceBatch
    from oracle import mpc_oracle as orc
    cmap = synthetic.make_costmap(500, seed=0)
    probs = synthetic.make_problems(96, 500, seed=8)
    st0, warm0 = synthetic.make_states(probs, 3)
    with BatchSolver(orc.make_params()) as s:
        s.set_costmap(*cmap)
        ref, xref = s.solve(probs, st0.copy(), warm0.copy())
        bad = probs.copy()
        bad["skip"][5] = 0x3f800000          # (what an uninitialised float 1.0 looks like in the old reserved slot)
        st, warm = st0.copy(), warm0.copy()
        with pytest.raises(_lib.NeoMpcError) as err:
            s.solve(bad, st, warm)
        assert err.value.code == -1 and "skip" in str(err.value)      # NEO_MPC_ERR_INVALID_ARGUMENT
        assert st.tobytes() == st0.tobytes() and (warm == warm0).all()
        # device batch: the value is not 1, so the robot is solved
        db = DeviceBatch(bad, st0.copy(), warm0.copy(), "cuda:0")
        s.solve_device(db.problems, db.states, db.warm, db.commands, db.solution)
        torch.cuda.synchronize()
        got = db.commands_host()
        assert (got["flags"] & abi.FLAG_SKIPPED == 0).all() and got.tobytes() == ref.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# K4 at its edges: constructed batches with exact arithmetic (tests/carrot_reference.py), non-finite inputs, the largest
# shapes and a wide random batch -- the transcription is the reference, the oracle has to agree with it on the CPU and
# the kernel on the GPU, through both entry points.
INT_FIELDS = ("begin", "end", "closer_to_goal", "slow_down", "status", "reserved")
PROBLEM_WRITES = ("carrot_xy", "carrot_q", "switch_opt", "skip")
Q_ATOL = 1e-12          # the project's tolerance for what goes through sincos


def _bits(got, want):
    """Bit for bit; a NaN matches a NaN (its sign and payload are nobody's contract)."""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    return bool(((got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))).all())


def _close(got, want, atol):
    """|got - want| <= atol where `want` is finite, the same NaN / infinity pattern elsewhere."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    fin = np.isfinite(want)
    return bool((np.abs(got[fin] - want[fin]) <= atol).all()) and _bits(got[~fin], want[~fin])


def _assert_carrots(got, want, exact):
    for f in INT_FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert len(bad) == 0, (f, bad[:5], got[f][bad[:5]], want[f][bad[:5]])
    assert _bits(got["lookahead_dist"], want["lookahead_dist"])
    assert _bits(got["xy"], want["xy"]) if exact else _close(got["xy"], want["xy"], 1e-12)
    assert _close(got["q"], want["q"], Q_ATOL) and _bits(got["q"][:, :2], want["q"][:, :2])


def _assert_problems(got, want, status, exact):
    """The request records: the four fields K4 owns against the reference's, every other byte unchanged (the reference
    started from the same byte pattern), rows that make no carrot (status 1, 2) unchanged apart from `skip`."""
    assert (got["skip"] == want["skip"]).all() and (got["switch_opt"] == want["switch_opt"]).all()
    assert _bits(got["carrot_xy"], want["carrot_xy"]) if exact else _close(got["carrot_xy"], want["carrot_xy"], 1e-12)
    assert _close(got["carrot_q"], want["carrot_q"], Q_ATOL)
    made = (status == 0) | (status == 3)
    assert (got["carrot_q"][made, :2] == 0.0).all() and not np.signbit(got["carrot_q"][made, :2]).any()
    assert got[~made].tobytes() == want[~made].tobytes()
    rest = got.copy()
    for f in PROBLEM_WRITES:
        rest[f] = want[f]
    assert rest.tobytes() == want.tobytes()


_REFERENCES = {}


def _reference(key, batch, fcost=True, problems=True):
    """(carrots, picks, slow_down after, problems after) of the transcription: computed once, never written again."""
    key = (key, fcost, problems)
    if key not in _REFERENCES:
        slow = batch["slow"].copy()
        probs = cref.fill_problems(len(slow)) if problems else None
        car, picks = cref.select_carrots(batch["poses"], batch["offsets"], batch["robots"], slow,
                                         batch["fcost"] if fcost else None, probs, batch["lp"])
        for a in (car, picks, slow, probs):
            if a is not None:
                a.flags.writeable = False
        _REFERENCES[key] = (car, picks, slow, probs)
    return _REFERENCES[key]


def _check(run, key, batch, exact, fcost=True, problems=True):
    """`run(batch, fcost, problems)` -> (carrots, slow_down, problems) against the reference."""
    want, _, want_slow, want_probs = _reference(key, batch, fcost, problems)
    got, slow, probs = run(batch, fcost, problems)
    _assert_carrots(got, want, exact)
    assert (slow == want_slow).all()
    if problems:
        _assert_problems(probs, want_probs, want["status"], exact)
    return got


def _run_oracle(batch, fcost=True, problems=True):
    slow = batch["slow"].copy()
    probs = cref.fill_problems(len(slow)) if problems else None
    got = c_oracle.select_carrots(batch["poses"], batch["offsets"], batch["robots"], slow,
                                  batch["fcost"] if fcost else None, problems=probs, **batch["lp"])
    return got, slow, probs


def _lengths(batch):
    return np.diff(batch["offsets"].astype(np.int64))


def _front(batch):
    """Distance of every pose of a constructed batch from its robot, exact: |x - ROBOT_X| on the line."""
    return np.abs(batch["poses"][:, 0] - cref.ROBOT_X)


CONSTRUCTED = ("lengths", "ties", "scan_wide", "scan_tight", "equality", "slow", "empty", "all_empty", "one")


def test_constructed_batches_names():
    assert tuple(cref.constructed()) == CONSTRUCTED


@pytest.mark.parametrize("name", CONSTRUCTED)
def test_oracle_matches_transcription_on_constructed_cases(name):
    _check(_run_oracle, name, cref.constructed()[name], exact=True)
    if name in ("slow", "empty"):
        for fcost, problems in ((True, False), (False, True), (False, False)):
            _check(_run_oracle, name, cref.constructed()[name], exact=True, fcost=fcost, problems=problems)


def test_constructed_lengths_cover_every_loop_of_the_search():
    """Every listed plan length crossed with every listed closest index inside it, pick offset 1, no cut -- counted on the
    reference's output."""
    batch = cref.constructed()["lengths"]
    car, picks, _, _ = _reference("lengths", batch)
    n = _lengths(batch)
    have = set(zip(n.tolist(), car["begin"].tolist()))
    need = {(L, b) for L in cref.LENGTHS for b in cref.BEGINS + (L - 2, L - 1) if 0 <= b < L}
    assert have == need and len(car) == len(need) and set(n.tolist()) == set(cref.LENGTHS)
    assert (car["status"] == 0).all() and (car["end"] == n).all()
    assert (picks == np.minimum(car["begin"] + 1, n - 1)).all()
    # the minimum in each of the four unrolled candidates of the first and of the second trip, and in the remainder loop
    unrolled = lambda L, b: (b // 256) * 256 + 192 + b % 64 < L
    for trip in (0, 1):
        assert {(b % 256) // 64 for L, b in have if b // 256 == trip and unrolled(L, b)} == {0, 1, 2, 3}
    assert sum(1 for L, b in have if not unrolled(L, b)) >= 50


def test_constructed_ties_repeat_the_closest_pose():
    batch = cref.constructed()["ties"]
    car, _, _, _ = _reference("ties", batch)
    gaps, copies = set(), set()
    for i, (length, ties) in enumerate(cref.TIES):
        plan = batch["poses"][batch["offsets"][i]:batch["offsets"][i + 1]]
        same = np.nonzero((plan == plan[car["begin"][i]]).all(axis=1))[0]
        d = _front(batch)[batch["offsets"][i]:batch["offsets"][i + 1]]
        assert len(plan) == length and same.tolist() == list(ties)
        assert len(same) == length or d[same].max() < np.delete(d, same).min()
        assert car["begin"][i] == same[0] == ties[0] and car["status"][i] == 0
        gaps.update((int(b - a), int(a % 64 < b % 64)) for a, b in zip(same[:-1], same[1:]))
        copies.add(len(same) if len(same) < length else "all")
    # one lane 64 apart, one lane two trips apart, neighbouring lanes, the later copy in a lower lane
    assert {(64, 0), (256, 0), (1, 1)} <= gaps and any(up == 0 and g % 64 for g, up in gaps)
    assert {2, 3, "all"} <= copies and max(c for c in copies if c != "all") >= 50
    assert sum(1 for length, ties in cref.TIES if len(ties) == length and length > 1) >= 4


@pytest.mark.parametrize("name", ("scan_wide", "scan_tight"))
def test_constructed_scans_place_pick_and_end_where_their_tags_say(name):
    """Tag (b, p, e): pose b+p is the first at least a look-ahead away, pose b+e the first beyond the cut-off -- checked
    on the inputs with the reference's look-ahead distance, and the reference's begin / pick / end follow from them."""
    batch = cref.constructed()[name]
    car, picks, _, _ = _reference(name, batch)
    d, n, lp = _front(batch), _lengths(batch), batch["lp"]
    for i, (b, p, e) in enumerate(batch["tags"]):
        o = int(batch["offsets"][i])
        assert car["begin"][i] == b
        far = np.nonzero(d[o + b:o + n[i]] > lp["max_transform_dist"])[0]
        assert (far[0] == e) if e is not None else len(far) == 0
        end = b + e if e is not None else n[i]
        assert car["end"][i] == end
        if e == 0:
            assert car["status"][i] == 2 and car["lookahead_dist"][i] == 0.0 and picks[i] == -1
            assert car["closer_to_goal"][i] == (name == "scan_tight")
            continue
        hit = np.nonzero(d[o + b:o + n[i]] >= car["lookahead_dist"][i])[0]
        assert (hit[0] == p) if p is not None else len(hit) == 0
        assert car["status"][i] == 0 and picks[i] == (b + p if p is not None and b + p < end else end - 1)
    tags = set(batch["tags"])
    if name == "scan_wide":
        assert tags == {(b, p, e) for b in cref.SCAN_BEGINS for p, e in cref.SCAN_WIDE + [(None, 0)]}
        same = lambda p, e: p // 64 == e // 64
        pe = [(p, e) for p, e in cref.SCAN_WIDE if p is not None and e is not None]
        assert {p for p, e in cref.SCAN_WIDE if e is None} == {0, 1, 63, 64, 65, 130, None}
        assert any(p < e and same(p, e) for p, e in pe) and any(p < e - 1 and not same(p, e) for p, e in pe)
        assert sum(p == e for p, e in pe) >= 3 and any(e == p + 1 and not same(p, e) for p, e in pe)
        assert (1, 1) in cref.SCAN_WIDE and (0, 1) in cref.SCAN_WIDE
    else:
        assert tags == {(b, p, e) for b in cref.SCAN_BEGINS for e, p in cref.SCAN_TIGHT + [(0, None)]}
        ep = [(e, p) for e, p in cref.SCAN_TIGHT if p is not None]
        assert any(e // 64 == p // 64 and e < p for e, p in ep) and any(e // 64 + 1 == p // 64 for e, p in ep)
        assert sum(p is None for e, p in cref.SCAN_TIGHT) >= 2


def test_constructed_equalities_and_lookahead_table():
    batch = cref.constructed()["equality"]
    car, picks, _, _ = _reference("equality", batch)
    d, lp = _front(batch), batch["lp"]
    table = set()
    for i, (_, sd, closer) in enumerate(batch["tags"]):
        assert batch["slow"][i] == sd and car["closer_to_goal"][i] == closer and car["status"][i] == 0
        table.add((sd, closer, float(car["lookahead_dist"][i])))
    assert table == {(0, 0, lp["lookahead_dist_max"]), (1, 0, lp["lookahead_dist_min"]),
                     (0, 1, lp["lookahead_dist_close_to_goal"]), (1, 1, lp["lookahead_dist_close_to_goal"])}
    assert len({lp["lookahead_dist_max"], lp["lookahead_dist_min"], lp["lookahead_dist_close_to_goal"]}) == 3
    for g in (0, 3):
        o = batch["offsets"][g:g + 3].astype(np.int64)
        # the picked pose is exactly a look-ahead away, the one before it is not; the last kept pose exactly at the cut-off
        assert d[o[0] + picks[g]] == car["lookahead_dist"][g] and d[o[0] + picks[g] - 1] < car["lookahead_dist"][g]
        assert d[o[0] + car["end"][g] - 1] == lp["max_transform_dist"] and car["end"][g] < _lengths(batch)[g]
        # the goal one grid step beyond close_to_goal: not closer; exactly at it: closer, whatever slow_down was
        assert d[o[2] - 1] == lp["lookahead_dist_close_to_goal"] + cref.EPS and not car["closer_to_goal"][g + 1]
        assert d[o[2] + _lengths(batch)[g + 2] - 1] == lp["lookahead_dist_close_to_goal"] and car["closer_to_goal"][g + 2]
        assert d[o[2] + picks[g + 2]] == lp["lookahead_dist_close_to_goal"] and picks[g + 2] < _lengths(batch)[g + 2] - 1


def test_constructed_slow_down_and_throw():
    batch = cref.constructed()["slow"]
    car, _, slow, _ = _reference("slow", batch)
    cost = np.array([t[0] for t in batch["tags"]])
    yaw = np.array([t[1] for t in batch["tags"]])
    wrapped = np.abs(np.arctan2(np.sin(yaw), np.cos(yaw)))
    assert (np.abs(wrapped - 1.0) >= 1e-6).all() and set(cost.tolist()) == set(cref.COSTS) and 200.0 < cref.COSTS[2] < 200.1
    assert {2.0 * math.pi - 0.5, -(2.0 * math.pi - 0.5), math.pi + 0.2, -(math.pi + 0.2)} <= set(yaw.tolist())
    assert ((wrapped < 1.0) & (np.abs(yaw) > 1.0)).any() and ((wrapped > 1.0) & (np.abs(yaw) > math.pi)).any()
    want = ((wrapped >= 1.0) & (cost > 200.0)).astype(np.int32)
    assert (car["slow_down"] == want).all() and (slow == want).all()
    assert ((car["status"] == 3) == (cost == 255.0)).all() and set(car["status"].tolist()) == {0, 3}
    thrown = car["status"] == 3
    assert ((slow != batch["slow"]) & thrown & (slow == 1)).any() and ((slow != batch["slow"]) & thrown & (slow == 0)).any()
    # without footprint costs: no slow-down, no throw
    car0, _, slow0, _ = _reference("slow", batch, fcost=False)
    assert (car0["status"] == 0).all() and (slow0 == 0).all()


def test_constructed_empty_plans():
    batch = cref.constructed()["empty"]
    car, _, slow, probs = _reference("empty", batch)
    assert car["status"].tolist() == [1, 0, 1, 3, 1] and (_lengths(batch) == 0).tolist() == [True, False, True, False, True]
    none = cref.constructed()["all_empty"]
    car, _, slow, probs = _reference("all_empty", none)
    assert none["offsets"][-1] == 0 and len(none["poses"]) == 0 and (car["status"] == 1).all()
    assert (slow == none["slow"]).all() and (probs["skip"] == 1).all()
    assert none["poses"].ctypes.data != 0      # (an empty array still has an address: the entry points refuse a null one)
    assert len(cref.constructed()["one"]["robots"]) == 1


def test_problem_pattern_marks_skip_on_robots_that_make_a_request():
    """Record hygiene needs robots that come in with skip = 1 and go out with status 0."""
    for name in ("lengths", "scan_wide", "slow"):
        car, _, _, probs = _reference(name, cref.constructed()[name])
        before = cref.fill_problems(len(car))
        assert ((before["skip"] == 1) & (car["status"] == 0)).sum() >= 10 and (probs["skip"] == (car["status"] != 0)).all()
        assert np.isfinite(before["carrot_xy"]).all() and (before["carrot_xy"] != 0.0).all()


def test_oracle_matches_transcription_on_non_finite_inputs():
    with_bad, without, bad, keep = cref.nonfinite()
    got = _check(_run_oracle, "nonfinite", with_bad, exact=True)
    clean = _check(_run_oracle, "nonfinite_without", without, exact=True)
    want = _reference("nonfinite", with_bad)[0]
    by = dict(zip(cref.NONFINITE, bad))
    # min_by keeps the first pose where no distance compares `<`; a NaN pose further on is passed over
    for kind in ("robot_nan", "robot_inf_x", "plan_all_nan", "plan_first_nan"):
        assert want["begin"][by[kind]] == 0, kind
    assert want["begin"][by["plan_one_nan"]] == 70 and want["begin"][by["robot_nan_yaw"]] == 70
    assert want["begin"][by["plan_first_inf_nan"]] == 70          # hypot(inf, NaN) is inf: the search moves on from it
    assert want["status"][by["robot_inf_x"]] == 2 and np.isnan(want["xy"][by["robot_nan"]]).all()
    assert np.isnan(want["q"][by["robot_nan_yaw"]][2:]).all() and want["slow_down"][by["robot_nan_yaw"]] == 0
    assert (np.diff(bad) == 2).all() and bad[0] == 1 and bad[-1] == len(want) - 2      # each between two ordinary robots
    assert got[keep].tobytes() == clean.tobytes() and np.isfinite(clean["xy"]).all()


def test_oracle_matches_transcription_at_the_largest_shapes():
    long_, many = cref.sizes()
    _check(_run_oracle, "long", long_, exact=True)
    _check(_run_oracle, "many", many, exact=True)
    car = _reference("long", long_)[0]
    assert _lengths(long_).tolist() == [100000, 100000] and car["begin"].tolist() == [99997, 70001]
    car = _reference("many", many)[0]
    assert len(car) == 70000 and (_lengths(many) == 2).all() and set(car["begin"].tolist()) == {0, 1}
    assert set(car["status"].tolist()) == {0, 3}


def _made_request(car):
    return (car["status"] == 0) | (car["status"] == 3)


def _random_checks(batch, car):
    for status in (0, 1, 2, 3):
        assert (car["status"] == status).sum() >= 100, status
    made = _made_request(car)
    cut = car["end"][made] < _lengths(batch)[made]
    assert cut.mean() >= 0.25 and (~cut).mean() >= 0.25, cut.mean()
    assert (car["closer_to_goal"] == 1).sum() >= 100 and len(car) == cref.RANDOM_COUNT


def test_oracle_matches_transcription_on_the_wide_random_batch():
    batch = cref.random_batch()
    _check(_run_oracle, "random", batch, exact=False)
    car = _reference("random", batch)[0]
    _random_checks(batch, car)
    n = _lengths(batch)
    assert n.min() == 0 and n[n > 0].min() == 1 and n.max() > 1200 and (n > 448).sum() > 1000
    tags = np.array(batch["tags"])
    doubled = np.isin(tags, (2, 3)) & _made_request(car)
    assert doubled.sum() >= 200


# ---- on the GPU
@pytest.fixture(scope="module")
def k4():
    """One solver handle for the module and the two ways into K4: `run(batch, fcost, problems)` -> (carrots, slow_down,
    problems) through neo_mpc_select_carrots, and through neo_mpc_select_carrots_device on a stream of its own."""
    import torch
    from neo_mpc_planner2_amd.solver import BatchSolver

    with BatchSolver({}) as s:
        def host(batch, fcost=True, problems=True):
            slow = batch["slow"].copy()
            probs = cref.fill_problems(len(slow)) if problems else None
            got = s.select_carrots(batch["poses"], batch["offsets"], batch["robots"], slow,
                                   batch["fcost"] if fcost else None, problems=probs, **batch["lp"])
            return got, slow, probs

        def device(batch, fcost=True, problems=True):
            dev = "cuda:0"
            count = len(batch["slow"])
            poses = batch["poses"] if len(batch["poses"]) else np.zeros((1, 3))   # (a null plan_poses is refused)
            d_poses, d_off, d_rob, d_slow = gpu(poses), gpu(batch["offsets"].view(np.int32)), gpu(batch["robots"]), gpu(batch["slow"])
            d_fc = gpu(batch["fcost"]) if fcost and batch["fcost"] is not None else None
            d_probs = gpu(cref.fill_problems(count).view(np.uint8).reshape(count, -1)) if problems else None
            d_car = torch.full((count, abi.CARROT_DTYPE.itemsize), 0xEE, dtype=torch.uint8, device=dev)
            lp = abi.NeoMpcLookaheadParams(*(batch["lp"][k] for k in ("lookahead_dist_min", "lookahead_dist_max",
                                                                     "lookahead_dist_close_to_goal", "max_transform_dist")))
            stream = torch.cuda.Stream(device=dev)
            stream.wait_stream(torch.cuda.current_stream(dev))
            s.select_carrots_device(lp, d_poses, d_off, d_rob, d_slow, d_car, d_fc, problems=d_probs,
                                    stream=stream.cuda_stream)
            stream.synchronize()
            got = d_car.cpu().numpy().reshape(-1).view(abi.CARROT_DTYPE).copy()
            probs = d_probs.cpu().numpy().reshape(-1).view(abi.PROBLEM_DTYPE).copy() if problems else None
            return got, d_slow.cpu().numpy(), probs

        yield dict(host=host, device=device, solver=s)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ("host", "device"))
@pytest.mark.parametrize("name", CONSTRUCTED)
def test_carrot_kernel_matches_transcription_on_constructed_cases(k4, name, entry):
    """Integer fields, lookahead_dist and xy bit for bit, q within 1e-12, the whole record for every status, the caller's
    slow_down, and the request records byte for byte outside the four fields K4 owns."""
    _check(k4[entry], name, cref.constructed()[name], exact=True)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ("host", "device"))
@pytest.mark.parametrize("fcost,problems", ((True, False), (False, True), (False, False)))
def test_carrot_kernel_without_footprint_costs_or_problems(k4, entry, fcost, problems):
    """footprint_costs == NULL: no slow-down and no throw; problems == NULL: nothing but carrots and slow_down."""
    for name in ("slow", "empty"):
        _check(k4[entry], name, cref.constructed()[name], exact=True, fcost=fcost, problems=problems)


@pytest.mark.gpu
def test_carrot_entry_points_with_no_robot(k4):
    """count = 0 with every pointer null: both entry points answer NEO_MPC_OK (the return code is all that is observed
    here: with no pointer there is nothing a launch could have written to)."""
    import ctypes as C
    import torch
    from neo_mpc_planner2_amd import _lib
    lib = _lib.load()
    lp = abi.NeoMpcLookaheadParams(0.5, 1.0, 0.25, 4.0)
    b = abi.NeoMpcPlanBatch()          # count 0, every pointer null
    handle = k4["solver"]._handle
    assert lib.neo_mpc_select_carrots(handle, C.byref(lp), C.byref(b)) == 0
    stream = torch.cuda.Stream(device="cuda:0")
    assert lib.neo_mpc_select_carrots_device(handle, C.byref(lp), C.byref(b), C.c_void_p(stream.cuda_stream)) == 0
    stream.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ("host", "device"))
def test_carrot_kernel_on_non_finite_inputs(k4, entry):
    """A robot pose of NaN, +inf in x, a NaN yaw; a plan of NaN poses, one NaN pose among good ones, a NaN first pose, a
    first pose of (inf, NaN) whose distance is infinite and not NaN: the reference's record (`begin` = 0 where no distance compares `<`: the plugin erases the plan's head with it), and the
    robots on either side come out bit for bit as in a call without the offenders."""
    with_bad, without, bad, keep = cref.nonfinite()
    got = _check(k4[entry], "nonfinite", with_bad, exact=True)
    clean = _check(k4[entry], "nonfinite_without", without, exact=True)
    assert got[keep].tobytes() == clean.tobytes()


@pytest.mark.gpu
def test_carrot_kernel_at_the_largest_shapes(k4):
    """100 000 poses in one plan (391 trips of the unrolled search, the closest pose third from the end, and a copy of it
    earlier in the plan), and 70 000 robots (check_count allows them: its limit is 2^31 - 1)."""
    long_, many = cref.sizes()
    _check(k4["host"], "long", long_, exact=True)
    _check(k4["device"], "long", long_, exact=True)
    _check(k4["host"], "many", many, exact=True)
    _check(k4["device"], "many", many, exact=True)


@pytest.mark.gpu
def test_carrot_kernel_matches_transcription_on_the_wide_random_batch(k4):
    """Plans of 0 to 2400 poses, robots far from everything and at the goal, plans doubled back over themselves (every
    pose twice: the first of equal minima), about half of the plans cut: integer fields and lookahead_dist equal, xy and
    q within 1e-12."""
    batch = cref.random_batch()
    _random_checks(batch, _reference("random", batch)[0])
    _check(k4["host"], "random", batch, exact=False)
    _check(k4["device"], "random", batch, exact=False)
