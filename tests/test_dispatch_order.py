"""K5 (k_dispatch_order) and the arming logic of neo_mpc_balance_dispatch_device against tests/dispatch_order_reference.py,
read back through the test hook neo_mpc_get_dispatch_order.  Every comparison is exact: the averages bit for bit, the order
bin by bin as sets (the ranks inside a bin come from atomics).  Command records with made-up `iterations` stand in for a
solve's -- no costmap and no K1 -- except in the last two tests, which share the one K1 launch of this file."""
import numpy as np
import pytest

from neo_mpc_planner2_amd import abi, synthetic
from tests import dispatch_order_reference as ref
from tests import util

pytestmark = pytest.mark.gpu


@pytest.fixture
def solver():
    from neo_mpc_planner2_amd.solver import BatchSolver
    with BatchSolver(util.orc.make_params()) as s:
        yield s


def commands(iterations):
    """Command records on the device with `iterations` in their field and other values in the fields next to it."""
    import torch
    rec = np.zeros(len(iterations), dtype=abi.COMMAND_DTYPE)
    rec["iterations"] = iterations
    rec["status"], rec["evaluations"], rec["flags"], rec["cost"] = 77, 99, -1, 1e9
    return torch.from_numpy(rec.view(np.uint8).reshape(len(rec), -1)).to("cuda:0")


def arm(s, iterations):
    """One balance_dispatch with `iterations` -> what the handle holds after it."""
    kept = commands(iterations)
    s.balance_dispatch(kept)
    return s.dispatch_order()                     # (waits for the device: `kept` may go)


def call(s, iterations, load_before, fresh):
    """One balance_dispatch with `iterations`, expected to continue `load_before` or to start afresh -> the averages."""
    order, load = arm(s, iterations)
    want = ref.update(load_before, iterations, fresh)
    assert load.dtype == np.float32 and load.tobytes() == want.tobytes(), \
        "averages differ at %s" % np.nonzero(load.view(np.uint32) != want.view(np.uint32))[0][:8]
    ref.check(order, load_before, iterations, fresh)
    return load


@pytest.mark.parametrize("count", ref.SORTED_COUNTS)
def test_sorted_counts(solver, count):
    for name, it in ref.sorted_inputs(count).items():
        print(name)
        solver.balance_dispatch(None)             # every input on a fresh average
        call(solver, it, None, True)


@pytest.mark.parametrize("count", ref.IDENTITY_COUNTS)
def test_launch_order_counts(solver, count):
    order, load = arm(solver, ref.random_iterations(count, 6))
    assert order.dtype == np.uint32 and order.tolist() == list(range(count)) and load is None


@pytest.mark.parametrize("count", ref.SEQUENCE_COUNTS)
def test_running_average(solver, count):
    """30 successive calls of one count, other iteration counts on every call: halves, quarters, eighths, values on the
    truncation boundary and float32 rounding (tests/test_dispatch_order_reference.py shows that this sequence has them)."""
    load = None
    for it in ref.sequence(count):
        load = call(solver, it, load, load is None)


def test_when_the_average_restarts(solver):
    s = solver
    assert s.dispatch_order() is None                                    # never armed
    a, b, c, d = (ref.random_iterations(2048, seed) for seed in (21, 22, 23, 24))
    load = call(s, a, None, True)
    load = call(s, b, load, False)                                       # the same count again: continued
    call(s, ref.random_iterations(1024, 25), None, True)                 # another sorted count: afresh, there ...
    load = call(s, c, None, True)                                        # ... and back here
    load = call(s, d, load, False)
    order, none = arm(s, ref.random_iterations(1500, 26))                # a count that gets launch order in between
    assert len(order) == 1500 and none is None
    load = call(s, a, None, True)
    load = call(s, b, load, False)
    s.balance_dispatch(None)
    assert s.dispatch_order() is None
    load = call(s, c, None, True)                                        # disarmed in between: afresh
    call(s, d, load, False)
    arm(s, ref.random_iterations(5120, 27))                              # launch order twice: still nothing to continue
    assert arm(s, ref.random_iterations(5120, 28))[0].tolist() == list(range(5120))
    call(s, ref.random_iterations(4096, 29), None, True)
    s.balance_dispatch(None)
    assert s.dispatch_order() is None


@pytest.mark.parametrize("count", [2048, 3072, 4096])
def test_what_it_is_for(solver, count):
    """The skewed fleet: launch order stacks the heavy robots on a quarter of the SIMDs.  Every SIMD's sum of bins under the
    returned order is the reference's, and the largest is strictly below launch order's."""
    it = ref.skewed_fleet(count)
    load = call(solver, it, None, True)
    order, _ = solver.dispatch_order()
    dealt = ref.simd_sums(order, load)
    assert dealt.tolist() == ref.simd_sums(ref.order_of(load), load).tolist()
    launch = ref.simd_sums(np.arange(count, dtype=np.uint32), load).max()
    print("count %d: largest per-SIMD sum of bins %d dealt, %d in launch order" % (count, dealt.max(), launch))
    assert dealt.max() < launch


@pytest.fixture(scope="module")
def after_a_solve():
    """The one K1 launch of this file: a C2 batch of 4096 solved on a handle that is armed for 2048, then handed to K5."""
    import torch
    from neo_mpc_planner2_amd.solver import BatchSolver, DeviceBatch
    cfg, cmap, probs, st, warm = synthetic.make_workload("C2", seed=5, batch=4096)
    first, second = ref.random_iterations(2048, 31), ref.random_iterations(2048, 32)
    out = dict(first=first, second=second)
    with BatchSolver(util.orc.make_params()) as s:
        s.set_costmap(*cmap)
        out["armed"] = arm(s, first)
        db = DeviceBatch(probs, st, warm, "cuda:0")
        s.solve_device(db.problems, db.states, db.warm, db.commands)          # another batch size: launch order
        out["after_solve"] = s.dispatch_order()
        out["continued"] = arm(s, second)
        s.balance_dispatch(db.commands)
        out["from_k1"] = s.dispatch_order()
        torch.cuda.synchronize()
        out["iterations"] = db.commands_host()["iterations"].copy()
    return out


def test_a_solve_of_another_size_leaves_order_and_average_alone(after_a_solve):
    r = after_a_solve
    load = ref.check(r["armed"][0], None, r["first"], True)
    assert r["armed"][1].tobytes() == load.tobytes()
    for got, was in zip(r["after_solve"], r["armed"]):
        assert got.tobytes() == was.tobytes()                                 # still armed for 2048, nothing rewritten
    again = ref.check(r["continued"][0], load, r["second"], False)            # ... and the average goes on
    assert r["continued"][1].tobytes() == again.tobytes()


def test_k1_feeds_k5(after_a_solve):
    """K5 reads the `iterations` K1 wrote: the order of a solved C2 fleet is the reference's for the counts read back from
    its commands -- and not launch order."""
    order, load = after_a_solve["from_k1"]
    it = after_a_solve["iterations"]
    assert it.dtype == np.int32 and it.max() > it.min()            # (a spread of loads: there was something to sort)
    ref.check(order, None, it, True)
    assert load.tolist() == (2.0 * np.clip(it, 0, 127)).tolist()
    assert order.tolist() != list(range(4096))
