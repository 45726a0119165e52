"""The rule of the dispatch-order kernel K5 (k_dispatch_order, neo_mpc_planner2_amd/csrc/neo_mpc_kernels.hip:259-315; line
numbers as `hip:`) restated in NumPy -- the reference of tests/test_dispatch_order.py.  No device, and nothing of the
library is called.  All of K5's arithmetic is exact in float32 or rounds once where NumPy's float32 rounds once: `2.0f * now`,
`0.5f * load` and `2.0f * e` are exact, so `0.5f * load + now` and `2.0f * e + 0.5f` round the same whether or not the
compiler contracts them.  Every comparison against this module is therefore exact.

The ranks of the instances of one bin come from atomics (hip:292), in any order: `check` compares bin by bin as sets.  That
pins everything but the order inside a bin, and with it every SIMD's sum of bins.

Below the rule: the inputs the CPU tests of this module (tests/test_dispatch_order_reference.py) and the GPU tests share.
Helper module: no tests in here."""
import numpy as np

SIMDS = 1024                # kDispatchSimds (neo_mpc_device.h): workgroups w, w + 1024, ... of a launch share a SIMD
BINS = 512                  # kBins (hip:272)
MAX_ITERATIONS = 127        # the clamp of hip:287
F32 = np.float32
INT32_MIN, INT32_MAX = np.iinfo(np.int32).min, np.iinfo(np.int32).max
#: what the clamp has to cope with, at and around both of its ends
EDGE_ITERATIONS = (-1, INT32_MIN, 0, 1, 126, 127, 128, INT32_MAX)
#: the four kinds of count K5 sorts: one slot (no mirroring), an even number of slots, an odd number (the last slot runs
#: forward again), the full round
SORTED_COUNTS = (1024, 2048, 3072, 4096)
#: ... and counts that get launch order: below, around and between multiples of 1024, and beyond one round -- multiples of
#: 1024 among them
IDENTITY_COUNTS = (1, 1023, 1025, 1500, 4097, 5120, 8192)
#: the counts of the 30-call sequences: one slot, and three (mirrored and forward slots under the finest averages)
SEQUENCE_COUNTS = (1024, 3072)


def is_identity_count(count):
    """hip:275: counts that are no multiple of 1024, or beyond 4096, get launch order."""
    return count % SIMDS != 0 or count > 4 * SIMDS


def update(load, iterations, fresh):
    """hip:286-288: the new average, float32.  `load` is not looked at when `fresh`."""
    iterations = np.asarray(iterations)
    assert iterations.dtype == np.int32
    now = np.clip(iterations, 0, MAX_ITERATIONS).astype(F32)                  # hip:287
    if fresh:
        return F32(2.0) * now                                                 # hip:288 (a fresh average starts at its steady state)
    load = np.asarray(load)
    assert load.dtype == F32 and load.shape == now.shape
    return F32(0.5) * load + now


def bins(load):
    """hip:290: a quarter of an iteration a bin, rounded to nearest by the + 0.5 and the truncation, clamped to the last bin."""
    load = np.asarray(load)
    assert load.dtype == F32
    q = np.minimum(F32(2.0) * load + F32(0.5), F32(BINS - 1))
    assert q.dtype == F32 and (q >= 0).all()
    return q.astype(np.uint32)                                                # (truncation, like the cast)


def keys(load):
    """hip:291: ascending key = descending load."""
    return np.uint32(BINS - 1) - bins(load)


def positions(count):
    """hip:309-312: where position p of the sorted sequence lies in `order` -- slot p // 1024, lane p % 1024, the lane
    mirrored in odd slots (the snake) -> int64 [count], so that `order[positions(count)]` is the sorted sequence."""
    assert not is_identity_count(count)
    p = np.arange(count, dtype=np.int64)
    slot, lane = p // SIMDS, p % SIMDS
    lane = np.where(slot % 2 == 1, SIMDS - 1 - lane, lane)
    return slot * SIMDS + lane


def order_of(load):
    """One of the orders K5 may return for these averages: equals in instance order."""
    order = np.empty(len(load), dtype=np.uint32)
    order[positions(len(load))] = np.argsort(keys(load), kind="stable")
    return order


def simd_sums(order, load):
    """The sum of bins each of the 1024 SIMDs is dealt under `order` (the quantity the deal balances) -> int64 [1024]."""
    return bins(load)[order].astype(np.int64).reshape(-1, SIMDS).sum(axis=0)


def check(order, load_before, iterations, fresh):
    """`order` is one of the orders K5 may return for a call with `iterations` on the averages `load_before` -> the new
    averages.  Raises AssertionError otherwise."""
    load = update(load_before, iterations, fresh)
    count = len(load)
    order = np.asarray(order)
    assert order.dtype == np.uint32 and order.shape == (count,)
    assert np.array_equal(np.sort(order), np.arange(count, dtype=np.uint32)), "not a permutation"
    key = keys(load)
    sequence = order[positions(count)]                                        # un-snaked
    got = key[sequence].astype(np.int64)
    down = np.nonzero(np.diff(got) < 0)[0]
    assert len(down) == 0, "keys fall at position %d: %d then %d" % (down[0], got[down[0]], got[down[0] + 1])
    # bin by bin: the run of positions the reference's histogram gives a bin holds exactly the instances of that bin
    run = np.repeat(np.arange(BINS), np.bincount(key, minlength=BINS))        # the key whose run position p lies in
    in_runs = sequence[np.lexsort((sequence, run))]                           # every run sorted by instance
    want = np.argsort(key, kind="stable")
    wrong = np.nonzero(in_runs != want)[0]
    assert len(wrong) == 0, "the run of key %d holds other instances than the reference's" % run[wrong[0]]
    return load


# ---------------------------------------------------------------------------------------------- shared inputs
def random_iterations(count, seed):
    return np.random.default_rng(seed).integers(0, MAX_ITERATIONS + 1, size=count).astype(np.int32)


def sequence(count, calls=30, seed=11):
    """`calls` successive ticks of one fleet: other counts on every call."""
    return [random_iterations(count, seed + 1000 * c) for c in range(calls)]


def with_edges(count, seed):
    """Random counts with eight of each of EDGE_ITERATIONS planted at random places."""
    rng = np.random.default_rng(seed)
    it = random_iterations(count, seed + 1)
    where = rng.choice(count, size=8 * len(EDGE_ITERATIONS), replace=False)
    it[where] = np.tile(np.array(EDGE_ITERATIONS, dtype=np.int64), 8).astype(np.int32)
    return it


def two_values(count, seed):
    return np.where(np.random.default_rng(seed).random(count) < 0.3, 9, 2).astype(np.int32)


def sorted_inputs(count):
    """name -> iteration counts: the inputs of the sorted counts."""
    return {
        "random": random_iterations(count, 3),
        "all 0": np.zeros(count, dtype=np.int32),           # every instance in the last bin: the scan runs its full length
        "all 127": np.full(count, 127, dtype=np.int32),     # ... in the first bin that can be reached
        "two values": two_values(count, 4),
        "edges": with_edges(count, 5),
    }


def skewed_fleet(count, seed=7):
    """The heavy robots sit at i % 1024 < 256, so launch order stacks them on a quarter of the SIMDs: 8 to 20 iterations
    against 2, no outliers.  (The deal is a heuristic: with a few 127-iteration outliers and three slots the snake can come out
    worse than launch order.  This fleet is one on which the rule, as restated above, wins for 2048, 3072 and 4096 --
    tests/test_dispatch_order_reference.py shows that without a device.)"""
    rng = np.random.default_rng(seed)
    heavy = np.arange(count) % SIMDS < 256
    return np.where(heavy, rng.integers(8, 21, size=count), 2).astype(np.int32)
