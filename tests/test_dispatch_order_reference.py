"""CPU tests of tests/dispatch_order_reference.py itself, the restatement of K5's rule that tests/test_dispatch_order.py holds
the kernel against: a case worked by hand, what `check` refuses, and that the shared inputs reach the places they are there
for -- the truncation boundary, float32 rounding, a fleet the deal does balance.  No GPU and no library."""
import numpy as np
import pytest

from tests import dispatch_order_reference as ref

F32 = np.float32


def hand_worked():
    """1024 robots, all of them at 2 iterations but seven: -> (iterations, the bins of a fresh call, one order K5 may return)."""
    it = np.full(1024, 2, dtype=np.int32)
    it[[5, 17]] = 127, 200          # 200 is clamped to 127
    it[[3, 700]] = 8
    it[1000] = -4                   # clamped to 0
    it[[40, 41]] = 3
    bins = np.full(1024, 8)         # load 2 * 2 = 4, bin 2 * 4 + 0.5 -> 8
    bins[[5, 17]] = 508             # load 254, 508.5 -> 508
    bins[[3, 700]] = 32             # load 16
    bins[1000] = 0
    bins[[40, 41]] = 12             # load 6
    rest = [i for i in range(1024) if i not in (5, 17, 3, 700, 40, 41, 1000)]
    # longest first; one slot, so nothing is mirrored; equals in any order (here: not in instance order)
    order = np.array([17, 5, 700, 3, 41, 40] + rest[::-1] + [1000], dtype=np.uint32)
    return it, bins, order


def test_hand_worked_case():
    it, bins, order = hand_worked()
    load = ref.update(None, it, True)
    assert load.dtype == F32 and load[5] == load[17] == 254 and load[3] == 16 and load[1000] == 0 and load[0] == 4
    assert ref.bins(load).tolist() == bins.tolist() and ref.keys(load).tolist() == (511 - bins).tolist()
    assert ref.check(order, None, it, True).tobytes() == load.tobytes()
    assert ref.check(ref.order_of(load), None, it, True) is not None
    assert ref.simd_sums(order, load).tolist() == bins[order].tolist()             # (one slot: a SIMD has one instance)
    # the next call, every robot at 3 iterations: 0.5 * load + 3
    again = np.full(1024, 3, dtype=np.int32)
    load2 = ref.update(load, again, False)
    assert load2[5] == 130 and load2[3] == 11 and load2[40] == 6 and load2[0] == 5 and load2[1000] == 3
    bins2 = ref.bins(load2)
    assert (bins2[5], bins2[3], bins2[40], bins2[0], bins2[1000]) == (260, 22, 12, 10, 6)
    assert ref.check(order, load, again, False).tobytes() == load2.tobytes()       # (the same ranking of the robots)
    # ... and when it is taken for a fresh one, 2 * 3 for everybody: one bin, any permutation will do
    assert ref.check(np.arange(1024, dtype=np.uint32), None, again, True).tolist() == [6.0] * 1024


def test_check_refuses_what_is_no_order_of_the_rule():
    it, bins, order = hand_worked()
    refused = {
        "launch order": np.arange(1024, dtype=np.uint32),
        "ascending": order[::-1].copy(),
        "an instance twice": np.where(np.arange(1024) == 9, order[8], order).astype(np.uint32),
        "two bins swapped": order[[2, 1, 0] + list(range(3, 1024))],
        "int64": order.astype(np.int64),
    }
    for name, bad in refused.items():
        with pytest.raises(AssertionError):
            ref.check(bad, None, it, True)
            print("accepted:", name)
    swapped_inside_a_bin = order[[1, 0] + list(range(2, 1024))]
    ref.check(swapped_inside_a_bin, None, it, True)


def test_the_snake():
    """Position p of the sorted sequence: slot p // 1024, lanes left to right in even slots, right to left in odd ones."""
    assert ref.positions(1024).tolist() == list(range(1024))
    p = ref.positions(3072)
    assert sorted(p.tolist()) == list(range(3072))
    assert (p[0], p[1023], p[1024], p[1025], p[2047], p[2048], p[3071]) == (0, 1023, 2047, 2046, 1024, 2048, 3071)
    # 2048 robots, robot i at i // 16 iterations: the 1024 longest go left to right, the others come back
    it = (np.arange(2048) // 16).astype(np.int32)
    order = ref.order_of(ref.update(None, it, True))
    assert order[:3].tolist() == [2032, 2033, 2034] and order[1024:1027].tolist() == [15, 14, 13] and order[2047] == 1008
    # SIMD l is dealt 127 - l // 16 and l // 16 iterations, 4 bins an iteration
    assert ref.simd_sums(order, ref.update(None, it, True)).tolist() == [4 * 127] * 1024
    for count in ref.IDENTITY_COUNTS:
        assert ref.is_identity_count(count)
    for count in ref.SORTED_COUNTS:
        assert not ref.is_identity_count(count)


def test_largest_reachable_load_and_bin():
    """The clamp keeps a count at 127 or below, so a fresh average is at most 254, a running one stays at or below 254
    (0.5 * 254 + 127), and the largest bin is 508 (2 * 254 + 0.5 truncated).  Keys 0 to 2 -- bins 509 to 511 -- are therefore
    never produced through the API: neither the fminf saturation of the bin (neo_mpc_kernels.hip:290) nor the `key ? ... : 0`
    branch of the position (hip:309, key 0) can be reached, and no test here claims to cover them."""
    top = np.full(1024, ref.INT32_MAX, dtype=np.int32)
    load = ref.update(None, top, True)
    for _ in range(40):
        assert load.max() == 254 and ref.bins(load).max() == 508 and ref.keys(load).min() == 3
        load = ref.update(load, top, False)
    for it in ref.sorted_inputs(1024).values():
        assert ref.keys(ref.update(None, it, True)).min() >= 3
    assert ref.update(None, np.array(ref.EDGE_ITERATIONS, dtype=np.int32), True).tolist() == [0, 0, 0, 2, 252, 254, 254, 254]


@pytest.mark.parametrize("count", ref.SEQUENCE_COUNTS)
def test_the_sequence_reaches_the_truncation_boundary_and_float32_rounding(count):
    """What the 30-call sequence of the GPU test is there for.  The first average is an even integer, the second an integer,
    the third has halves and the fourth quarters: from the fourth call on 2 * e + 0.5 lands exactly on integers -- the
    boundary of the truncation, where a dropped `+ 0.5f` or a rounding the other way moves an instance to another bin.  Every
    call adds a binary digit, so after about 18 calls the float32 average has rounded and differs from the float64 one."""
    seq = ref.sequence(count)
    assert len(seq) == 30 and all((a != b).any() for a, b in zip(seq, seq[1:]))
    load, exact = None, None
    on_boundary, adjacent_bins, rounded = [], [], None
    for call, it in enumerate(seq, start=1):
        load = ref.update(load, it, call == 1)
        now = np.clip(it, 0, 127).astype(np.float64)
        exact = 2.0 * now if call == 1 else 0.5 * exact + now
        q = 2.0 * load.astype(np.float64) + 0.5                  # (exact in float64)
        if (q == np.floor(q)).any():
            on_boundary.append(call)
        occupied = np.bincount(ref.bins(load), minlength=ref.BINS) > 0
        if (occupied[1:] & occupied[:-1]).any():
            adjacent_bins.append(call)
        if rounded is None and (load.astype(np.float64) != exact).any():
            rounded = call
    assert on_boundary[:5] == [4, 5, 6, 7, 8]                    # (rarer with every digit the average gains)
    assert adjacent_bins[0] == 3                                 # (before that only every fourth, then every second bin is used)
    assert rounded is not None and rounded <= 30


@pytest.mark.parametrize("count", [2048, 3072, 4096])
def test_the_deal_balances_the_skewed_fleet(count):
    """The rule alone, without a device: on the skewed fleet the largest per-SIMD sum of bins is strictly below launch
    order's."""
    it = ref.skewed_fleet(count)
    load = ref.update(None, it, True)
    dealt = ref.simd_sums(ref.order_of(load), load).max()
    launch = ref.simd_sums(np.arange(count, dtype=np.uint32), load).max()
    assert dealt < launch, (dealt, launch)
    assert ref.simd_sums(np.arange(count, dtype=np.uint32), load).sum() == ref.simd_sums(ref.order_of(load), load).sum()


def test_one_slot_has_nothing_to_balance():
    it = ref.skewed_fleet(1024)
    load = ref.update(None, it, True)
    assert ref.simd_sums(ref.order_of(load), load).max() == ref.simd_sums(np.arange(1024, dtype=np.uint32), load).max()
