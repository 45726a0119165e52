"""The stage-wise sweep (csrc/riccati.h) writes some of its compare-and-select chains as one maximum instruction.  That is
only allowed where both forms give the same BITS for every input -- NaN, signed zeros, infinities and denormals included.
Here the select form (what ric_max / ric_abs / the generic ric_pivot compute) and the instruction form are evaluated in
float32 with NumPy over every combination of a grid of edge values plus a seeded random sample, and compared as bit
patterns.  `np.fmax` has the instruction's NaN rule (a NaN operand is dropped), `np.where(a > b, a, b)` the select's.

The one shape that must NOT be rewritten -- ric_max(a, b) with a b that can be NaN, the maxima over the diagonal inside
`delta` -- is held against fmax as well, and the two are asserted to DIFFER: the test would notice a rule that is too lax."""
import itertools

import numpy as np

F = np.float32
TINY = F(1e-30)        # the floor of delta (riccati.h: 1e-30f)
SCALE = F(1e-6)


def _grid():
    d = np.finfo(np.float32)
    base = [0.0, d.smallest_subnormal, 3 * d.smallest_subnormal, d.smallest_normal * F(0.5), d.smallest_normal,
            np.nextafter(TINY, F(0)), TINY, np.nextafter(TINY, F(1)), F(1e-24), np.nextafter(F(1e-24), F(1)), F(1e-6), F(0.5),
            F(1.0), F(3.0), F(1e24), F(1e30), F(1e36), d.max, np.inf]
    vals = [F(v) for v in base] + [-F(v) for v in base] + [F(np.nan), -F(np.nan)]
    return np.array(vals, dtype=np.float32)


def _sample(n, seed):
    """Random bit patterns (every exponent, both signs, NaNs among them) and ordinary magnitudes."""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32).view(np.float32)
    mags = (rng.standard_normal(n) * 10.0 ** rng.uniform(-35, 35, size=n)).astype(np.float32)
    return np.concatenate([bits, mags])


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ---- the select forms (riccati.h: ric_max, ric_abs, the generic ric_pivot) ----------------------------------------
def sel_max(a, b):
    return np.where(a > b, a, b).astype(np.float32)


def sel_abs(a):
    return np.where(a < F(0), -a, a).astype(np.float32)


def sel_pivot(p, delta):
    return np.where(p > delta, p, sel_max(sel_abs(p), delta)).astype(np.float32)


# ---- the instruction forms (ric_floor, ric_mag, the float32 ric_pivot) --------------------------------------------
def ins_floor(a):
    return np.fmax(a, TINY).astype(np.float32)


def ins_pivot(p, delta):
    return np.fmax(np.abs(p), delta).astype(np.float32)


def _values():
    return np.concatenate([_grid(), _sample(2000, 20)])


def test_floor_is_fmax_against_a_constant():
    """ric_max(a, 1e-30f) == fmaxf(a, 1e-30f) for every a."""
    a = _values()
    with np.errstate(all="ignore"):
        assert _same(sel_max(a, TINY), ins_floor(a))


def test_pivot_is_fmax_of_magnitude_and_delta():
    """ric_pivot(p, delta) == fmaxf(|p|, delta) for every p and every delta the sweep can produce: delta is the result
    of ric_max(., 1e-30f), so it is never NaN and never below 1e-30f."""
    v = _values()
    with np.errstate(all="ignore"):
        deltas = np.unique(np.concatenate([sel_max(v, TINY), sel_max(SCALE * sel_abs(v), TINY)]))
        assert not np.isnan(deltas).any() and (deltas >= TINY).all()
        p, d = np.meshgrid(v, deltas, indexing="ij")
        assert _same(sel_pivot(p, d), ins_pivot(p, d))


def test_delta_with_fabs_under_the_floor():
    """delta of the three sweep shapes: ric_floor(1e-6f * max(...)) with fabsf for ric_abs and the maxima over the
    diagonal kept as selects equals the all-select form -- a zero of either sign and a NaN of either sign end as 1e-30f."""
    g = _grid()
    with np.errstate(all="ignore"):
        # one diagonal entry (RC_SLIDE, RC_W)
        a = _values()
        assert _same(sel_max(SCALE * sel_abs(a), TINY), ins_floor(SCALE * np.abs(a)))
        # two (RC_SLIDE_W, RC_XY)
        a, b = (np.concatenate([x.ravel(), s]) for x, s in zip(np.meshgrid(g, g, indexing="ij"),
                                                                (_sample(3000, 21), _sample(3000, 22))))
        old = sel_max(SCALE * sel_max(sel_abs(a), sel_abs(b)), TINY)
        new = ins_floor(SCALE * sel_max(np.abs(a), np.abs(b)))
        assert _same(old, new)
        # three (RC_FREE3)
        trip = np.array(list(itertools.product(g, repeat=3)), dtype=np.float32)
        rnd = np.stack([_sample(3000, 23 + k) for k in range(3)], axis=1)
        a, b, c = np.concatenate([trip, rnd]).T
        old = sel_max(SCALE * sel_max(sel_abs(a), sel_max(sel_abs(b), sel_abs(c))), TINY)
        new = ins_floor(SCALE * sel_max(np.abs(a), sel_max(np.abs(b), np.abs(c))))
        assert _same(old, new)
        # ... and the pivots taken with it: the whole chain from the diagonal to the three replaced pivots
        assert _same(sel_pivot(a, old), ins_pivot(a, new)) and _same(sel_pivot(b, old), ins_pivot(b, new))


def test_the_maxima_inside_delta_are_not_fmax():
    """ric_max(a, b) with a b that can be NaN: the select hands back b, the instruction a.  These keep their selects."""
    g = _grid()
    a, b = (x.ravel() for x in np.meshgrid(g, g, indexing="ij"))
    with np.errstate(all="ignore"):
        old, new = sel_max(a, b), np.fmax(a, b).astype(np.float32)
        differ = _bits(old) != _bits(new)
        assert differ.any()
        # where b is NaN and a is a number the two forms disagree, every time
        where = np.isnan(b) & ~np.isnan(a)
        assert where.any() and differ[where].all()
        # and it reaches delta: a NaN in the LAST diagonal entry makes the select form fall to the floor, fmax would not
        q = np.array([F(2.0), F(3.0), F(np.nan)], dtype=np.float32)
        d_sel = sel_max(SCALE * sel_max(sel_abs(q[0:1]), sel_max(sel_abs(q[1:2]), sel_abs(q[2:3]))), TINY)
        d_max = ins_floor(SCALE * np.fmax(np.abs(q[0:1]), np.fmax(np.abs(q[1:2]), np.abs(q[2:3]))))
        assert d_sel[0] == TINY and d_max[0] != TINY


def test_row_maximum_of_non_negative_values_is_order_free():
    """wave_max_f_few (csrc/wave_ops.h) takes the nine values of the three-stage step test in another order than the
    64-lane ladder: for non-negative values that are not NaN (zeros positive: they come out of fabs) every order gives
    the same bits."""
    rng = np.random.default_rng(30)
    pool = np.abs(np.concatenate([_grid(), _sample(500, 31)]))
    pool = pool[~np.isnan(pool)]
    for _ in range(200):
        v = rng.choice(pool, size=9)
        ref = _bits(np.max(v))
        for _ in range(5):
            w = rng.permutation(v)
            acc = w[0]
            for x in w[1:]:
                acc = np.fmax(acc, x)
            assert _bits(acc) == ref
