"""The host restatement of the sampler and dropout streams (tests/counter_streams.py) checked on its own: the rules it states
give the distributions they are meant to give, and the sampler's uniform number never leaves (0, 1)."""
import numpy as np
import pytest

import counter_streams as cs


def test_hashes_are_the_documented_functions():
    """Scalar Python-int restatements (arbitrary precision, masked by hand) against the vectorised uint64 ones, at counters and seeds
    with bits above 2^32 and 2^63."""
    M = (1 << 64) - 1

    def mix(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)

    def h_hi(seed, i):
        return mix((seed + (i + 1) * cs.GOLDEN) & M) >> 32

    def d_h(seed, i):
        k = mix(((seed + 0x632BE59BD9B4E019) * cs.GOLDEN) & M)
        hi = (i >> 32) & 0xFFFFFFFF
        x = ((i & 0xFFFFFFFF) + (((hi << 19) | (hi >> 13)) & 0xFFFFFFFF)) & 0xFFFFFFFF
        x ^= k & 0xFFFFFFFF
        x = ((x ^ (x >> 16)) * 0x7FEB352D) & 0xFFFFFFFF
        x = (((x ^ (x >> 15)) + (k >> 32)) * 0x846CA68B) & 0xFFFFFFFF
        return x ^ (x >> 16)

    ids = [0, 1, 255, 2 ** 32 - 1, 2 ** 32, 5 * 2 ** 32 + 7, 2 ** 45 + 3, 2 ** 63 + 11, 2 ** 64 - 1]
    for seed in (0, 987654321, 2 ** 63 + 12345, 2 ** 64 - 1):
        got_h, got_d = cs.hash64_hi(seed, np.array(ids, dtype=np.uint64)), cs.drop_hash(seed, np.array(ids, dtype=np.uint64))
        assert [int(v) for v in got_h] == [h_hi(seed, i) for i in ids]
        assert [int(v) for v in got_d] == [d_h(seed, i) for i in ids]
    # the rotated upper half of the element id is part of the dropout hash
    assert int(cs.drop_hash(1, np.uint64(2 ** 32))) != int(cs.drop_hash(1, np.uint64(0)))


@pytest.mark.parametrize("T", [1.0, 0.7])
def test_the_rule_gives_the_distribution(T):
    """200 000 restated draws at V = 8: every frequency within 5 binomial standard deviations of softmax(lp / T)."""
    n, V = 200_000, 8
    lp = np.log(np.array([0.40, 0.25, 0.15, 0.10, 0.05, 0.03, 0.015, 0.005])).astype(np.float32)
    scores = cs.gumbel_scores(lp, 20240607, 0, np.arange(n), n, T)
    assert scores.shape == (n, V) and np.isfinite(scores).all()
    freq = np.bincount(scores.argmax(1), minlength=V) / n
    z = lp.astype(np.float64) / T
    p = np.exp(z - z.max()); p /= p.sum()
    sd = np.sqrt(p * (1 - p) / n)
    assert (np.abs(freq - p) <= 5 * sd).all(), (freq, p, sd)


def test_uniform_stays_inside_the_open_unit_interval():
    """The float32 conversion rounds every hash >= 0xFFFFFF80 to 2^32; without a bound below 1 the uniform number is 1.0 there, its
    Gumbel value +inf, and the entry wins the draw whatever its log-prob."""
    edge = np.array([0, 1, 0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFFFF], dtype=np.uint32)
    u = cs.uniform(edge)
    assert u.dtype == np.float32 and (u > 0).all() and (u < 1).all(), u
    # ... over a sweep of the top of the range and a stride through all of it
    top = np.arange(0xFFFFF000, 0x100000000, dtype=np.uint64).astype(np.uint32)
    stride = np.arange(0, 0x100000000, 4093, dtype=np.uint64).astype(np.uint32)
    for h in (top, stride):
        u = cs.uniform(h)
        assert (u > 0).all() and (u < 1).all()
        assert (np.diff(u.astype(np.float64)) >= 0).all()                 # monotone in the hash
    g = -np.log(-np.log(cs.uniform(edge).astype(np.float64)))
    assert np.isfinite(g).all() and g.max() < 17.0 and g.min() > -3.2     # -log(-log(1 - 2^-24)) = 16.64, -log(-log(2^-33)) = -3.13
    # every restated score of a finite log-prob is finite
    lp = np.linspace(-30, 0, 257).astype(np.float32)
    for seed in (0, 12345, 2 ** 64 - 1):
        assert np.isfinite(cs.gumbel_scores(lp, seed, 3, np.arange(7), 7, 0.7)).all()
    # the rule without the bound: exactly the faults described above (what the clamp is for)
    old = cs.uniform_unclamped(edge)
    assert old[3] == 1.0 and old[4] == 1.0 and old[2] < 1.0
    # and the clamp changes no other hash's uniform number
    assert np.array_equal(cs.uniform(stride[stride < 0xFFFFFF80]), cs.uniform_unclamped(stride[stride < 0xFFFFFF80]))


def test_a_24_bit_mantissa_form_would_round_to_one_as_well():
    """((h >> 8) + 0.5) * 2^-24 needs 25 significant bits from h >> 8 = 2^23 on: 16777215.5 rounds to 2^24 and the product is 1.0.
    Stated here so that the clamp is not replaced by that form."""
    x = (np.float32(0xFFFFFFFF >> 8) + np.float32(0.5)) * np.float32(2.0 ** -24)
    assert x == np.float32(1.0)


def test_streams_of_distinct_draws_do_not_overlap():
    """Counters of (row, c) are the V consecutive integers from (row * n + c) * V: distinct (row, c) give disjoint ranges, by construction
    (row * n + c is a bijection onto 0 .. rows * n - 1)."""
    rows, n, V = 15, 7, 257
    base = np.array([[(r * n + c) * V for c in range(n)] for r in range(rows)])
    assert np.array_equal(np.sort(base.ravel()), np.arange(rows * n) * V)
    # ... and the restatement does use them: the scores of draw (r, c) are those of row 0's draw r * n + c among rows * n
    lp = np.linspace(-9, 0, V).astype(np.float32)
    a = cs.gumbel_scores(lp, 5, 4, 3, n, 1.0)
    b = cs.gumbel_scores(lp, 5, 0, 4 * n + 3, rows * n, 1.0)
    assert a.shape == (V,) and np.array_equal(a, b)
    assert not np.array_equal(a, cs.gumbel_scores(lp, 5, 4, 2, n, 1.0))


def test_draw_candidates():
    s = np.array([0.0, 1.0, 0.99995, -np.inf, 1.0 - 1e-3])
    assert cs.draw_candidates(s, 6e-5).tolist() == [1, 2]
    assert cs.draw_candidates(s, 0.0).tolist() == [1]
    assert cs.draw_candidates(np.full(5, -np.inf), 1e-3).tolist() == [0]
    tol = cs.near_tie_tol(np.array([-3.0, -np.inf, np.nan, -20.0]), 1.0)
    assert tol == 16 * 2.0 ** -18                                         # ulp of float32 at 32 is 2^-18
    assert cs.near_tie_tol(np.array([-20.0]), 1e-3) == 16 * float(np.spacing(np.float32(20000.0)))


@pytest.mark.parametrize("p", [0.1, 0.3, 0.5])
def test_dropout_rate_and_seed_independence(p):
    n = 1 << 20
    idx = np.arange(n, dtype=np.uint64)
    k0, k1 = cs.keep_mask(777, 0, p, idx), cs.keep_mask(778, 0, p, idx)
    sd = np.sqrt(p * (1 - p) / n)
    assert abs(k0.mean() - (1 - p)) <= 5 * sd and abs(k1.mean() - (1 - p)) <= 5 * sd
    q = 2 * p * (1 - p)
    assert abs((k0 != k1).mean() - q) <= 5 * np.sqrt(q * (1 - q) / n)
    # the step word adds to the seed
    assert np.array_equal(cs.keep_mask(777, 1, p, idx), k1)
    # element ids
    assert cs.linear_ids(3, 5)[2, 4] == 14
    assert cs.attn_ids_padded(2, 3, 4, 5)[1, 2, 3, 4] == ((1 * 3 + 2) * 4 + 3) * 5 + 4
    assert cs.attn_ids_unpadded([7, 9], 2, 5)[1, 1, 3] == (9 * 2 + 1) * 5 + 3
