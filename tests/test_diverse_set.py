"""The Hamming-diverse caption set of the NAIC decode, host side (no GPU): the rule of ``bofi_vocab_diverse`` (include/boficap_hip.h states it in words) RESTATED in
numpy (``diverse_np``: the candidates in ``order_np``'s order, the host-made penalty table, the per-position pick and the Viterbi with their tie orders), held against a
BRUTE FORCE over every valid caption with the augmented objective -- what tests/test_gpu_diverse_set.py holds the kernel and the engines to --, hand-worked cases, the
properties the header states, the declarations, and the refusals that need no device."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_constrained_pick import order_np, pick_np
from test_nbest import same_bits
from test_nbest_no_repeat import is_valid, nbest_nr_np

NAN, INF = float("nan"), float("inf")


# ----------------------------------------------------------------------------- the rule, restated
def diverse_np(x, n, N, lam, ban=(), no_repeat=False, repeat_min_id=7, K=None, pad=0):
    """The diverse sets of x [B, S, >= V] (all of x.shape[2] columns are the vocabulary) with n [B] live positions (clamped to 0 .. S): a dict of ``seq`` int64
    [B, N, S], ``total`` and ``aug`` float64 [B, N], ``count`` int32 [B], and ``degenerate`` bool [B].  ``K``: candidates per row -- the rule's N, or N + 2 under the
    repeat rule, by default.  K is the one place where N enters a group's result: with K held fixed, the first N' groups of the N-set are the N'-set."""
    x = np.asarray(x)
    B, S, _ = x.shape
    K = (N + 2 if no_repeat else N) if K is None else K
    ban = sorted({int(i) for i in ban})
    pen = [float(lam) * float(k) for k in range(N)]             # the one product of the rule: python floats are the host's doubles
    seq = np.full((B, N, S), pad, np.int64)
    total = np.full((B, N), -INF, np.float64)
    aug = np.full((B, N), -INF, np.float64)
    count = np.zeros(B, np.int32)
    degenerate = np.zeros(B, bool)
    for b in range(B):
        nb = min(max(int(n[b]), 0), S)
        rows = []                                               # per live row: (first id or None, {r: (id, value)} of its candidates)
        for p in range(nb):
            order = [int(i) for i in order_np(x[b, p], ban)[:K]]
            first = order[0] if order else None
            if first is None or not np.isfinite(x[b, p, first]):
                degenerate[b] = True
            rows.append((first, {r: (i, float(x[b, p, i])) for r, i in enumerate(order) if r == 0 or np.isfinite(x[b, p, i])}))
        if degenerate[b]:
            count[b], total[b, 0], aug[b, 0] = 1, NAN, NAN
            seq[b, 0, :nb] = [pad if first is None else first for first, _ in rows]
            continue
        if nb == 0:
            count[b], total[b, 0], aug[b, 0] = 1, 0.0, 0.0
            continue
        cnt = [dict.fromkeys(c, 0) for _, c in rows]            # cnt[p][r]: the earlier groups that took c[p][r] (a row's candidates are distinct ids)
        for g in range(N):
            a = [{r: v - pen[cnt[p][r]] for r, (_, v) in rows[p][1].items()} for p in range(nb)]      # one float64 subtraction each
            if not no_repeat:
                take, t = [], 0.0
                for p in range(nb):
                    best = None
                    for r in sorted(a[p]):
                        if best is None or a[p][r] > a[p][best]:
                            best = r
                    take.append(best)
                    t = t + a[p][best]
            else:
                Vp = {r: 0.0 + a[0][r] for r in sorted(a[0])}
                back = [None]
                for p in range(1, nb):
                    new, bp = {}, {}
                    for r in sorted(a[p]):
                        i = rows[p][1][r][0]
                        best = None
                        for rq in sorted(Vp):
                            iq = rows[p - 1][1][rq][0]
                            if iq == i and iq >= repeat_min_id:
                                continue
                            val = Vp[rq] + a[p][r]               # one float64 add per pair
                            if best is None or val > best[0]:
                                best = (val, rq)
                        if best is not None:
                            new[r], bp[r] = best
                    Vp = new
                    back.append(bp)
                if not Vp:                                      # no valid caption over the candidates: the same for every group
                    break
                end = None
                for r in sorted(Vp):
                    if end is None or Vp[r] > Vp[end]:
                        end = r
                t = Vp[end]
                take = [end]
                for p in range(nb - 1, 0, -1):
                    take.append(back[p][take[-1]])
                take.reverse()
            own = 0.0
            for p, r in enumerate(take):
                own = own + rows[p][1][r][1]
                cnt[p][r] += 1
            seq[b, g, :nb] = [rows[p][1][r][0] for p, r in enumerate(take)]
            total[b, g], aug[b, g] = own, t
            count[b] = g + 1
    return dict(seq=seq, total=total, aug=aug, count=count, degenerate=degenerate)


def brute_diverse(x, n, N, lam, ban=(), no_repeat=False, repeat_min_id=7):
    """Group by group over EVERY valid caption of one image x [S, V]: the maximiser of the left-to-right float64 sum of x - pen[cnt], cnt from the brute force's own
    earlier groups.  Returns (captions, values, tie): tie = at some group two captions attained the maximum (the groups from there on are not comparable); an empty
    list when there is no valid caption."""
    V = x.shape[1]
    ids = np.array([i for i in range(V) if i not in set(ban)], np.int64)
    caps = np.zeros((1, 0), np.int64)
    for _ in range(n):
        caps = np.concatenate([np.repeat(caps, len(ids), 0), np.tile(ids, len(caps))[:, None]], 1)
    ok = np.ones(len(caps), bool)
    if no_repeat:
        for p in range(1, n):
            ok &= ~((caps[:, p] == caps[:, p - 1]) & (caps[:, p - 1] >= repeat_min_id))
    caps = caps[ok]
    if not len(caps):
        return [], [], False
    pen = np.array([float(lam) * float(k) for k in range(N)], np.float64)
    cnt = np.zeros((n, V), np.int64)
    got, vals = [], []
    for g in range(N):
        T = np.zeros(len(caps), np.float64)
        for p in range(n):
            T = T + (x[p, caps[:, p]].astype(np.float64) - pen[cnt[p, caps[:, p]]])
        best = T.max()
        where = np.flatnonzero(T == best)
        if len(where) > 1:
            return got, vals, True
        cap = caps[where[0]]
        got.append([int(i) for i in cap])
        vals.append(float(best))
        cnt[np.arange(n), cap] += 1
    return got, vals, False


def _brute_cases(count=1200):
    """V in 2..7, S = 4, n in 1..4, the repeat rule on every second case, N in 1..8 (1..6 under the rule), lambda from {0.25, 0.3, 0.5, 1, 3}, repeat_min_id in 0..2;
    values on a grid of eighths in [-8, 0], every third case float32 logs of Dirichlet(0.5) rows; every fourth case a random ban list that leaves at least one id."""
    rng = np.random.default_rng(31)
    for case in range(count):
        nr = bool(case % 2)
        V, S, n = int(rng.integers(2, 8)), 4, int(rng.integers(1, 5))
        N = int(rng.integers(1, 7 if nr else 9))
        lam = (0.25, 0.3, 0.5, 1.0, 3.0)[int(rng.integers(0, 5))]
        lo = int(rng.integers(0, 3))
        x = (-rng.integers(0, 65, (1, S, V)) / 8.0).astype(np.float32)
        if case % 3 == 0:
            x = np.log(rng.dirichlet(np.full(V, 0.5), (1, S)) + 1e-30).astype(np.float32)
        ban = tuple(int(i) for i in rng.choice(V, int(rng.integers(0, V)), replace=False)) if (case + case // 4) % 4 == 0 else ()      # (one case in every four, on both parities)
        yield case, x, n, N, lam, ban, nr, lo


# ----------------------------------------------------------------------------- tests
def test_every_group_is_the_brute_force_maximiser():
    """1 200 cases (``_brute_cases``).  A case is left out only when, at some group, two captions attain the brute force's maximum; in every other case the captions
    are the brute force's and aug its values, bit for bit; count = 0 exactly where there is no valid caption.  At most 25 % of the cases are left out."""
    left, empty, nr_cases = 0, 0, 0
    for case, x, n, N, lam, ban, nr, lo in _brute_cases():
        r = diverse_np(x, [n], N, lam, ban, nr, lo)
        caps, vals, tie = brute_diverse(x[0], n, N, lam, ban, nr, lo)
        if tie:
            left += 1
            continue
        if not caps:
            empty += 1
            assert r["count"][0] == 0 and (r["seq"] == 0).all() and (r["total"] == -INF).all() and (r["aug"] == -INF).all(), case
            continue
        nr_cases += nr
        assert r["count"][0] == N and not r["degenerate"][0], case
        assert r["seq"][0, :, :n].tolist() == caps, (case, r["seq"][0, :, :n].tolist(), caps)
        assert same_bits(r["aug"][0], np.array(vals)), (case, r["aug"][0], vals)
        assert (r["seq"][0, :, n:] == 0).all()
    print(f"diverse set against the brute force: 1200 cases, {left} left out (a group's maximum attained twice), {empty} without a valid caption, "
          f"{nr_cases} compared under the repeat rule")
    assert left <= 300 and nr_cases >= 200


def test_hand_worked_cases():
    """V = 4, S = 2, every id a word (repeat_min_id = 0).  row 0 = [-0.25, -1, -0.5, -3], row 1 = [-2, -0.125, -0.25, -1]; the orders are 0, 2, 1, 3 and 1, 2, 3, 0.
    (a) no_repeat = 0, N = 3, lambda = 0.5.  g0: (0, 1), aug = total = -0.375.  g1: row 0 has id 0 at -0.25 - 0.5 = -0.75 against id 2 at -0.5; row 1 has id 1 at
        -0.625 against id 2 at -0.25: (2, 2), aug = total = -0.75.  g2: row 0: id 0 -0.75, id 2 -1.0, id 1 -1.0 -> id 0; row 1: id 1 -0.625, id 2 -0.75, id 3 -1.0 -> id 1:
        (0, 1) AGAIN (captions need not differ), aug = -1.375, total = -0.375.
    (b) the same with lambda = 1: lambda decides between repeating a word and taking the runner-up.  g1 as before ((2, 2), aug -0.75); g2: row 0: id 0 -1.25, id 2 -1.5,
        id 1 -1.0 -> id 1; row 1: id 1 -1.125, id 2 -1.25, id 3 -1.0 -> id 3: (1, 3), aug = total = -2.0.
    (c) no_repeat = 1, N = 2, lambda = 0.5.  g0 = (0, 1): valid as it is.  g1: (2, 2), the best under (a), repeats a word; (0, 2) = -0.75 - 0.25 = -1.0 beats
        (2, 1) = -1.125, (1, 2) = -1.25, (2, 3) = -1.5: aug = -1.0, total = -0.5.
    (d) the repeat rule changes group 0: ids >= 7 words; row 0: 8 at 0, 9 at -1; row 1: 8 at 0, 9 at -1, 7 at -1.  Plain group 0 is (8, 8); under the rule
        V_1 = -1 for each of 8 (from 9), 7 (from 8) and 9 (from 8): the tie goes to the lowest r, id 8, so (9, 8), aug = total = -1."""
    x = np.array([[[-0.25, -1.0, -0.5, -3.0], [-2.0, -0.125, -0.25, -1.0]]], np.float32)
    a = diverse_np(x, [2], 3, 0.5, repeat_min_id=0)
    assert a["seq"][0].tolist() == [[0, 1], [2, 2], [0, 1]] and a["aug"][0].tolist() == [-0.375, -0.75, -1.375] and a["total"][0].tolist() == [-0.375, -0.75, -0.375]
    assert a["count"].tolist() == [3]
    b = diverse_np(x, [2], 3, 1.0, repeat_min_id=0)
    assert b["seq"][0].tolist() == [[0, 1], [2, 2], [1, 3]] and b["aug"][0].tolist() == [-0.375, -0.75, -2.0] and b["total"][0].tolist() == [-0.375, -0.75, -2.0]
    c = diverse_np(x, [2], 2, 0.5, no_repeat=True, repeat_min_id=0)
    assert c["seq"][0].tolist() == [[0, 1], [0, 2]] and c["aug"][0].tolist() == [-0.375, -1.0] and c["total"][0].tolist() == [-0.375, -0.5]
    for r, (N, lam, nr) in ((a, (3, 0.5, False)), (b, (3, 1.0, False)), (c, (2, 0.5, True))):
        caps, vals, tie = brute_diverse(x[0], 2, N, lam, (), nr, 0)
        assert not tie and caps == r["seq"][0].tolist() and vals == r["aug"][0].tolist()
    y = np.full((1, 2, 10), -9.0, np.float32)
    y[0, 0, 8], y[0, 0, 9] = 0.0, -1.0
    y[0, 1, 8], y[0, 1, 9], y[0, 1, 7] = 0.0, -1.0, -1.0
    assert diverse_np(y, [2], 1, 0.5)["seq"][0].tolist() == [[8, 8]]
    d = diverse_np(y, [2], 1, 0.5, no_repeat=True)
    assert d["seq"][0].tolist() == [[9, 8]] and d["aug"][0].tolist() == [-1.0] and d["total"][0].tolist() == [-1.0]


def sandwich2(V=12):
    """S = 3, repeat_min_id = 0: row 0 is finite only at id 9, row 2 only at id 10; row 1 is led by 9, then 10, then ids 0, 1, 2, ...  Both leaders of row 1 are
    excluded by the neighbours, group 0 takes id 0 (rank 2), and group 1 -- g = 1 -- is best served by id 1: rank 3 = g + 2, the (g + 3)-th candidate."""
    x = np.full((1, 3, V), -INF, np.float32)
    x[0, 0, 9], x[0, 2, 10] = -0.5, -0.25
    x[0, 1] = -2.0 - np.arange(V) / 4.0
    x[0, 1, 9], x[0, 1, 10] = -0.125, -0.375
    return x


def test_g_plus_2_candidates_are_not_enough_under_the_repeat_rule():
    x = sandwich2()
    full = diverse_np(x, [3], 2, 0.5, no_repeat=True, repeat_min_id=0)               # K = N + 2 = 4 = g + 3 for the last group
    short = diverse_np(x, [3], 2, 0.5, no_repeat=True, repeat_min_id=0, K=3)         # g + 2
    assert full["seq"][0].tolist() == [[9, 0, 10], [9, 1, 10]] and short["seq"][0].tolist() == [[9, 0, 10], [9, 0, 10]]
    # group 1: 9 and 10 are penalised once wherever they stand; id 1 at -2.25 against id 0 at -2.0 - 0.5
    assert full["aug"][0].tolist() == [-2.75, ((-0.5 - 0.5) + -2.25) + (-0.25 - 0.5)] and short["aug"][0, 1] == ((-0.5 - 0.5) + -2.5) + (-0.25 - 0.5)
    assert full["aug"][0, 1] > short["aug"][0, 1]
    caps, vals, tie = brute_diverse(x[0], 3, 2, 0.5, (), True, 0)
    assert not tie and caps == full["seq"][0].tolist() and vals == full["aug"][0].tolist()


def _random_rows(rng, S=6, V=11, grid=False):
    if grid:
        return (-rng.integers(0, 9, (1, S, V)) / 4.0).astype(np.float32)
    x = np.log(rng.dirichlet(np.full(V, 0.4), (1, S)) + 1e-30).astype(np.float32)
    for p in range(1, S):                                       # neighbours share leaders: the repeat rule bites
        if rng.random() < 0.5:
            x[0, p] = x[0, p - 1] + (rng.random(V) * 1e-2).astype(np.float32)
    return x


def test_properties_the_header_states():
    """300 images, half of them on a coarse grid (ties inside a row), ids >= 2 words.  Group 0 is the greedy pick, aug[0] and total[0] the same bits; under the repeat
    rule group 0's total is entry 0 of ``nbest_nr_np``, bit for bit, and every caption is valid; lambda = 0 gives N equal rows; a huge lambda gives candidate r = g;
    total is the left-to-right sum of the caption's own x; the first N' groups of the N-set are the N'-set with K held fixed."""
    rng = np.random.default_rng(32)
    S, V, lo = 6, 11, 2
    for case in range(300):
        x = _random_rows(rng, S, V, grid=case % 2 == 0)
        n = int(rng.integers(1, S + 1))
        ban = tuple(int(i) for i in rng.choice(V, 2, replace=False)) if case % 3 == 0 else ()
        lam = (0.25, 0.5, 1.0)[case % 3]
        plain = diverse_np(x, [n], 8, lam, ban)
        greedy = pick_np(x, [n], ban)["seq"][0]
        assert plain["seq"][0, 0].tolist() == greedy.tolist() and same_bits(plain["aug"][0, :1], plain["total"][0, :1]) and plain["count"][0] == 8
        nr = diverse_np(x, [n], 6, lam, ban, True, lo)
        assert nr["count"][0] == 6 and same_bits(nr["total"][0, :1], nbest_nr_np(x, [n], 6, ban, 0, lo)["total"][0, :1]) and same_bits(nr["aug"][0, :1], nr["total"][0, :1])
        for r in (plain, nr):
            for g in range(int(r["count"][0])):
                cap = [int(i) for i in r["seq"][0, g, :n]]
                assert is_valid(cap, ban, lo if r is nr else 10 ** 9)
                t = 0.0
                for p, i in enumerate(cap):
                    t = t + float(x[0, p, i])
                assert t == r["total"][0, g] and r["aug"][0, g] <= r["total"][0, g]
        for no_rep in (False, True):
            z = diverse_np(x, [n], 6, 0.0, ban, no_rep, lo)
            assert (z["seq"][0] == z["seq"][0, :1]).all() and same_bits(z["aug"][0], np.repeat(z["aug"][0, :1], 6)) and same_bits(z["aug"][0], z["total"][0])
            small = diverse_np(x, [n], 3, lam, ban, no_rep, lo, K=8 if no_rep else 6)
            big = diverse_np(x, [n], 6, lam, ban, no_rep, lo, K=8 if no_rep else 6)
            assert np.array_equal(big["seq"][0, :3], small["seq"][0]) and same_bits(big["aug"][0, :3], small["aug"][0]) and same_bits(big["total"][0, :3], small["total"][0])
        huge = diverse_np(x, [n], 8, 1e6, ban)
        for p in range(n):
            order = order_np(x[0, p], ban)[:8]
            assert huge["seq"][0, :len(order), p].tolist() == order.tolist()


def test_degenerate_empty_and_impossible_images():
    """A NaN or an infinity leads a live row, or every id is banned: count 1, the rows' first unbanned ids, total = aug = NaN.  n = 0: one empty caption of 0.0.  Two
    adjacent rows with one candidate each, the same word: count 0 under the repeat rule, N captions without it.  A non-finite entry at rank >= 1 is no candidate."""
    d = np.full((3, 2, 4), -1.0, np.float32)
    d[:, :, 2] = -0.5
    d[0, 1, 3] = NAN
    d[1, 0, :] = -INF
    for nr in (False, True):
        q = diverse_np(d, [2, 2, 2], 2, 0.5, pad=9, no_repeat=nr, repeat_min_id=0)
        assert q["degenerate"].tolist() == [True, True, False] and q["seq"][0, 0].tolist() == [2, 3] and q["seq"][1, 0].tolist() == [0, 2]
        assert np.isnan(q["total"][:2, 0]).all() and np.isnan(q["aug"][:2, 0]).all() and (q["total"][:2, 1] == -INF).all() and (q["aug"][:2, 1] == -INF).all()
        assert (q["seq"][:2, 1] == 9).all() and q["count"].tolist() == [1, 1, 2]
        allb = diverse_np(d[2:], [2], 2, 0.5, ban=(0, 1, 2, 3), pad=9, no_repeat=nr)
        assert allb["degenerate"][0] and allb["seq"][0, 0].tolist() == [9, 9] and allb["count"].tolist() == [1]
        e = diverse_np(d[2:], [0], 3, 0.5, pad=5, no_repeat=nr)
        assert e["count"].tolist() == [1] and e["total"][0].tolist() == [0.0, -INF, -INF] and e["aug"][0].tolist() == [0.0, -INF, -INF] and (e["seq"] == 5).all()
    assert diverse_np(d[2:], [2], 2, 0.5, repeat_min_id=0)["seq"][0].tolist() == [[2, 2], [2, 2]]       # -0.5 - 0.5 ties with id 0's -1.0: the lower r keeps id 2
    assert diverse_np(d[2:], [2], 2, 0.5, no_repeat=True, repeat_min_id=0)["seq"][0].tolist() == [[0, 2], [2, 0]]
    y = np.full((1, 3, 10), -INF, np.float32)
    y[0, 0, 8] = y[0, 1, 8] = -1.0
    y[0, 2] = -np.arange(10, dtype=np.float32) / 4.0
    z = diverse_np(y, [3], 3, 0.5, pad=5, no_repeat=True)
    assert z["count"].tolist() == [0] and (z["seq"] == 5).all() and (z["total"] == -INF).all() and (z["aug"] == -INF).all() and not z["degenerate"][0]
    w = diverse_np(y, [3], 3, 0.5, pad=5)
    # rows 0 and 1 have ONE candidate (-inf at rank >= 1 is none), taken at any penalty; row 2: g1 has id 0 at -0.5 against id 1 at -0.25; g2 has id 0 at -0.5, id 1 at
    # -0.75, id 2 at -0.5: the tie goes to the lower r
    assert w["count"].tolist() == [3] and w["seq"][0].tolist() == [[8, 8, 0], [8, 8, 1], [8, 8, 0]]
    assert w["aug"][0].tolist() == [-2.0, -3.25, -4.5] and w["total"][0].tolist() == [-2.0, -2.25, -2.0]


def _lib():
    from boficap_amd import hip
    assert os.path.exists(hip.LIB_PATH), "build the library first (python -m boficap_amd.build)"
    return hip, hip.lib()


def test_declarations_agree():
    from boficap_amd import build, hip
    header = open(os.path.join(ROOT, "include", "boficap_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    found = re.findall(r"\bbofi_vocab_diverse\s*\(([^;{]*?)\)\s*;", code, flags=re.S)
    assert len(found) == 1 and found[0].count(",") + 1 == len(hip.SIGNATURES["bofi_vocab_diverse"][1]) == 20
    assert hip.SIGNATURES["bofi_vocab_diverse"][1][10] is C.c_double and "double lambda" in found[0]
    assert int(re.search(r"#define\s+BOFI_DIVERSE_MAX\s+(\d+)", code).group(1)) == hip.DIVERSE_MAX == 8
    assert int(re.search(r"#define\s+BOFI_DIVERSE_NR_MAX\s+(\d+)", code).group(1)) == hip.DIVERSE_NR_MAX == 6
    assert C.sizeof(hip.BofiCallOpts) == 128 and hip.ABI_VERSION == 5
    kernels = open(os.path.join(build.CSRC, "bofi_kernels.h")).read()
    assert "launch_vocab_diverse" in kernels and "vocab_diverse_check" in kernels
    for stated in ("pen[k] = lambda * (double)k", "ON THE HOST", "ties to the lowest r'", "K = N + 2 with no_repeat = 1", "g + 2 candidates are not enough",
                   "bofi_vocab_nbest_workspace(rows) bytes: there is no query of its own", "need not be pairwise different"):
        assert stated in header, stated
    _, lib = _lib()
    assert hasattr(lib, "bofi_vocab_diverse") and callable(hip.vocab_diverse) and lib.bofi_abi_version() == 5


def test_entry_point_refuses_bad_arguments_without_a_device():
    """Each returns BOFI_ERR_ARG (1) from the argument check, with a message "vocab_diverse: ...": the pointers are never read, nothing is launched.  rows = 0 is
    BOFI_OK."""
    hip, lib = _lib()
    p = C.c_void_p(0x1000)
    need = lib.bofi_vocab_nbest_workspace(40)
    good = dict(x=p, ldx=9491, rows=40, V=9491, S=20, ntok=None, ntok_bias=0, pad=0, ban=None, N=5, lam=0.5, nr=0, lo=7, seq_n=p, total=p, aug=p, count=p, work=p,
                work_bytes=need)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.bofi_vocab_diverse(a["x"], a["ldx"], a["rows"], a["V"], a["S"], a["ntok"], a["ntok_bias"], a["pad"], a["ban"], a["N"], a["lam"], a["nr"], a["lo"],
                                    a["seq_n"], a["total"], a["aug"], a["count"], a["work"], a["work_bytes"], None)
        if rc == 1:
            assert lib.bofi_last_error().startswith(b"vocab_diverse: "), (kw, lib.bofi_last_error())
        return rc

    assert call(x=None) == 1 and call(seq_n=None) == 1 and call(total=None) == 1 and call(aug=None) == 1 and call(count=None) == 1
    assert call(rows=41) == 1 and call(rows=-20) == 1 and call(V=1) == 1 and call(ldx=9490) == 1
    assert call(S=0, rows=0) == 1 and call(S=65, rows=65) == 1 and b"S in 1..64" in lib.bofi_last_error()
    assert call(N=0) == 1 and call(N=9) == 1 and b"N in 1..8" in lib.bofi_last_error() and call(N=-1) == 1
    assert call(N=7, nr=1) == 1 and b"N in 1..6" in lib.bofi_last_error() and call(N=8, nr=1) == 1
    for lam in (-0.5, NAN, INF, -INF):
        assert call(lam=lam) == 1 and b"lambda" in lib.bofi_last_error(), lam
    assert call(nr=2) == 1 and b"no_repeat" in lib.bofi_last_error() and call(nr=-1) == 1
    assert call(lo=-1) == 1 and b"repeat_min_id" in lib.bofi_last_error() and call(lo=-1, nr=1) == 1
    assert call(work=None) == 1 and call(work_bytes=need - 1) == 1 and call(work_bytes=-1) == 1 and b"workspace" in lib.bofi_last_error()
    assert call(rows=0) == 0 and call(rows=0, work=None, work_bytes=0, S=64, N=6, nr=1, lo=0, lam=0.0) == 0 and call(rows=0, N=8, lam=1e300) == 0


def test_engine_keywords_are_validated_on_the_host():
    from boficap_amd import hip
    from boficap_amd.engine import DIVERSE_KEYS, BofiEngine
    opt = BofiEngine._diverse_options
    assert opt(None) is None and opt(0) is None and opt(False, 0.5, False) is None
    assert opt(4) == (4, 0.5, False, 0) and opt(8, 0.0) == (8, 0.0, False, 0) and opt(6, 2, True, 3) == (6, 2.0, True, 3)
    assert DIVERSE_KEYS == ("diverse_seq", "diverse_logp", "diverse_aug", "diverse_count")
    with pytest.raises(hip.BofiHipError, match="needs diverse") as e:
        opt(0, 0.5, True)
    assert "diverse_no_repeat" in str(e.value)
    for bad, nr, word in ((9, False, r"1\.\.8"), (-1, False, r"1\.\.8"), (7, True, r"1\.\.6"), (8, True, r"1\.\.6")):
        with pytest.raises(hip.BofiHipError, match=word) as e:
            opt(bad, 0.5, nr)
        assert "diverse" in str(e.value)
    for lam in (-1.0, NAN, INF):
        with pytest.raises(hip.BofiHipError, match="lambda") as e:
            opt(3, lam)
        assert "diverse" in str(e.value)
    with pytest.raises(hip.BofiHipError, match="repeat_min_id"):
        opt(3, 0.5, True, -1)
    ref = BofiEngine._diverse_refusals
    for args, word in (((True, 0, False, False, False, False, True), "ids_only"), ((False, 1, False, False, False, False, True), "mask_predict"),
                       ((False, 0, True, False, False, False, True), "no_repeat"), ((False, 0, False, True, False, False, True), "block_trigrams"),
                       ((False, 0, False, False, True, False, True), "require_"), ((False, 0, False, False, False, True, True), "nbest")):
        with pytest.raises(hip.BofiHipError, match=word) as e:
            ref(None, *args)
        assert str(e.value).startswith("diverse")
    ref(None, False, 0, False, False, False, False, True)


def test_eval_options_resolve_and_refuse():
    from boficap_amd import eval_utils as E
    assert E.SAMPLE_N_METHODS == ("sample", "nbest", "diverse")
    assert E.sample_n_method_of({"sample_n_method": "diverse"}, "NAIC", 8) == "diverse" and E.sample_n_method_of({"sample_n_method": "diverse"}, "SAIC", 1) == "diverse"
    for kw, mode, n, word in (({}, "SAIC", 3, "NAIC"), ({}, "NAIC", 9, "at most 8"), ({"refine_method": "mask_predict"}, "NAIC", 3, "mask_predict"),
                              ({"decoding_constraint": 1}, "NAIC", 3, "decoding_constraint"), ({"block_trigrams": 1}, "NAIC", 3, "block_trigrams")):
        with pytest.raises(ValueError, match=word) as e:
            E.sample_n_method_of(dict(kw, sample_n_method="diverse"), mode, n)
        assert "'diverse'" in str(e.value)
    with pytest.raises(ValueError, match="'sample'.*'nbest'.*'diverse'"):
        E.sample_n_method_of({"sample_n_method": "bs"}, "NAIC", 3)
    with pytest.raises(ValueError, match="'sample' and 'nbest'.*'diverse'"):
        E.sample_n_predictions(None, [], 3, method="dbs")
    assert E.diverse_options_of({}) == (0.5, False) and E.diverse_options_of({"diversity_lambda": 0.3}, 5) == (0.3, False)
    assert E.diverse_options_of({"sample_n_method": "diverse"}, 8) == (0.5, False)
    assert E.diverse_options_of({"sample_n_method": "diverse", "diversity_lambda": 2, "diverse_no_repeat": 1}, 6) == (2.0, True)
    for kw, n, word in (({"diverse_no_repeat": 1}, 3, "sample_n_method"), ({"sample_n_method": "nbest", "diverse_no_repeat": 1}, 3, "sample_n_method"),
                        ({"sample_n_method": "diverse", "diverse_no_repeat": 1}, 7, "at most 6"), ({"sample_n_method": "diverse", "diverse_no_repeat": 2}, 3, "0 or 1"),
                        ({"sample_n_method": "diverse", "diversity_lambda": -0.5}, 3, "diversity_lambda"),
                        ({"sample_n_method": "diverse", "diversity_lambda": NAN}, 3, "diversity_lambda"),
                        ({"sample_n_method": "diverse", "diversity_lambda": INF}, 3, "diversity_lambda")):
        with pytest.raises(ValueError, match=word):
            E.diverse_options_of(kw, n)
    # banned words go with the set as with the list; a rule that couples neighbours does not; required words stay with greedy picks
    vocab = {"0": "UNK", "9": "dog"}
    assert E.constraint_of({"suppress_UNK": 1, "sample_n_method": "diverse"}, vocab, "NAIC", 3) == {"ban_ids": [0], "no_repeat": False}
    with pytest.raises(ValueError, match="'diverse' takes suppress_UNK / ban_words only"):
        E.constraint_of({"decoding_constraint": 1, "sample_n_method": "diverse"}, vocab, "NAIC", 3)
    with pytest.raises(ValueError, match="sample_n > 1"):
        E.required_of({"require_words": "dog", "sample_n_method": "diverse"}, vocab, [0], "NAIC", 3)


@pytest.mark.parametrize("args,word", [(["--sample_n_method", "bs", "--sample_n", "3"], "invalid choice"),
                                       (["--sample_n_method", "diverse", "--sample_n", "9"], "at most 8"),
                                       (["--sample_n_method", "diverse", "--sample_n", "3", "--inference_mode", "SAIC"], "NAIC"),
                                       (["--sample_n_method", "diverse", "--sample_n", "3", "--decoding_constraint", "1"], "decoding_constraint"),
                                       (["--sample_n_method", "diverse", "--sample_n", "3", "--refine_rounds", "1", "--refine_method", "mask_predict"], "mask_predict"),
                                       (["--sample_n_method", "diverse", "--sample_n", "3", "--require_words", "dog"], "require_words"),
                                       (["--sample_n_method", "diverse", "--sample_n", "7", "--diverse_no_repeat", "1"], "at most 6"),
                                       (["--sample_n_method", "diverse", "--sample_n", "3", "--diversity_lambda", "-1"], "diversity_lambda"),
                                       (["--sample_n_method", "diverse", "--sample_n", "3", "--diverse_no_repeat", "2"], "invalid choice"),
                                       (["--sample_n_method", "nbest", "--sample_n", "3", "--diverse_no_repeat", "1"], "diverse_no_repeat")])
def test_eval_tool_refuses_the_method_where_it_cannot_apply(args, word):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval.py"), *args, "--synthetic", "8"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 2 and word in r.stderr, r.stderr
