"""Required phrases of the NAIC decode, host side (no GPU): the rule of ``bofi_vocab_require_units`` (include/boficap_hip.h states it in words) RESTATED in numpy
(``require_units_np``: classification, span gains, the backward recurrence in float64 over spans, the forward walk), held against a hand-worked case, against a BRUTE
FORCE over every placement of non-overlapping spans, and -- with units of length 1 -- against ``require_np`` of tests/test_required_words.py; the host table, the
declarations, and the refusals that need no device.  tests/test_gpu_required_phrases.py holds the kernel and the engine to ``require_units_np``."""
import ctypes as C
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_required_words import KEEP, _Eng, _lib, _random_case, require_np

NAN, INF = float("nan"), float("inf")


# ----------------------------------------------------------------------------- the rule, restated
def classify_units_np(row, V, ban=(), no_repeat=False, min_id=7):
    """The units of one image's table [K, L]: the id list of a kept unit, -1 for an empty one, -2 for a skipped one."""
    ban = {int(i) for i in ban}
    raw = []
    for u in row:
        ids = []
        for v in u:
            if int(v) < 0:
                break                                            # (entries after the first negative id are not read)
            ids.append(int(v))
        raw.append(ids)
    out = []
    for j, u in enumerate(raw):
        if not u:
            out.append(-1)
            continue
        bad = any(w >= V or w in ban for w in u) or u in raw[:j]
        if not bad and no_repeat:
            bad = any(a == b and a >= min_id for a, b in zip(u, u[1:]))
            for v in out[:j]:                                    # an earlier KEPT unit it could meet at a shared word
                if isinstance(v, list) and ((u[0] >= min_id and u[0] == v[-1]) or (u[-1] >= min_id and u[-1] == v[0])):
                    bad = True
        out.append(-2 if bad else u)
    return out


def spans_np(x, n, f, seq, no_repeat=False, min_id=7):
    """gain float64 [n, K] and eligible bool [n, K] of "unit j starts at p" for one image: x [S, V], f the classified units, seq the ids on entry."""
    V, K = x.shape[1], len(f)
    gain, ok = np.zeros((n, K), np.float64), np.zeros((n, K), bool)
    for p in range(n):
        for j, u in enumerate(f):
            if not isinstance(u, list) or p + len(u) > n:
                continue
            g, good = np.float64(0.0), True
            for i, w in enumerate(u):
                here = int(seq[p + i])
                if here == w:
                    continue
                a = np.float64(x[p + i, w])
                b = np.float64(x[p + i, here]) if 0 <= here < V else np.float64(NAN)
                if np.isfinite(a) and np.isfinite(b):
                    g = g + (a - b)                              # left to right
                else:
                    good = False
            if no_repeat:
                e = p + len(u)
                if u[0] >= min_id and int(seq[p]) != u[0] and p > 0 and int(seq[p - 1]) == u[0]:
                    good = False
                if u[-1] >= min_id and int(seq[e - 1]) != u[-1] and e < n and int(seq[e]) == u[-1]:
                    good = False
            if good:
                gain[p, j], ok[p, j] = g, True
    return gain, ok


def require_units_np(x, n, units, seq, ban=(), no_repeat=False, min_id=7, chosen=None):
    """``bofi_vocab_require_units`` on x [B, S, V] with n [B] live positions (clamped to 0 .. S), units int [B, K, L] and the ids on entry seq [B, S]: a dict of ``seq``
    int64 [B, S], ``chosen`` float32 [B, S] (x at every span position; what ``chosen`` held -- zeros without it -- elsewhere), ``pos`` int32 [B, K] (start positions),
    ``moved`` int32 [B] and ``margin`` float64 [B]: the smallest gap, along the forward walk, between the chosen option's value and the next-best option's -- inf where
    their counts differ or where there was one option, else the difference of the totals."""
    x, units = np.asarray(x), np.asarray(units)
    B, S, V = x.shape
    K = units.shape[1]
    out = np.array(seq, np.int64, copy=True)
    ch = np.zeros((B, S), np.float32) if chosen is None else np.array(chosen, np.float32, copy=True)
    pos = np.zeros((B, K), np.int32)
    moved = np.zeros(B, np.int32)
    margin = np.full(B, INF)
    M = 1 << K
    for b in range(B):
        nb = min(max(int(n[b]), 0), S)
        f = classify_units_np(units[b], V, ban, no_repeat, min_id)
        gain, ok = spans_np(x[b], nb, f, out[b], no_repeat, min_id)
        cnt = np.zeros((nb + 1, M), np.int64)
        tot = np.zeros((nb + 1, M), np.float64)
        opts = [[None] * M for _ in range(nb)]
        choice = np.full((nb, M), KEEP, np.int64)
        for p in range(nb - 1, -1, -1):
            for m in range(M):
                o = [(j, 1 + cnt[p + len(f[j]), m ^ (1 << j)], gain[p, j] + tot[p + len(f[j]), m ^ (1 << j)]) for j in range(K) if (m >> j) & 1 and ok[p, j]]
                o.append((KEEP, cnt[p + 1, m], tot[p + 1, m]))
                best = o[0]
                for c in o[1:]:
                    if c[1] > best[1] or (c[1] == best[1] and c[2] > best[2]):      # strictly greater only: the first best option stays
                        best = c
                opts[p][m] = o
                choice[p, m], cnt[p, m], tot[p, m] = best
        m = sum(1 << j for j, u in enumerate(f) if isinstance(u, list))
        pos[b] = [-3 if isinstance(u, list) else u for u in f]
        p = 0
        while p < nb and m:
            o, c = opts[p][m], int(choice[p, m])
            mine = next(v for v in o if v[0] == c)
            for v in o:
                if v[0] != c:
                    margin[b] = min(margin[b], INF if v[1] != mine[1] else float(mine[2] - v[2]))
            if c == KEEP:
                p += 1
                continue
            pos[b, c] = p
            for i, w in enumerate(f[c]):
                moved[b] += int(out[b, p + i] != w)
                out[b, p + i], ch[b, p + i] = w, x[b, p + i, w]
            m ^= 1 << c
            p += len(f[c])
    return dict(seq=out, chosen=ch, pos=pos, moved=moved, margin=margin)


def brute_units_np(x, n, f, seq, no_repeat=False, min_id=7):
    """The placement of one image WITHOUT a recurrence: every choice of a start position (or none) for every kept unit -- every subset, every order -- whose spans are
    eligible and do not overlap, preferred first by the number of units placed, then by the total gain (the inputs are multiples of 2^-3: every sum is exact in any
    order), then by the decisions read left to right: at a position that no earlier span covers, taking a unit (the earliest-listed first) over keeping the id.
    Returns the start of every kept unit (None: not placed)."""
    gain, ok = spans_np(x, n, f, seq, no_repeat, min_id)
    req = [j for j, u in enumerate(f) if isinstance(u, list)]
    best, best_key = None, None
    for where in itertools.product([None] + list(range(n)), repeat=len(req)):
        placed = [(p, j) for j, p in zip(req, where) if p is not None]
        if any(p + len(f[j]) > n or not ok[p, j] for p, j in placed):
            continue
        covered = [q for p, j in placed for q in range(p, p + len(f[j]))]
        if len(set(covered)) != len(covered):
            continue
        total = sum(gain[p, j] for p, j in placed)
        start = dict(placed)
        decisions, p = [], 0
        while p < n:
            if p in start:
                decisions.append(start[p])
                p += len(f[start[p]])
            else:
                decisions.append(len(f))
                p += 1
        key = (-len(placed), -total, decisions)
        if best_key is None or key < best_key:
            best, best_key = dict(zip(req, where)), key
    return best


# ----------------------------------------------------------------------------- tests
def _hand_case():
    S, V = 6, 12
    x = np.full((4, S, V), -4.0, np.float32)
    seq = np.array([[9, 9, 8, 3, 5, 5], [9, 10, 9, 5, 5, 5], [9, 5, 5, 5, 5, 5], [9, 9, 9, 9, 5, 5]], np.int64)
    for b in range(4):
        for p in range(S):
            x[b, p, seq[b, p]] = -0.5                           # every standing id at -0.5
    x[0, :5, 10] = [-1.0, -0.75, -2.0, -0.75, -4.0]
    x[0, :5, 11] = [-4.0, -1.0, -0.75, -1.5, -0.75]
    x[0, :5, 8] = [-3.0, -3.0, -0.5, -3.0, -3.0]
    x[1, 0, 10], x[1, 1, 9], x[1, 2, 10], x[1, 3, 9] = -1.0, -0.75, -1.5, -4.0
    x[3, :4, 10] = x[3, :4, 8] = x[3, :4, 11] = -1.0
    units = np.array([[[10, 11], [8, -1], [-1, -1], [-1, -1]],
                      [[10, 9], [-1, -1], [-1, -1], [-1, -1]],
                      [[10, 11], [7, 7], [-1, 5], [10, 11]],
                      [[10, 8], [8, 11], [-1, -1], [-1, -1]]], np.int32)
    return x, [5, 4, 1, 4], units, seq


def test_require_units_np_on_a_hand_worked_case():
    """S = 6, V = 12, K = 4, L = 2; every standing id has -0.5; worked by hand.

    Image 0, n = 5, seq 9 9 8 3 5, units A = (10 11) and B = (8).  x[., 10] = -1 -.75 -2 -.75 -4, x[., 11] = -4 -1 -.75 -1.5 -.75, so A gains (-.5) + (-.5) = -1 at 0,
    (-.25) + (-.25) = -.5 at 1, -1.5 - .25... = (-1.5) + (-1) = -2.5 at 2, (-.25) + (-.25) = -.5 at 3, and does not fit at 4.  B stands at 2 (0 there, -2.5 elsewhere).
    Both placed: A@3 B@2 = -.5; A@0 B@2 = -1; A@1 covers position 2, so B moves: -.5 - 2.5 = -3.  Walk: position 0 keeps (-.5 against A@0: -1, gap .5; B@0: -3);
    position 1 keeps (-.5 against -3 and -3); position 2 takes B (A@2: -2.5 + B@4 -2.5 = -5); position 3 takes A.  9 9 8 10 11 | pos 3 2 | moved 2 | margin .5.
    Image 1, n = 4, seq 9 10 9 5, unit (10 9), which stands at 1.  At 0: (-1 + .5) + (-.75 + .5) = -.75; at 1: 0; at 2: (-1.5 + .5) + (-4 + .5) = -4.5.  Position 0
    keeps (0 against -.75), position 1 takes it: nothing moves, pos 1, margin .75.  With no_repeat the span at 0 would put 9 next to the 9 at 2, the span at 2 would put
    10 next to the 10 at 1: one option is left, margin inf.
    Image 2, n = 1: (10 11) does not fit: -3.  (7 7) does not fit either, and under no_repeat it is skipped for repeating a word; (-1 5) is empty (what follows the first
    negative id is not read); the second (10 11) repeats the first: -2.
    Image 3, n = 4, seq 9 9 9 9, units (10 8) and (8 11), every word at -1: each span costs -1 wherever it goes.  Both fit only as 0-1 and 2-3: position 0 takes the
    first-listed unit (a tie with the other order: margin 0): 10 8 8 11, moved 4.  Under no_repeat the second unit could meet the first at 8 8: it is skipped, and the
    first takes position 0 (a tie with keeping: margin 0)."""
    x, n, units, seq = _hand_case()
    r = require_units_np(x, n, units, seq)
    assert r["seq"].tolist() == [[9, 9, 8, 10, 11, 5], [9, 10, 9, 5, 5, 5], [9, 5, 5, 5, 5, 5], [10, 8, 8, 11, 5, 5]]
    assert r["pos"].tolist() == [[3, 2, -1, -1], [1, -1, -1, -1], [-3, -3, -1, -2], [0, 2, -1, -1]]
    assert r["moved"].tolist() == [2, 0, 0, 4]
    assert r["margin"].tolist() == [0.5, 0.75, INF, 0.0]
    want = np.zeros((4, 6), np.float32)
    want[0, 2:5] = [-0.5, -0.75, -0.75]
    want[1, 1:3] = [-0.5, -0.5]
    want[3, :4] = -1.0
    assert np.array_equal(r["chosen"], want)
    rep = require_units_np(x, n, units, seq, no_repeat=True, chosen=np.full((4, 6), 7.0, np.float32))
    assert rep["seq"].tolist() == [[9, 9, 8, 10, 11, 5], [9, 10, 9, 5, 5, 5], [9, 5, 5, 5, 5, 5], [10, 8, 9, 9, 5, 5]]
    assert rep["pos"].tolist() == [[3, 2, -1, -1], [1, -1, -1, -1], [-3, -2, -1, -2], [0, -2, -1, -1]]
    assert rep["margin"].tolist() == [0.5, INF, INF, 0.0] and rep["moved"].tolist() == [2, 0, 0, 2]
    assert rep["chosen"][0].tolist() == [7.0, 7.0, -0.5, -0.75, -0.75, 7.0]      # (what stood in row_chosen stays where no unit was placed)
    ban = require_units_np(x, n, units, seq, ban=[11])             # a banned id skips the whole unit
    assert ban["pos"].tolist() == [[-2, 2, -1, -1], [1, -1, -1, -1], [-2, -3, -1, -2], [0, -2, -1, -1]] and ban["seq"][0].tolist() == [9, 9, 8, 3, 5, 5]
    assert classify_units_np([[3, 4], [3, 4], [-5, 2], [12, 1], [4, 11], [3, -1], [4, 3]], 12, ban=[11]) == [[3, 4], -2, -1, -2, -2, [3], [4, 3]]
    assert classify_units_np([[8, 9], [9, 5], [5, 6], [3, 3], [8, 8], [3, 8], [6, 3]], 12, no_repeat=True) == [[8, 9], -2, [5, 6], [3, 3], -2, -2, [6, 3]]


def _random_units(rng, K, L, V=16):
    units = rng.integers(5, 12, size=(K, L))                    # around min_id = 7, with shared ids and duplicates
    units[rng.random((K, L)) < 0.2] = -1                        # shorter units, empties, garbage behind a negative id
    units[rng.random((K, L)) < 0.05] = V + 3
    return units.astype(np.int32)


def test_require_units_np_equals_the_brute_force():
    """Every placement of non-overlapping spans enumerated, S <= 7, K <= 3, L <= 3, V = 16; inputs multiples of 2^-3 with NaN and +-inf, ties, units that stand in seq
    already and units that share ids, with and without the adjacency rule and a ban."""
    rng = np.random.default_rng(20261)
    tied = long_placed = standing = barred = skipped_meet = 0
    for it in range(600):
        S, K, L = int(rng.integers(3, 8)) if it % 4 else int(rng.integers(1, 3)), int(rng.integers(1, 4)), int(rng.integers(1, 4))
        x, n, _, seq = _random_case(rng, S, K)
        units = _random_units(rng, K, L)
        if it % 3 == 0 and n >= 2 and units[0, 0] >= 0:         # a unit that already stands in seq
            u = [int(v) for v in units[0] if v >= 0] if (units[0] >= 0).all() else [int(units[0, 0])]
            if len(u) <= n and max(u) < 16:
                seq[:len(u)] = u
        rep, ban = bool(it & 1), ([int(units[0, 0])] if it % 7 == 0 and 0 <= units[0, 0] < 16 else [])
        r = require_units_np(x[None], [n], units[None], seq[None], ban=ban, no_repeat=rep)
        f = classify_units_np(units, 16, ban, rep)
        want = brute_units_np(x, n, f, seq, rep)
        got = {j: (int(r["pos"][0, j]) if r["pos"][0, j] >= 0 else None) for j, u in enumerate(f) if isinstance(u, list)}
        assert got == want, (it, S, K, L, n, units, seq, rep, ban)
        assert [int(v) for j, v in enumerate(r["pos"][0]) if not isinstance(f[j], list)] == [u for u in f if not isinstance(u, list)]
        after = seq.copy()
        for j, p in want.items():
            if p is not None:
                standing += int(list(seq[p:p + len(f[j])]) == f[j])
                long_placed += int(len(f[j]) > 1)
                after[p:p + len(f[j])] = f[j]
        assert np.array_equal(r["seq"][0], after) and r["moved"][0] == int((after != seq).sum())
        tied += int(r["margin"][0] == 0.0)
        if rep:
            free = classify_units_np(units, 16, ban, False)
            skipped_meet += sum(1 for a, b in zip(free, f) if isinstance(a, list) and b == -2)
            _, ok_free = spans_np(x, min(n, S), f, seq, False)
            _, ok_rep = spans_np(x, min(n, S), f, seq, True)
            barred += int((ok_free & ~ok_rep).sum())
            for p in range(1, n):                                # a placement never creates an adjacent repeat of a word
                assert not (after[p] == after[p - 1] and after[p] >= 7 and (after[p] != seq[p] or after[p - 1] != seq[p - 1])), (it, seq, after, f)
    print(f"tied {tied}, units of two or more ids placed {long_placed}, placed where they stood {standing}, spans barred by the adjacency rule {barred}, "
          f"units skipped under no_repeat {skipped_meet}")
    assert tied >= 60 and long_placed >= 60 and standing >= 60 and barred >= 60 and skipped_meet >= 30      # the cases are not vacuous


def test_units_of_length_one_are_require_np():
    """With L = 1 -- and with longer tables whose units all have length 1 -- seq, pos, moved, chosen and margin equal ``require_np`` on the random cases of
    tests/test_required_words.py, with and without the adjacency rule and a ban."""
    rng = np.random.default_rng(20260)
    for it in range(300):
        S, K = int(rng.integers(1, 8)), int(rng.integers(1, 4))
        x, n, words, seq = _random_case(rng, S, K)
        rep, ban = bool(it & 1), ([int(words[0])] if it % 7 == 0 and words[0] >= 0 else [])
        keep = np.full((1, S), 3.0, np.float32)
        want = require_np(x[None], [n], words[None], seq[None], ban=ban, no_repeat=rep, chosen=keep)
        for L in (1, 3):
            units = np.full((1, K, L), -1, np.int32)
            units[0, :, 0] = words
            if L == 3:
                units[0, :, 2] = 9                               # (behind the first negative id: not read)
            got = require_units_np(x[None], [n], units, seq[None], ban=ban, no_repeat=rep, chosen=keep)
            for k in ("seq", "pos", "moved", "margin"):
                assert np.array_equal(got[k], want[k]), (it, L, k)
            assert np.array_equal(got["chosen"].view(np.int32), want["chosen"].view(np.int32)), (it, L)


def test_require_unit_table_is_checked_on_the_host():
    from boficap_amd import hip
    t = hip.require_unit_table([[[3, 4], [5]], [], [[6, 7, 8], [6, 7, 8], [], [2]]], 3, 10)
    assert t.dtype == torch.int32 and t.tolist() == [[[3, 4, -1], [5, -1, -1]], [[-1] * 3] * 2, [[6, 7, 8], [2, -1, -1]]]      # (repeated and empty units are dropped)
    assert hip.require_unit_table([[7, 8], [9]], 2, 10).tolist() == [[[7, 8], [9, -1]]] * 2      # one flat list of units: every image
    assert hip.require_unit_table(np.array([[[1, 2], [-1, -1]], [[3, -1], [4, 5]]]), 2, 10).tolist() == [[[1, 2], [-1, -1]], [[3, -1], [4, 5]]]
    assert hip.require_unit_table(torch.tensor([[1, 2], [3, -1]]), 2, 10).tolist() == [[[1, 2], [3, -1]]] * 2
    for off in (None, [], [[], []], [[[]], None]):
        assert hip.require_unit_table(off, 2, 10) is None
    for bad, word in (([[[10]]], "0..9"), ([[[-2, 1]]], "0..9"), ([[[1, 2, 3, 4, 5]]], r"at most 4 ids, got \[1, 2, 3, 4, 5\]"), ([[[i] for i in range(9)]], "at most 8"),
                      ([[[1, 3]]], r"id 3 of unit \[1, 3\] is also in ban_ids"), ([[[1]], [[2]]], "rows"), ([3, 4], "a unit is a list"), ([[3, [4]]], "a unit is a list of ids, got"), ([[[3], 4]], "bare id 4")):
        with pytest.raises(hip.BofiHipError, match=word) as e:
            hip.require_unit_table(bad, 1, 10, ban_ids=[3] if "ban_ids" in word else ())
        assert "require_phrases" in str(e.value)
    # under no_repeat: a unit that repeats a word, and two units that could meet -- both named; neither is refused without the rule, or below repeat_min_id
    with pytest.raises(hip.BofiHipError, match=r"unit \[8, 8, 9\] repeats a word"):
        hip.require_unit_table([[[8, 8, 9]]], 1, 10, no_repeat=True)
    with pytest.raises(hip.BofiHipError, match=r"units \[7, 8\] and \[8, 9\] could meet"):
        hip.require_unit_table([[[7, 8], [8, 9]]], 1, 10, no_repeat=True)
    with pytest.raises(hip.BofiHipError, match=r"units \[8, 9\] and \[7, 8\] could meet"):
        hip.require_unit_table([[[8, 9], [7, 8]]], 1, 10, no_repeat=True)
    assert hip.require_unit_table([[[8, 8, 9], [7, 8], [9, 7]]], 1, 10).shape == (1, 3, 3)
    assert hip.require_unit_table([[[3, 3], [2, 3]]], 1, 10, no_repeat=True).shape == (1, 2, 2)
    assert hip.require_unit_table([[[8, 8]]], 1, 10, no_repeat=True, repeat_min_id=9).shape == (1, 1, 2)
    assert hip.REQUIRE_UNIT_MAX == 4 and hip.REQUIRE_MAX == 8


def test_declarations_agree():
    """The entry point in header, ctypes table, build list and library; BOFI_REQUIRE_UNIT_MAX; the per-call record and the ABI version as they were."""
    from boficap_amd import build, hip
    header = open(os.path.join(ROOT, "include", "boficap_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    found = re.findall(r"\bbofi_vocab_require_units\s*\(([^;{]*?)\)\s*;", code, flags=re.S)
    assert len(found) == 1 and found[0].count(",") + 1 == len(hip.SIGNATURES["bofi_vocab_require_units"][1]) == 18
    assert int(re.search(r"#define\s+BOFI_REQUIRE_UNIT_MAX\s+(\d+)", code).group(1)) == hip.REQUIRE_UNIT_MAX == 4
    assert int(re.search(r"#define\s+BOFI_REQUIRE_MAX\s+(\d+)", code).group(1)) == hip.REQUIRE_MAX == 8
    assert "record stays 128 bytes" in header and C.sizeof(hip.BofiCallOpts) == 128 and hip.ABI_VERSION == 5
    assert "force.hip" in build.SOURCES
    kernels = open(os.path.join(build.CSRC, "bofi_kernels.h")).read()
    assert "launch_vocab_require_units" in kernels and "vocab_require_units_check" in kernels
    assert "vocab_require_units_kernel" in open(os.path.join(build.CSRC, "force.hip")).read()
    _, lib = _lib()
    assert hasattr(lib, "bofi_vocab_require_units") and callable(hip.vocab_require_units) and callable(hip.require_unit_table) and lib.bofi_abi_version() == 5


def test_entry_point_refuses_bad_arguments_without_a_device():
    """Each returns BOFI_ERR_ARG (1) from the argument check, with a message: the pointers are never read, nothing is launched.  rows = 0 is BOFI_OK."""
    hip, lib = _lib()
    p = C.c_void_p(0x1000)
    good = dict(x=p, ldx=9491, rows=40, V=9491, S=20, ntok=None, ntok_bias=0, units=p, K=4, L=2, ban=None, no_repeat=1, min_id=7, seq=p, chosen=None, pos=p, moved=None)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.bofi_vocab_require_units(a["x"], a["ldx"], a["rows"], a["V"], a["S"], a["ntok"], a["ntok_bias"], a["units"], a["K"], a["L"], a["ban"], a["no_repeat"],
                                          a["min_id"], a["seq"], a["chosen"], a["pos"], a["moved"], None)
        if rc == 1:
            assert b"vocab_require_units" in lib.bofi_last_error(), kw
        return rc

    assert call(x=None) == 1 and call(seq=None) == 1 and call(units=None) == 1 and call(pos=None) == 1
    assert call(rows=41) == 1 and call(rows=-20) == 1
    assert call(V=1) == 1 and call(V=0) == 1
    assert call(ldx=9490) == 1
    assert call(S=0, rows=0) == 1 and call(S=65, rows=65) == 1
    assert call(K=0) == 1 and call(K=9) == 1 and b"K in 1..8" in lib.bofi_last_error()
    assert call(L=0) == 1 and call(L=5) == 1 and b"L in 1..4" in lib.bofi_last_error() and call(L=-1) == 1
    assert call(no_repeat=2) == 1 and call(no_repeat=-1) == 1
    assert call(min_id=-1) == 1
    assert call(rows=0) == 0 and call(rows=0, S=64, K=8, L=4) == 0 and call(rows=0, L=1) == 0


def test_engine_keywords_are_validated_on_the_host():
    from boficap_amd import hip
    from boficap_amd.engine import BofiEngine, DecodePipeline
    table = BofiEngine._require_unit_table
    assert table(_Eng, None, 2) is None and table(_Eng, [], 2) is None and table(_Eng, [[], []], 2) is None
    assert table(_Eng, [[3, 4], [5]], 2).tolist() == [[[3, 4], [5, -1]]] * 2
    for bad, ban, rep, word in (([[10]], None, False, "0..9"), ([[1, 2, 3, 4, 5]], None, False, "at most 4"), ([[3, 4]], [3], False, "ban_ids"),
                                ([[[1]]], None, False, "rows"), ([[7, 8], [8, 9]], None, True, "could meet"), ([[8, 8]], None, True, "repeats a word")):
        with pytest.raises(hip.BofiHipError, match=word):
            table(_Eng, bad, 2, ban, rep)
    for args, word in (((True, 0, False), "ids_only"), ((False, hip.FLAG_MASK_PREDICT, False), "mask_predict"), ((False, 0, True), "block_trigrams")):
        with pytest.raises(hip.BofiHipError, match=word) as e:
            BofiEngine._require_refusals(*args, "require_phrases")
        assert "require_phrases" in str(e.value)

    class _E(_Eng):
        _pick_ban = staticmethod(lambda ban_ids, block_trigrams=False: None)
        _require_table, _require_unit_table, _require_refusals = BofiEngine._require_table, BofiEngine._require_unit_table, staticmethod(BofiEngine._require_refusals)
    with pytest.raises(hip.BofiHipError, match="give one"):      # both options: refused before anything else is resolved
        BofiEngine._post_options(_E(), None, False, 7, False, [3], None, False, 2, False, 0, True, [[4, 5]])

    class _Pipe:
        fused_vocab, refine_method, block_trigrams, root_vocab, ban_ids, no_repeat, repeat_min_id = False, "feed_back", False, 10, (3,), True, 7
    split = DecodePipeline._phrase_split
    assert split(_Pipe, None) == (None, None) and split(_Pipe, []) == (None, None)
    assert split(_Pipe, [[4, 5], [6], [4, 5]]) == ([[4, 5], [6]], None)      # one flat list of units
    flat, per_batch = split(_Pipe, [[[[1, 2]]], None])
    assert flat is None and list(per_batch) == [[[[1, 2]]], None]
    for bad, word in (([[3, 4]], "ban_ids"), ([[10]], "0..9"), (np.zeros((2, 2, 2), np.int64), "per-batch"), ([4, 5], "a unit is a list"), ([[7, 8], [8, 9]], "could meet")):
        with pytest.raises(hip.BofiHipError, match=word):
            split(_Pipe, bad)
    for attr, value, word in (("fused_vocab", True, "fused_vocab"), ("refine_method", "mask_predict", "mask_predict"), ("block_trigrams", True, "block_trigrams")):
        P = type("P", (_Pipe,), {attr: value})
        with pytest.raises(hip.BofiHipError, match=word) as e:
            split(P, [[4]])
        assert "require_phrases" in str(e.value)
        assert split(P, None) == (None, None)                   # off: nothing to refuse
    with pytest.raises(hip.BofiHipError, match="give one"):
        DecodePipeline._require_both([4], [[5, 6]])
    DecodePipeline._require_both([4], None), DecodePipeline._require_both([], [[5, 6]]), DecodePipeline._require_both(None, None)


def test_eval_options_resolve_phrases():
    from boficap_amd import eval_utils as E
    vocab = {"7": "a", "8": "fire", "9": "dog", "10": "hydrant", "11": "dog", "12": "hot dog", "13": "hot"}
    keys = [0, 1, 2]
    # no phrase anywhere: single ids through require_ids, as before
    ids, words = E.required_of({"require_words": "dog,a"}, vocab, keys)
    assert ids == [[9, 7]] * 3 and not E.required_phrases(ids)
    # a phrase: the whole evaluation goes through units, single words as units of length 1
    ids, words = E.required_of({"require_words": "fire hydrant,dog,fire hydrant"}, vocab, keys)
    assert ids == [[[8, 10], [9]]] * 3 and words == [["fire hydrant", "dog"]] * 3 and E.required_phrases(ids)
    ids, words = E.required_of({"require_words": {"1": ["a"], 2: "dog a,a"}}, vocab, keys)
    assert ids == [[], [[7]], [[9, 7], [7]]] and words == [[], ["a"], ["dog a", "a"]] and E.required_phrases(ids)
    # a vocabulary entry that equals the whole item wins over splitting
    ids, _ = E.required_of({"require_words": ["hot dog"]}, vocab, keys)
    assert ids == [[12]] * 3 and not E.required_phrases(ids)
    ids, _ = E.required_of({"require_words": ["hot dog", "hot a"]}, vocab, keys)
    assert ids == [[[12], [13, 7]]] * 3
    with pytest.raises(ValueError, match="'cat'") as e:          # the unknown word inside a phrase is named, not the phrase
        E.required_of({"require_words": ["fire cat"]}, vocab, keys)
    assert "fire cat" not in str(e.value)
    with pytest.raises(ValueError, match="1 to 4 words"):
        E.required_of({"require_words": ["a a a a a"]}, vocab, keys)
    with pytest.raises(ValueError, match="'hydrant' is also banned"):
        E.required_of({"require_words": ["fire hydrant"]}, vocab, keys, ban_ids=[10])
    with pytest.raises(ValueError, match="at most 8"):
        E.required_of({"require_words": ["a dog"] + [f"{i} a" for i in range(8)]}, dict(vocab, **{str(20 + i): str(i) for i in range(8)}), keys)
    for kw, mode, n, word in (({}, "SAIC", 1, "NAIC"), ({"fused_vocab": True}, "NAIC", 1, "fused_vocab"), ({"refine_method": "mask_predict"}, "NAIC", 1, "mask_predict"),
                              ({}, "NAIC", 5, "sample_n"), ({"block_trigrams": 1}, "NAIC", 1, "block_trigrams")):
        with pytest.raises(ValueError, match=word) as e:
            E.required_of(dict(kw, require_words=["fire hydrant"]), vocab, keys, mode, n)
        assert "require_words" in str(e.value)
    # under decoding_constraint: what the unit table would refuse, in the items' own words
    with pytest.raises(ValueError, match="'fire hydrant' and 'hydrant a' could meet"):
        E.required_of({"require_words": "fire hydrant,hydrant a", "decoding_constraint": 1}, vocab, keys)
    with pytest.raises(ValueError, match="'fire fire' repeats a word"):
        E.required_of({"require_words": "fire fire", "decoding_constraint": 1}, vocab, keys)
    assert E.required_of({"require_words": "fire hydrant,hydrant a"}, vocab, keys)[0] == [[[8, 10], [10, 7]]] * 3
    # 'required' holds [phrase, start position or None]; required_rate counts units
    pos = torch.tensor([[3, -3, -1], [-3, 0, 5]], dtype=torch.int32)
    assert E.required_entry(["fire hydrant", "dog"], pos[0]) == [["fire hydrant", 3], ["dog", None]]
    assert E.required_rates([["fire hydrant", "dog"], ["a", "dog a", "hot a"]], list(pos), 3, 12) == {"required_rate": 3 / 5, "required_moved_rate": 0.25}


@pytest.mark.parametrize("args,word", [(["--require_words", "fire hydrant", "--inference_mode", "SAIC"], "NAIC"), (["--require_words", "fire hydrant,dog", "--fused_vocab"], "fused_vocab"),
                                       (["--require_words", "a b", "--refine_rounds", "2", "--refine_method", "mask_predict"], "mask_predict"),
                                       (["--require_words", "a b", "--sample_n", "3"], "sample_n"), (["--require_words", "a b", "--block_trigrams", "1"], "block_trigrams")])
def test_eval_tool_refuses_required_phrases_where_they_cannot_apply(args, word):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval.py"), *args, "--synthetic", "8"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 2 and "--require_words" in r.stderr and word in r.stderr, r.stderr[-400:]


def test_eval_tool_help_says_phrases_are_accepted():
    text = open(os.path.join(ROOT, "tools", "eval.py")).read()
    assert "fire hydrant" in text and "phrase" in re.search(r'"--require_words",.*?\)\n', text, flags=re.S).group(0)
