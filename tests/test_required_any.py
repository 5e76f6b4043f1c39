"""Required alternatives of the NAIC decode, host side (no GPU): the rule of ``bofi_vocab_require_any`` (include/boficap_hip.h states it in words) RESTATED in numpy
(``require_any_np``: classification of the slots, span gains through ``spans_np`` of tests/test_required_phrases.py, the backward recurrence in float64 over masks of
GROUPS with one option per kept slot, the forward walk with its margin), held against hand-worked cases, against a BRUTE FORCE over every assignment, and -- with one
alternative per group -- against ``require_units_np``; the host table, the ``|`` items of the evaluation, the declarations, and the refusals that need no device.
tests/test_gpu_required_any.py holds the kernel and the engine to ``require_any_np``."""
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
from test_required_phrases import _random_units, require_units_np, spans_np
from test_required_words import KEEP, _Eng, _lib, _random_case

NAN, INF = float("nan"), float("inf")


# ----------------------------------------------------------------------------- the rule, restated
def classify_any_np(table, V, ban=(), no_repeat=False, min_id=7):
    """The slots of one image's table [K, A, L], in slot order c = j * A + a: the id list of a kept slot, -1 for an empty one, -2 for a skipped one."""
    table = np.asarray(table)
    K, A, _ = table.shape
    ban = {int(i) for i in ban}
    raw = []
    for u in table.reshape(K * A, -1):
        ids = []
        for v in u:
            if int(v) < 0:
                break                                            # (entries after the first negative id are not read)
            ids.append(int(v))
        raw.append(ids)
    out = []
    for c, u in enumerate(raw):
        if not u:
            out.append(-1)
            continue
        bad = any(w >= V or w in ban for w in u) or u in raw[:c]      # (equal to an earlier slot of any group, kept or not)
        if not bad and no_repeat:
            bad = any(a == b and a >= min_id for a, b in zip(u, u[1:]))
            for v in out[:(c // A) * A]:                         # an earlier KEPT slot of ANOTHER group it could meet at a shared word
                if isinstance(v, list) and ((u[0] >= min_id and u[0] == v[-1]) or (u[-1] >= min_id and u[-1] == v[0])):
                    bad = True
        out.append(-2 if bad else u)
    return out


def group_codes(f, K, A):
    """Per group: -3 kept (at least one kept slot), -2 no slot kept and at least one skipped, -1 every slot empty."""
    out = []
    for j in range(K):
        mine = f[j * A:(j + 1) * A]
        out.append(-3 if any(isinstance(u, list) for u in mine) else -2 if any(u == -2 for u in mine) else -1)
    return out


def require_any_np(x, n, alts, seq, ban=(), no_repeat=False, min_id=7, chosen=None):
    """``bofi_vocab_require_any`` on x [B, S, V] with n [B] live positions (clamped to 0 .. S), alts int [B, K, A, L] and the ids on entry seq [B, S]: a dict of ``seq``
    int64 [B, S], ``chosen`` float32 [B, S] (x at every span position; what ``chosen`` held -- zeros without it -- elsewhere), ``pos`` int32 [B, K] (start of the group's
    placed alternative, or its code), ``which`` int32 [B, K] (the alternative's index, -1 not placed), ``moved`` int32 [B] and ``margin`` float64 [B]: the smallest gap,
    along the forward walk, between the chosen option's value and every other option's -- inf where their counts differ or where there was one option, else the
    difference of the totals (``require_units_np``'s margin)."""
    x, alts = np.asarray(x), np.asarray(alts)
    B, S, V = x.shape
    K, A = alts.shape[1], alts.shape[2]
    out = np.array(seq, np.int64, copy=True)
    ch = np.zeros((B, S), np.float32) if chosen is None else np.array(chosen, np.float32, copy=True)
    pos, which = np.zeros((B, K), np.int32), np.full((B, K), -1, np.int32)
    moved = np.zeros(B, np.int32)
    margin = np.full(B, INF)
    M = 1 << K
    for b in range(B):
        nb = min(max(int(n[b]), 0), S)
        f = classify_any_np(alts[b], V, ban, no_repeat, min_id)
        gain, ok = spans_np(x[b], nb, f, out[b], no_repeat, min_id)      # per SLOT: the units' rule, word for word
        cnt = np.zeros((nb + 1, M), np.int64)
        tot = np.zeros((nb + 1, M), np.float64)
        opts = [[None] * M for _ in range(nb)]
        choice = np.full((nb, M), KEEP, np.int64)
        for p in range(nb - 1, -1, -1):
            for m in range(M):
                o = [(c, 1 + cnt[p + len(f[c]), m ^ (1 << j)], gain[p, c] + tot[p + len(f[c]), m ^ (1 << j)])
                     for j in range(K) if (m >> j) & 1 for c in range(j * A, j * A + A) if ok[p, c]]
                o.append((KEEP, cnt[p + 1, m], tot[p + 1, m]))
                best = o[0]
                for c in o[1:]:
                    if c[1] > best[1] or (c[1] == best[1] and c[2] > best[2]):      # strictly greater only: the first best option stays
                        best = c
                opts[p][m] = o
                choice[p, m], cnt[p, m], tot[p, m] = best
        codes = group_codes(f, K, A)
        m = sum(1 << j for j, code in enumerate(codes) if code == -3)
        pos[b] = codes
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
            j = c // A
            pos[b, j], which[b, j] = p, c - j * A
            for i, w in enumerate(f[c]):
                moved[b] += int(out[b, p + i] != w)
                out[b, p + i], ch[b, p + i] = w, x[b, p + i, w]
            m ^= 1 << j
            p += len(f[c])
    return dict(seq=out, chosen=ch, pos=pos, which=which, moved=moved, margin=margin)


def brute_any_np(x, n, f, K, A, seq, no_repeat=False, min_id=7):
    """The placement of one image WITHOUT a recurrence: per kept group "not placed" or (alternative, start) -- every combination -- whose spans are eligible and do not
    overlap, preferred first by the number of groups placed, then by the total gain (the inputs are multiples of 2^-3: every sum is exact in any order), then by the
    decisions read left to right: at a position that no earlier span covers, taking a slot (the lowest slot first) over keeping the id.  Returns {group: (alternative,
    start) or None} over the kept groups."""
    gain, ok = spans_np(x, n, f, seq, no_repeat, min_id)
    groups = [j for j in range(K) if any(isinstance(u, list) for u in f[j * A:(j + 1) * A])]
    per_group = [[None] + [(c, p) for c in range(j * A, j * A + A) if isinstance(f[c], list) for p in range(n)] for j in groups]
    best, best_key = None, None
    for pick in itertools.product(*per_group):
        placed = [cp for cp in pick if cp is not None]
        if any(p + len(f[c]) > n or not ok[p, c] for c, p in placed):
            continue
        covered = [q for c, p in placed for q in range(p, p + len(f[c]))]
        if len(set(covered)) != len(covered):
            continue
        total = sum(gain[p, c] for c, p in placed)
        start = {p: c for c, p in placed}
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
            best, best_key = {j: (None if cp is None else (cp[0] - j * A, cp[1])) for j, cp in zip(groups, pick)}, key
    return best


# ----------------------------------------------------------------------------- tests
def test_require_any_np_on_hand_worked_cases():
    """S = 4, V = 12, n = 4, seq 9 9 9 9, every standing id at -0.5, everything else at -4 unless said.

    Image 0, one group, alternatives (10) and (11).  x[., 10] = -2 everywhere: (10) costs -1.5 wherever it goes.  x[2, 11] = -0.75: (11) costs -0.25 at position 2 and
    -3.5 elsewhere.  The LATER alternative is the cheaper one and wins: position 2 takes alternative 1.  Walk: positions 0 and 1 keep (-0.25 against -1.5 and -3.5: gap
    1.25), position 2 takes slot 1 (-0.25 against slot 0's -1.5 and against keeping, which leaves position 3: -1.5): margin 1.25.  9 9 11 9, pos 2, which 1, moved 1.
    Image 1, one group, alternatives (10) and (11), both at -1 on position 1 and -4 elsewhere: both cost -0.5 there -- an exact tie, and the EARLIER alternative wins:
    9 10 9 9, pos 1, which 0, margin 0.
    Image 2, two groups: ("fire hydrant" = (10 11) or "hydrant" = (11)) and (8).  x[1, 10] = x[2, 11] = -0.75: the bigram costs -0.5 at 1..2; x[., 11] = -0.75 at 2 alone,
    so (11) alone costs -0.25 at 2 -- the shorter alternative is cheaper; 8 costs -0.25 at 1 (x[1, 8] = -0.75), -3.5 elsewhere.  Both groups: (11)@2 + 8@1 = -0.5;
    the bigram at 1..2 would push 8 away: -0.5 - 3.5.  9 8 11 9, pos 2 1, which 1 0, moved 2.
    Image 3, n = 1: group 0 holds (10 11) (does not fit) and (12) (id >= V: skipped): kept, not placeable: -3.  Group 1 holds (13) and an empty slot: -2.  Group 2 is
    empty: -1.  Group 3 repeats (10 11): its only slot is skipped: -2."""
    S, V = 4, 12
    x = np.full((4, S, V), -4.0, np.float32)
    x[:, :, 9] = -0.5
    seq = np.full((4, S), 9, np.int64)
    x[0, :, 10], x[0, 2, 11] = -2.0, -0.75
    x[1, 1, 10] = x[1, 1, 11] = -1.0
    x[2, 1, 10] = x[2, 2, 11] = x[2, 1, 8] = -0.75
    alts = np.full((4, 4, 2, 2), -1, np.int32)
    alts[0, 0, 0, 0], alts[0, 0, 1, 0] = 10, 11
    alts[1, 0, 0, 0], alts[1, 0, 1, 0] = 10, 11
    alts[2, 0, 0], alts[2, 0, 1, 0], alts[2, 1, 0, 0] = [10, 11], 11, 8
    alts[3, 0, 0], alts[3, 0, 1, 0], alts[3, 1, 0, 0], alts[3, 3, 0] = [10, 11], 12, 13, [10, 11]
    r = require_any_np(x, [4, 4, 4, 1], alts, seq, chosen=np.full((4, S), 7.0, np.float32))
    assert r["seq"].tolist() == [[9, 9, 11, 9], [9, 10, 9, 9], [9, 8, 11, 9], [9, 9, 9, 9]]
    assert r["pos"].tolist() == [[2, -1, -1, -1], [1, -1, -1, -1], [2, 1, -1, -1], [-3, -2, -1, -2]]
    assert r["which"].tolist() == [[1, -1, -1, -1], [0, -1, -1, -1], [1, 0, -1, -1], [-1, -1, -1, -1]]
    assert r["moved"].tolist() == [1, 1, 2, 0]
    assert r["margin"].tolist()[:2] == [1.25, 0.0] and r["margin"][3] == INF
    assert r["chosen"].tolist() == [[7.0, 7.0, -0.75, 7.0], [7.0, -1.0, 7.0, 7.0], [7.0, -0.75, -0.75, 7.0], [7.0] * 4]
    # alternatives of one group may share a word under no_repeat ((10 11) and (11) above); alternatives of DIFFERENT groups that could meet are skipped
    t = [[[8, 9], [9, 8]], [[9, 5], [3, 3]], [[8, 8], [5, 6]]]
    assert classify_any_np(t, 12, no_repeat=True) == [[8, 9], [9, 8], -2, [3, 3], -2, [5, 6]]
    assert classify_any_np(t, 12) == [[8, 9], [9, 8], [9, 5], [3, 3], [8, 8], [5, 6]]
    assert classify_any_np([[[3, 4], [3, 4]], [[-5, 2], [3, 4]], [[12, 1], [4, 11]]], 12, ban=[11]) == [[3, 4], -2, -1, -2, -2, -2]
    assert group_codes([[3], -2, -1, -2, -1, -1], 3, 2) == [-3, -2, -1]


def _random_alts(rng, K, A, L, V=16):
    alts = np.stack([_random_units(rng, A, L, V) for _ in range(K)])
    alts[rng.random((K, A)) < 0.2] = -1                         # empty alternatives in the middle of a group
    return alts.astype(np.int32)


def test_require_any_np_equals_the_brute_force():
    """Every assignment enumerated, S <= 6, K <= 3, A <= 3, L <= 3, V = 16; inputs multiples of 2^-3 with NaN and +-inf, ties, alternatives that stand in seq already
    and alternatives that share ids, with and without the adjacency rule and a ban."""
    rng = np.random.default_rng(20262)
    tied = later = long_placed = standing = skipped_meet = 0
    for it in range(800):
        S, K, A, L = int(rng.integers(2, 7)), int(rng.integers(1, 4)), int(rng.integers(1, 4)), int(rng.integers(1, 4))
        x, n, _, seq = _random_case(rng, S, K)
        alts = _random_alts(rng, K, A, L)
        first = [int(v) for v in alts[0, A - 1] if v >= 0] if (alts[0, A - 1] >= 0).all() else []
        if it % 3 == 0 and first and len(first) <= n and max(first) < 16:      # the LAST alternative of group 0 already stands in seq
            seq[:len(first)] = first
        rep, ban = bool(it & 1), ([int(alts[0, 0, 0])] if it % 7 == 0 and 0 <= alts[0, 0, 0] < 16 else [])
        r = require_any_np(x[None], [n], alts[None], seq[None], ban=ban, no_repeat=rep)
        f = classify_any_np(alts, 16, ban, rep)
        want = brute_any_np(x, n, f, K, A, seq, rep)
        codes = group_codes(f, K, A)
        got = {j: ((int(r["which"][0, j]), int(r["pos"][0, j])) if r["pos"][0, j] >= 0 else None) for j in range(K) if codes[j] == -3}
        assert got == want, (it, S, K, A, L, n, alts, seq, rep, ban)
        assert all(r["pos"][0, j] == codes[j] and r["which"][0, j] == -1 for j in range(K) if codes[j] != -3)
        assert ((r["pos"][0] >= 0) == (r["which"][0] >= 0)).all()
        after = seq.copy()
        for j, ap in want.items():
            if ap is not None:
                u = f[j * A + ap[0]]
                standing += int(list(seq[ap[1]:ap[1] + len(u)]) == u)
                long_placed += int(len(u) > 1)
                later += int(ap[0] > 0)
                after[ap[1]:ap[1] + len(u)] = u
        assert np.array_equal(r["seq"][0], after) and r["moved"][0] == int((after != seq).sum())
        tied += int(r["margin"][0] == 0.0)
        if rep:
            free = classify_any_np(alts, 16, ban, False)
            skipped_meet += sum(1 for a, b in zip(free, f) if isinstance(a, list) and b == -2)
            for p in range(1, n):                                # a placement never creates an adjacent repeat of a word
                assert not (after[p] == after[p - 1] and after[p] >= 7 and (after[p] != seq[p] or after[p - 1] != seq[p - 1])), (it, seq, after, f)
    print(f"tied {tied}, groups placed by a later alternative {later}, alternatives of two or more ids placed {long_placed}, placed where they stood {standing}, "
          f"slots skipped under no_repeat {skipped_meet}")
    assert tied >= 40 and later >= 40 and long_placed >= 40 and standing >= 40 and skipped_meet >= 20      # the cases are not vacuous


def test_one_alternative_per_group_is_require_units_np():
    """A = 1 -- and A = 3 with empty slots behind the first -- give ``require_units_np``'s seq, pos, moved, chosen and margin, field for field, and which = 0 where
    placed; with and without the adjacency rule and a ban."""
    rng = np.random.default_rng(20263)
    for it in range(300):
        S, K, L = int(rng.integers(1, 8)), int(rng.integers(1, 4)), int(rng.integers(1, 4))
        x, n, _, seq = _random_case(rng, S, K)
        units = _random_units(rng, K, L)
        rep, ban = bool(it & 1), ([int(units[0, 0])] if it % 7 == 0 and 0 <= units[0, 0] < 16 else [])
        keep = np.full((1, S), 3.0, np.float32)
        want = require_units_np(x[None], [n], units[None], seq[None], ban=ban, no_repeat=rep, chosen=keep)
        for A in (1, 3):
            alts = np.full((1, K, A, L), -1, np.int32)
            alts[0, :, 0] = units
            if A == 3:
                alts[0, :, 2, 1:] = 9                            # (behind the first negative id: not read)
            got = require_any_np(x[None], [n], alts, seq[None], ban=ban, no_repeat=rep, chosen=keep)
            for k in ("seq", "pos", "moved", "margin"):
                assert np.array_equal(got[k], want[k]), (it, A, k)
            assert np.array_equal(got["chosen"].view(np.int32), want["chosen"].view(np.int32)), (it, A)
            assert np.array_equal(got["which"], np.where(want["pos"] >= 0, 0, -1)), (it, A)


def test_require_any_table_is_checked_on_the_host():
    from boficap_amd import hip
    t = hip.require_any_table([[[[3, 4], [5]], [[6]]], [], [[[6, 7, 8], [], [2]], []]], 3, 10)
    assert t.dtype == torch.int32 and t.shape == (3, 2, 3, 3)
    assert t[0].tolist() == [[[3, 4, -1], [5, -1, -1], [-1] * 3], [[6, -1, -1], [-1] * 3, [-1] * 3]] and (t[1] == -1).all()
    assert t[2].tolist() == [[[6, 7, 8], [-1] * 3, [2, -1, -1]], [[-1] * 3] * 3]      # (an empty alternative keeps its place: ``which`` indexes the group as given; an empty group is dropped)
    assert hip.require_any_table([[[7, 8], [9]], [[5]]], 2, 10).tolist() == [[[[7, 8], [9, -1]], [[5, -1], [-1, -1]]]] * 2      # one flat list of groups: every image
    arr = np.array([[[[1, 2], [-1, -1]], [[3, -1], [4, 5]]], [[[6, -1], [7, -1]], [[-1, -1], [-1, -1]]]])
    assert hip.require_any_table(arr, 2, 10).tolist() == arr.tolist()
    assert hip.require_any_table(torch.tensor(arr[0]), 2, 10).tolist() == [arr[0].tolist()] * 2      # [K, A, L]: every image
    for off in (None, [], [[], []], [[[]], None], [[[[]]], []], np.full((2, 1, 2, 2), -1), np.full((1, 2, 2), -1)):
        assert hip.require_any_table(off, 2, 10) is None
    for bad, word in (([[[[10]]]], "0..9"), ([[[[-2, 1]]]], "0..9"), ([[[[1, 2, 3, 4, 5]]]], r"at most 4 ids, got \[1, 2, 3, 4, 5\]"),
                      ([[[[i]] for i in range(9)]], "at most 8 required groups"), ([[[[i] for i in range(5)]]], "at most 4 alternatives"),
                      ([[[[1, 3]]]], r"id 3 of alternative \[1, 3\] is also in ban_ids"), ([[[[1]]], [[[2]]]], "rows"),
                      ([[[[1, 2], [1, 2]]]], r"alternative \[1, 2\] is given twice in one group"), ([[[[1, 2]], [[4], [1, 2]]]], r"alternative \[1, 2\] is given twice \(in two groups\)"),
                      ([3, 4], r"bare id 3.*\[\[\[3\], \[4, 5\]\]\]"), ([[3, 4]], r"bare id 3.*\[\[\[3\], \[4, 5\]\]\]"), ([[[3], 4]], "bare id 4"), ([[[[3], 4]]], "bare id 4"),
                      (np.zeros((2, 2), np.int64), r"\[B, K, A, L\]")):
        with pytest.raises(hip.BofiHipError, match=word) as e:
            hip.require_any_table(bad, 1, 10, ban_ids=[3] if "ban_ids" in word else ())
        assert "require_any" in str(e.value)
    # under no_repeat: an alternative that repeats a word, and two alternatives of DIFFERENT groups that could meet -- both named; alternatives of one group may share
    # a word; neither is refused without the rule, or below repeat_min_id
    with pytest.raises(hip.BofiHipError, match=r"alternative \[8, 8, 9\] repeats a word"):
        hip.require_any_table([[[[8, 8, 9]]]], 1, 10, no_repeat=True)
    with pytest.raises(hip.BofiHipError, match=r"alternatives \[7, 8\] and \[8, 9\] of different groups could meet"):
        hip.require_any_table([[[[7, 8]], [[5], [8, 9]]]], 1, 10, no_repeat=True)
    with pytest.raises(hip.BofiHipError, match=r"alternatives \[8, 9\] and \[7, 8\] of different groups could meet"):
        hip.require_any_table([[[[8, 9]], [[7, 8]]]], 1, 10, no_repeat=True)
    assert hip.require_any_table([[[[7, 8], [8, 9]]]], 1, 10, no_repeat=True).shape == (1, 1, 2, 2)
    assert hip.require_any_table([[[[8, 8, 9]], [[7, 8]], [[9, 7]]]], 1, 10).shape == (1, 3, 1, 3)
    assert hip.require_any_table([[[[3, 3]], [[2, 3]]]], 1, 10, no_repeat=True).shape == (1, 2, 1, 2)
    assert hip.require_any_table([[[[8, 8]]]], 1, 10, no_repeat=True, repeat_min_id=9).shape == (1, 1, 1, 2)
    assert hip.REQUIRE_ALT_MAX == 4 and hip.REQUIRE_UNIT_MAX == 4 and hip.REQUIRE_MAX == 8


def test_the_host_table_is_what_the_rule_keeps():
    """What ``require_any_table`` accepts, the rule classifies as kept (or empty): the host refuses by name exactly what the kernel would skip."""
    from boficap_amd import hip
    rng = np.random.default_rng(20264)
    accepted = 0
    for it in range(300):
        K, A, L = int(rng.integers(1, 4)), int(rng.integers(1, 4)), int(rng.integers(1, 4))
        alts = _random_alts(rng, K, A, L)
        alts[alts >= 16] = 12
        rep, ban = bool(it & 1), ([9] if it % 5 == 0 else [])
        lists = [[[[int(v) for v in u[:next((i for i, v in enumerate(u) if v < 0), len(u))]] for u in g] for g in alts]]
        try:
            t = hip.require_any_table(lists, 1, 16, ban, rep, 7)
        except hip.BofiHipError:
            assert -2 in classify_any_np(alts, 16, ban, rep), (alts, rep, ban)
            continue
        accepted += 1
        if t is not None:
            assert -2 not in classify_any_np(t[0].numpy(), 16, ban, rep)
    assert 30 <= accepted <= 270


def test_declarations_agree():
    """The entry point in header, ctypes table, build list and library; BOFI_REQUIRE_ALT_MAX; the per-call record and the ABI version as they were."""
    from boficap_amd import build, hip
    header = open(os.path.join(ROOT, "include", "boficap_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    found = re.findall(r"\bbofi_vocab_require_any\s*\(([^;{]*?)\)\s*;", code, flags=re.S)
    assert len(found) == 1 and found[0].count(",") + 1 == len(hip.SIGNATURES["bofi_vocab_require_any"][1]) == 20
    assert int(re.search(r"#define\s+BOFI_REQUIRE_ALT_MAX\s+(\d+)", code).group(1)) == hip.REQUIRE_ALT_MAX == 4
    assert int(re.search(r"#define\s+BOFI_REQUIRE_UNIT_MAX\s+(\d+)", code).group(1)) == hip.REQUIRE_UNIT_MAX == 4
    assert int(re.search(r"#define\s+BOFI_REQUIRE_MAX\s+(\d+)", code).group(1)) == hip.REQUIRE_MAX == 8
    assert "record stays 128 bytes" in header and C.sizeof(hip.BofiCallOpts) == 128 and hip.ABI_VERSION == 5
    assert [n for n, _ in hip.BofiCallOpts._fields_][-3:] == ["pick_ban", "pick_no_repeat", "pick_repeat_min_id"]      # no field for this option
    assert "force.hip" in build.SOURCES
    kernels = open(os.path.join(build.CSRC, "bofi_kernels.h")).read()
    assert "launch_vocab_require_any" in kernels and "vocab_require_any_check" in kernels
    assert "vocab_require_any_kernel" in open(os.path.join(build.CSRC, "force.hip")).read()
    _, lib = _lib()
    assert hasattr(lib, "bofi_vocab_require_any") and callable(hip.vocab_require_any) and callable(hip.require_any_table) and lib.bofi_abi_version() == 5


def test_entry_point_refuses_bad_arguments_without_a_device():
    """Each returns BOFI_ERR_ARG (1) from the argument check, with a message: the pointers are never read, nothing is launched.  rows = 0 is BOFI_OK."""
    hip, lib = _lib()
    p = C.c_void_p(0x1000)
    good = dict(x=p, ldx=9491, rows=40, V=9491, S=20, ntok=None, ntok_bias=0, alts=p, K=4, A=3, L=2, ban=None, no_repeat=1, min_id=7, seq=p, chosen=None, pos=p, which=p,
                moved=None)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.bofi_vocab_require_any(a["x"], a["ldx"], a["rows"], a["V"], a["S"], a["ntok"], a["ntok_bias"], a["alts"], a["K"], a["A"], a["L"], a["ban"], a["no_repeat"],
                                        a["min_id"], a["seq"], a["chosen"], a["pos"], a["which"], a["moved"], None)
        if rc == 1:
            assert b"vocab_require_any" in lib.bofi_last_error(), kw
        return rc

    assert call(x=None) == 1 and call(seq=None) == 1 and call(alts=None) == 1 and call(pos=None) == 1
    assert call(which=None) == 1 and b"which" in lib.bofi_last_error()
    assert call(rows=41) == 1 and call(rows=-20) == 1
    assert call(V=1) == 1 and call(V=0) == 1
    assert call(ldx=9490) == 1
    assert call(S=0, rows=0) == 1 and call(S=65, rows=65) == 1
    assert call(K=0) == 1 and call(K=9) == 1 and b"K in 1..8" in lib.bofi_last_error()
    assert call(A=0) == 1 and call(A=5) == 1 and b"A in 1..4" in lib.bofi_last_error() and call(A=-1) == 1
    assert call(L=0) == 1 and call(L=5) == 1 and b"L in 1..4" in lib.bofi_last_error() and call(L=-1) == 1
    assert call(no_repeat=2) == 1 and call(no_repeat=-1) == 1
    assert call(min_id=-1) == 1
    assert call(rows=0) == 0 and call(rows=0, S=64, K=8, A=4, L=4) == 0 and call(rows=0, A=1, L=1) == 0


def test_engine_keywords_are_validated_on_the_host():
    from boficap_amd import hip
    from boficap_amd.engine import BofiEngine, DecodePipeline
    table = BofiEngine._require_any_table
    assert table(_Eng, None, 2) is None and table(_Eng, [], 2) is None and table(_Eng, [[], []], 2) is None
    assert table(_Eng, [[[3, 4], [5]], [[6]]], 2).tolist() == [[[[3, 4], [5, -1]], [[6, -1], [-1, -1]]]] * 2
    for bad, ban, rep, word in (([[[10]]], None, False, "0..9"), ([[[1, 2, 3, 4, 5]]], None, False, "at most 4 ids"), ([[[3, 4]]], [3], False, "ban_ids"),
                                ([[[[1]]]], None, False, "rows"), ([[[7, 8]], [[8, 9]]], None, True, "could meet"), ([[[8, 8]]], None, True, "repeats a word"),
                                ([[[5], [5]]], None, False, "given twice"), ([[5, 6]], None, False, "bare id 5")):
        with pytest.raises(hip.BofiHipError, match=word):
            table(_Eng, bad, 2, ban, rep)
    for args, word in (((True, 0, False), "ids_only"), ((False, hip.FLAG_MASK_PREDICT, False), "mask_predict"), ((False, 0, True), "block_trigrams")):
        with pytest.raises(hip.BofiHipError, match=word) as e:
            BofiEngine._require_refusals(*args, "require_any")
        assert "require_any" in str(e.value)

    class _E(_Eng):
        _pick_ban = staticmethod(lambda ban_ids, block_trigrams=False: None)
        _require_table, _require_unit_table, _require_any_table = BofiEngine._require_table, BofiEngine._require_unit_table, BofiEngine._require_any_table
        _require_refusals = staticmethod(BofiEngine._require_refusals)
    for ids, phrases in (([3], None), (None, [[4, 5]])):        # two of the three options: refused before anything else is resolved
        with pytest.raises(hip.BofiHipError, match="give one"):
            BofiEngine._post_options(_E(), None, False, 7, False, ids, None, False, 2, False, 0, True, phrases, [[[6], [7]]])

    class _Pipe:
        fused_vocab, refine_method, block_trigrams, root_vocab, ban_ids, no_repeat, repeat_min_id = False, "feed_back", False, 10, (3,), True, 7
    split = DecodePipeline._any_split
    assert split(_Pipe, None) == (None, None) and split(_Pipe, []) == (None, None)
    assert split(_Pipe, [[[4, 5], [6]], [[7]]]) == ([[[4, 5], [6]], [[7], []]], None)      # one flat list of groups
    flat, per_batch = split(_Pipe, [[[[[1, 2]]]], None])
    assert flat is None and list(per_batch) == [[[[[1, 2]]]], None]
    for bad, word in (([[[3, 4]]], "ban_ids"), ([[[10]]], "0..9"), (np.zeros((2, 2, 2, 2), np.int64), "per-batch"), ([4, 5], "bare id 4"),
                      ([[[7, 8]], [[8, 9]]], "could meet")):
        with pytest.raises(hip.BofiHipError, match=word):
            split(_Pipe, bad)
    for attr, value, word in (("fused_vocab", True, "fused_vocab"), ("refine_method", "mask_predict", "mask_predict"), ("block_trigrams", True, "block_trigrams")):
        P = type("P", (_Pipe,), {attr: value})
        with pytest.raises(hip.BofiHipError, match=word) as e:
            split(P, [[[4]]])
        assert "require_any" in str(e.value)
        assert split(P, None) == (None, None)                   # off: nothing to refuse
    for ids, phrases in (([4], None), (None, [[5, 6]]), ([4], [[5, 6]])):
        with pytest.raises(hip.BofiHipError, match="give one"):
            DecodePipeline._require_both(ids, phrases, [[[7]]])
    DecodePipeline._require_both(None, None, [[[7]]]), DecodePipeline._require_both([4], None, []), DecodePipeline._require_both(None, [[5]], None)


def test_eval_options_resolve_alternatives():
    from boficap_amd import eval_utils as E
    vocab = {"7": "a", "8": "fire", "9": "dog", "10": "hydrant", "11": "dog", "12": "hot dog", "13": "hot", "14": "dogs", "15": "puppy", "16": "tv|dvd", "17": "tv"}
    keys = [0, 1, 2]
    # no '|' anywhere: the output as it was, shape included
    assert E.required_of({"require_words": "dog,a"}, vocab, keys) == ([[9, 7]] * 3, [["dog", "a"]] * 3)
    ids, words = E.required_of({"require_words": "fire hydrant,dog"}, vocab, keys)
    assert ids == [[[8, 10], [9]]] * 3 and E.required_key(ids) == "require_phrases" and not E.required_any(ids)
    assert E.required_key([[9, 7]]) == "require_ids"
    # an item that is itself a vocabulary entry is a plain word, '|' or not
    assert E.required_of({"require_words": "tv|dvd,a"}, vocab, keys) == ([[16, 7]] * 3, [["tv|dvd", "a"]] * 3)
    # a '|' item: the whole evaluation goes through groups, plain items as groups of one alternative
    ids, words, texts = E.required_of({"require_words": "dog|dogs|puppy,fire hydrant|hydrant,a,dog|dogs|puppy"}, vocab, keys)
    assert ids == [[[[9], [14], [15]], [[8, 10], [10]], [[7]]]] * 3 and E.required_any(ids) and E.required_key(ids) == "require_any"
    assert words == [["dog|dogs|puppy", "fire hydrant|hydrant", "a"]] * 3 and texts == [[["dog", "dogs", "puppy"], ["fire hydrant", "hydrant"], ["a"]]] * 3
    ids, words, texts = E.required_of({"require_words": {"1": ["a"], 2: "dog a| dogs ,tv|dvd"}}, vocab, keys)
    assert ids == [[], [[[7]]], [[[9, 7], [14]], [[16]]]] and words == [[], ["a"], ["dog a| dogs ", "tv|dvd"]] and texts == [[], [["a"]], [["dog a", "dogs"], ["tv|dvd"]]]
    # a vocabulary entry that equals the whole alternative wins over splitting
    ids, _, texts = E.required_of({"require_words": ["hot dog|hot a"]}, vocab, keys)
    assert ids == [[[[12], [13, 7]]]] * 3 and texts == [[["hot dog", "hot a"]]] * 3
    with pytest.raises(ValueError, match="'cat'") as e:          # the unknown word inside an alternative is named
        E.required_of({"require_words": ["dog|fire cat"]}, vocab, keys)
    assert "fire cat" not in str(e.value)
    with pytest.raises(ValueError, match="1 to 4 words"):
        E.required_of({"require_words": ["dog|a a a a a"]}, vocab, keys)
    with pytest.raises(ValueError, match="at most 4 alternatives"):
        E.required_of({"require_words": ["dog|dogs|puppy|a|hot"]}, vocab, keys)
    with pytest.raises(ValueError, match="'hydrant' is also banned"):
        E.required_of({"require_words": ["fire|hydrant"]}, vocab, keys, ban_ids=[10])
    with pytest.raises(ValueError, match="'dog' is given twice in 'dog\\|dog'"):
        E.required_of({"require_words": ["dog|dog"]}, vocab, keys)
    with pytest.raises(ValueError, match="'dogs' is given twice \\(in 'dog\\|dogs' and 'puppy\\|dogs'\\)"):
        E.required_of({"require_words": ["dog|dogs", "puppy|dogs"]}, vocab, keys)
    with pytest.raises(ValueError, match="at most 8"):
        E.required_of({"require_words": ["a|dog"] + [f"{i}" for i in range(8)]}, dict(vocab, **{str(20 + i): str(i) for i in range(8)}), keys)
    for kw, mode, n, word in (({}, "SAIC", 1, "NAIC"), ({"fused_vocab": True}, "NAIC", 1, "fused_vocab"), ({"refine_method": "mask_predict"}, "NAIC", 1, "mask_predict"),
                              ({}, "NAIC", 5, "sample_n"), ({"block_trigrams": 1}, "NAIC", 1, "block_trigrams")):
        with pytest.raises(ValueError, match=word) as e:
            E.required_of(dict(kw, require_words=["dog|dogs"]), vocab, keys, mode, n)
        assert "require_words" in str(e.value)
    # under decoding_constraint: what the table would refuse, in the items' own words; alternatives of ONE item may share a word
    with pytest.raises(ValueError, match="'fire hydrant' and 'hydrant a' could meet"):
        E.required_of({"require_words": "fire hydrant|fire,dog|hydrant a", "decoding_constraint": 1}, vocab, keys)
    with pytest.raises(ValueError, match="'fire fire' repeats a word"):
        E.required_of({"require_words": "dog|fire fire", "decoding_constraint": 1}, vocab, keys)
    assert E.required_of({"require_words": "fire hydrant|hydrant a", "decoding_constraint": 1}, vocab, keys)[0] == [[[[8, 10], [10, 7]]]] * 3
    assert E.required_of({"require_words": "fire hydrant|fire,dog|hydrant a"}, vocab, keys)[0] == [[[[8, 10], [8]], [[9], [10, 7]]]] * 3
    # 'required' holds [item, start or None, the alternative placed or None]; required_rate counts groups
    pos = torch.tensor([[3, -3, -1], [-3, 0, 5]], dtype=torch.int32)
    alt = torch.tensor([[1, -1, -1], [-1, 0, 2]], dtype=torch.int32)
    assert E.required_entry(["fire hydrant|hydrant", "dog"], pos[0], alt[0], [["fire hydrant", "hydrant"], ["dog"]]) == [["fire hydrant|hydrant", 3, "hydrant"], ["dog", None, None]]
    assert E.required_entry(["a", "dog|dogs", "x|y|dogs"], pos[1], alt[1], [["a"], ["dog", "dogs"], ["x", "y", "dogs"]]) == [["a", None, None], ["dog|dogs", 0, "dog"], ["x|y|dogs", 5, "dogs"]]
    assert E.required_entry(["fire hydrant", "dog"], pos[0]) == [["fire hydrant", 3], ["dog", None]]      # (without alternatives: the entry as it was)
    assert E.required_rates([["fire hydrant|hydrant", "dog"], ["a", "dog|dogs", "x|y|dogs"]], list(pos), 3, 12) == {"required_rate": 3 / 5, "required_moved_rate": 0.25}


@pytest.mark.parametrize("args,word", [(["--require_words", "dog|dogs", "--inference_mode", "SAIC"], "NAIC"), (["--require_words", "fire hydrant|hydrant,dog", "--fused_vocab"], "fused_vocab"),
                                       (["--require_words", "a|b", "--refine_rounds", "2", "--refine_method", "mask_predict"], "mask_predict"),
                                       (["--require_words", "a|b", "--sample_n", "3"], "sample_n"), (["--require_words", "a|b", "--block_trigrams", "1"], "block_trigrams")])
def test_eval_tool_refuses_required_alternatives_where_they_cannot_apply(args, word):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval.py"), *args, "--synthetic", "8"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 2 and "--require_words" in r.stderr and word in r.stderr, r.stderr[-400:]


def test_eval_tool_help_says_alternatives_are_accepted():
    text = open(os.path.join(ROOT, "tools", "eval.py")).read()
    assert "dog|dogs" in text and "alternatives" in re.search(r'"--require_words",.*?\)\n', text, flags=re.S).group(0)
    assert "required_key" in text and "required_alt" in text
