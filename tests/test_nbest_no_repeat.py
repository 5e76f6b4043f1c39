"""The N most probable captions with no adjacent repeated word, host side (no GPU): the rule of ``bofi_vocab_nbest_norepeat`` (include/boficap_hip.h states it in
words) RESTATED in numpy (``nbest_nr_np``: the N + 2 candidates in ``order_np``'s order, the per-candidate float64 lists, the tie order), held against a BRUTE FORCE over
every valid caption -- what tests/test_gpu_nbest_no_repeat.py holds the kernel and the engines to --, the evidence that N + 1 candidates are not enough, the relation to
the plain list (``nbest_np``) and to the scan of ``bofi_vocab_constrain`` (``pick_np``), the declarations, and the refusals that need no device."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_constrained_pick import order_np, pick_np
from test_nbest import nbest_np, same_bits

NAN, INF = float("nan"), float("inf")


# ----------------------------------------------------------------------------- the rule, restated
def nbest_nr_np(x, n, N, ban=(), pad=0, repeat_min_id=7, K=None):
    """The no-repeat N-best lists of x [B, S, >= V] (all of x.shape[2] columns are the vocabulary) with n [B] live positions (clamped to 0 .. S): a dict of ``seq``
    int64 [B, N, S], ``total`` float64 [B, N], ``count`` int32 [B], and for the tests' own statistics ``tie`` bool [B] (two pairs of some list, or two entries of the
    result, had the same total) and ``degenerate`` bool [B].  ``K``: candidates per row, the rule's N + 2 by default (the tests show that N + 1 are too few)."""
    x = np.asarray(x)
    B, S, _ = x.shape
    K = N + 2 if K is None else K
    ban = sorted({int(i) for i in ban})
    seq = np.full((B, N, S), pad, np.int64)
    total = np.full((B, N), -INF, np.float64)
    count = np.zeros(B, np.int32)
    tie, degenerate = np.zeros(B, bool), np.zeros(B, bool)
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
            count[b], total[b, 0] = 1, NAN
            seq[b, 0, :nb] = [pad if first is None else first for first, _ in rows]
            continue
        if nb == 0:
            count[b], total[b, 0] = 1, 0.0
            continue
        A = {r: [(0.0 + v, [i])] for r, (i, v) in rows[0][1].items()}
        for p in range(1, nb):
            prev, new = rows[p - 1][1], {}
            for r, (i, v) in rows[p][1].items():
                pairs = [(T + v, rq, j, ids + [i]) for rq in sorted(A) for j, (T, ids) in enumerate(A[rq])
                         if not (prev[rq][0] == i and prev[rq][0] >= repeat_min_id)]      # (python floats: one float64 add per pair)
                pairs.sort(key=lambda t: (-t[0], t[1], t[2]))
                tie[b] |= len({t[0] for t in pairs}) < len(pairs)
                new[r] = [(t[0], t[3]) for t in pairs[:N]]
            A = new
        fin = [(T, r, j, ids) for r in sorted(A) for j, (T, ids) in enumerate(A[r])]
        fin.sort(key=lambda t: (-t[0], t[1], t[2]))
        tie[b] |= len({t[0] for t in fin}) < len(fin)
        count[b] = min(N, len(fin))
        for j, (T, _, _, ids) in enumerate(fin[:N]):
            total[b, j] = T
            seq[b, j, :nb] = ids
    return dict(seq=seq, total=total, count=count, tie=tie, degenerate=degenerate)


def is_valid(cap, ban=(), repeat_min_id=7):
    return all(i not in ban for i in cap) and not any(cap[p] == cap[p - 1] and cap[p - 1] >= repeat_min_id for p in range(1, len(cap)))


def brute_nr_np(x, n, ban=(), repeat_min_id=7):
    """Every VALID caption of one image x [S, V] with a finite total, the float64 sum taken left to right (itertools.product's order, built as arrays):
    (totals float64 [M] best first, captions int [M, n])."""
    V = x.shape[1]
    ids = np.array([i for i in range(V) if i not in set(ban)], np.int64)
    caps = np.zeros((1, 0), np.int64)
    T = np.zeros(1, np.float64)
    for p in range(n):
        v = x[p, ids].astype(np.float64)
        T = (T[:, None] + v[None, :]).reshape(-1)               # one float64 add per caption and position, left to right
        caps = np.concatenate([np.repeat(caps, len(ids), 0), np.tile(ids, len(caps))[:, None]], 1)
    ok = np.isfinite(T)
    for p in range(1, n):
        ok &= ~((caps[:, p] == caps[:, p - 1]) & (caps[:, p - 1] >= repeat_min_id))
    T, caps = T[ok], caps[ok]
    o = np.argsort(-T, kind="stable")
    return T[o], caps[o]


def _brute_cases(count=1500):
    """The cases of the brute-force tests: V in 2..7, S = 5, n in 0..5, N in 1..6, repeat_min_id in 0..2.  Values: case % 3 == 0 a grid of eighths in [-8, 0], == 1 a
    four-value grid (ties everywhere), == 2 a grid of eighths in [-2, 0]; every fifth case float32 logs of Dirichlet rows instead (off any grid: every add rounds).
    Every second case with a random ban list that leaves at least one id."""
    rng = np.random.default_rng(21)
    for case in range(count):
        V, S, N = int(rng.integers(2, 8)), 5, int(rng.integers(1, 7))
        n, lo = int(rng.integers(0, 6)), int(rng.integers(0, 3))
        hi = (65, 4, 17)[case % 3]
        x = (-rng.integers(0, hi, (1, S, V)) / 8.0).astype(np.float32)
        if case % 5 == 0:
            x = np.log(rng.dirichlet(np.full(V, 0.5), (1, S)) + 1e-30).astype(np.float32)
        ban = tuple(int(i) for i in rng.choice(V, int(rng.integers(0, V)), replace=False)) if case % 2 else ()
        yield case, x, n, N, ban, lo


def _agrees_with_brute(r, T, caps, n, N):
    """Does the list ``r`` of one image meet what the brute force (T, caps) demands?  The totals are its first count, count = min(N, valid captions), the rows are
    distinct, and the captions strictly above the last total are the same set."""
    c = int(r["count"][0])
    if c != min(N, len(T)) or r["total"][0, :c].tolist() != T[:c].tolist():
        return False
    got = [tuple(int(v) for v in r["seq"][0, j, :n]) for j in range(c)]
    if len(set(got)) != c:
        return False
    if c == 0:
        return True
    last = r["total"][0, c - 1]
    return {tuple(int(v) for v in cap) for t, cap in zip(T, caps) if t > last} == {cap for cap, t in zip(got, r["total"][0, :c]) if t > last}


# ----------------------------------------------------------------------------- tests
def test_list_equals_the_brute_force_over_every_valid_caption():
    """1 500 cases (``_brute_cases``): the totals are the brute force's first ``count`` totals, the captions strictly above the last total are the same set, the rows
    are distinct and valid, each total is the left-to-right float64 sum of its own values, the totals do not increase, count = min(N, number of valid captions).  At
    least 100 cases each with ties, without, with count < N, with a ban list that bites and with an adjacent repeat in the UNconstrained best caption."""
    ties = short = bites = plain = 0
    for case, x, n, N, ban, lo in _brute_cases():
        r = nbest_nr_np(x, [n], N, ban, pad=0, repeat_min_id=lo)
        T, caps = brute_nr_np(x[0], n, ban, lo)
        c = int(r["count"][0])
        assert _agrees_with_brute(r, T, caps, n, N), (case, r["total"], T[:N])
        assert (r["total"][0, c:] == -INF).all() and (r["seq"][0, c:] == 0).all() and (r["seq"][0, :, n:] == 0).all() and not r["degenerate"][0]
        for j in range(c):
            cap = [int(v) for v in r["seq"][0, j, :n]]
            assert is_valid(cap, ban, lo), (case, cap)
            s = 0.0
            for p, i in enumerate(cap):
                s = s + float(x[0, p, i])
            assert s == r["total"][0, j]
        assert (np.diff(r["total"][0, :c]) <= 0).all()
        ties += bool(r["tie"][0])
        short += c < N
        first = [int(order_np(x[0, p], ban)[0]) for p in range(n)]
        plain += not is_valid(first, (), lo)
        bites += bool(ban) and n > 0 and any(int(order_np(x[0, p])[0]) in ban for p in range(n))
    print(f"no-repeat n-best against the brute force: 1500 cases, {ties} with ties, {short} with count < N, {plain} whose unconstrained best caption repeats a word, "
          f"{bites} in which the ban list removes a row's best id")
    assert ties >= 100 and 1500 - ties >= 100 and short >= 100 and plain >= 100 and bites >= 100


def test_n_plus_1_candidates_are_not_enough():
    """The same cases with K = N + 1 candidates per row disagree with the brute force somewhere; and the sandwich shows it by construction."""
    wrong = [case for case, x, n, N, ban, lo in _brute_cases()
             if not _agrees_with_brute(nbest_nr_np(x, [n], N, ban, 0, lo, K=N + 1), *brute_nr_np(x[0], n, ban, lo), n, N)]
    print(f"K = N + 1 candidates: wrong in {len(wrong)} of 1500 cases {wrong[:8]}")
    assert wrong
    x, want = sandwich()
    short = nbest_nr_np(x, [3], 6, K=7)
    assert short["count"][0] == 5 and short["seq"][0, :5].tolist() == want[:5]      # (9, 5, 10), rank 7 of row 1, is out of reach


def sandwich(V=12):
    """S = 3, repeat_min_id = 7: row 0 is finite only at id 9, row 2 only at id 10; row 1 is led by 9, then 10, then ids 0, 1, 2, ...  Both leaders of row 1 are
    excluded by the neighbours, so the 6 best valid captions are (9, k, 10), k = 0..5: ranks 2..7 of row 1.  Returns (x [1, 3, V], the list)."""
    x = np.full((1, 3, V), -INF, np.float32)
    x[0, 0, 9], x[0, 2, 10] = -0.5, -0.25
    x[0, 1] = -2.0 - np.arange(V) / 4.0
    x[0, 1, 9], x[0, 1, 10] = -0.125, -0.375
    return x, [[9, k, 10] for k in range(6)]


def test_sandwich_needs_n_plus_2_candidates():
    x, want = sandwich()
    r = nbest_nr_np(x, [3], 6)
    assert r["count"][0] == 6 and r["seq"][0].tolist() == want and not r["tie"][0]
    assert r["total"][0].tolist() == [(-0.5 + (-2.0 - k / 4.0)) + -0.25 for k in range(6)]
    T, caps = brute_nr_np(x[0], 3)
    assert caps[:6].tolist() == want and T[:6].tolist() == r["total"][0].tolist()
    # the plain list's entries all repeat a word or are the two captions (9, 9, 10) and (9, 10, 10)
    p = nbest_np(x, [3], 6)
    assert p["seq"][0, 0].tolist() == [9, 9, 10] and p["seq"][0, 1].tolist() == [9, 10, 10]


def test_hand_worked_cases():
    """ids 7.. are words.  (a) two positions with a tie; (b) count = 0; (c) a degenerate image; (d) ids below repeat_min_id may repeat; (e) n = 0 and n = 1."""
    V = 10
    # (a) row 0: 8 at 0, 9 at -1; row 1: 8 at 0, 9 at -1, 7 at -1.  Valid: (8,9) -1, (8,7) -1, (9,8) -1, (9,7) -2.  (8,8) and (9,9) are excluded.
    # Lists of row 1: state r=0 (id 8): [(9,8) -1]; r=1 (id 7; the tie at -1 goes to the lower id): [(8,7) -1, (9,7) -2]; r=2 (id 9): [(8,9) -1].  Result order: total, r, j.
    x = np.full((1, 2, V), -9.0, np.float32)
    x[0, 0, 8], x[0, 0, 9] = 0.0, -1.0
    x[0, 1, 8], x[0, 1, 9], x[0, 1, 7] = 0.0, -1.0, -1.0
    r = nbest_nr_np(x, [2], 4)
    assert r["count"].tolist() == [4] and r["total"][0].tolist() == [-1.0, -1.0, -1.0, -2.0] and r["tie"][0]
    assert r["seq"][0].tolist() == [[9, 8], [8, 7], [8, 9], [9, 7]]
    assert nbest_np(x, [2], 1)["seq"][0, 0].tolist() == [8, 8]                 # the plain list's best repeats the word
    assert nbest_nr_np(x, [2], 1)["seq"][0].tolist() == [[9, 8]]
    # (b) two adjacent rows with one candidate each, the same word: no valid caption
    y = np.full((1, 3, V), -INF, np.float32)
    y[0, 0, 8] = y[0, 1, 8] = -1.0
    y[0, 2] = -np.arange(V, dtype=np.float32)
    z = nbest_nr_np(y, [3], 3, pad=5)
    assert z["count"].tolist() == [0] and (z["seq"] == 5).all() and (z["total"] == -INF).all() and not z["degenerate"][0]
    assert nbest_nr_np(y, [3], 3, pad=5, repeat_min_id=9)["count"].tolist() == [3]          # 8 is no word then: (8, 8, 0) ...
    # (c) a NaN leads a live row; a row of -inf alone; a row with every id banned: count 1, the per-row first unbanned ids, total NaN
    d = np.full((3, 2, 4), -1.0, np.float32)
    d[:, :, 2] = -0.5
    d[0, 1, 3] = NAN
    d[1, 0, :] = -INF
    q = nbest_nr_np(d, [2, 2, 2], 2, pad=9, repeat_min_id=0)
    assert q["degenerate"].tolist() == [True, True, False] and q["seq"][0, 0].tolist() == [2, 3] and q["seq"][1, 0].tolist() == [0, 2]
    assert np.isnan(q["total"][:2, 0]).all() and (q["total"][:2, 1] == -INF).all() and (q["seq"][:2, 1] == 9).all() and q["count"].tolist() == [1, 1, 2]
    assert q["seq"][2].tolist() == [[0, 2], [1, 2]]             # (2, 2) is excluded with repeat_min_id = 0; the ties at -1.5 by (r, j): state 0 (id 2) first
    allb = nbest_nr_np(d[2:], [2], 2, ban=(0, 1, 2, 3), pad=9)
    assert allb["degenerate"][0] and allb["seq"][0, 0].tolist() == [9, 9] and allb["count"].tolist() == [1]
    # (d) ids below repeat_min_id may repeat: the same rows under repeat_min_id = 7 keep (2, 2) in front
    assert nbest_nr_np(d[2:], [2], 2)["seq"][0].tolist() == [[2, 2], [0, 2]]
    # (e) n = 0: one empty caption of total 0; n = 1: the row's candidates
    e = nbest_nr_np(x, [0], 3, pad=5)
    assert e["count"].tolist() == [1] and e["total"][0].tolist() == [0.0, -INF, -INF] and (e["seq"] == 5).all()
    assert nbest_nr_np(x, [1], 3)["seq"][0, :, 0].tolist() == [8, 9, 0]


def _shared_leader_rows(rng, S=6, V=9):
    """Off-grid rows whose neighbours share leaders: on half of the rows, row p = row p-1 plus a small positive jitter."""
    x = np.log(rng.dirichlet(np.full(V, 0.4), (1, S)) + 1e-30).astype(np.float32)
    for p in range(1, S):
        if rng.random() < 0.5:
            x[0, p] = x[0, p - 1] + (rng.random(V) * 1e-2).astype(np.float32)
    return x


def test_against_the_plain_list_and_the_scan():
    """300 images of V = 9 whose neighbours share leaders, repeat_min_id = 0 (every id is a word).  The valid captions of the plain 8-list that lie strictly above its
    eighth total are, where no totals tie, the first entries of the no-repeat list, totals as bits.  Entry 0's total is >= the total of the scan's caption
    (``pick_np``, bofi_vocab_constrain's rule), which is valid but greedy."""
    rng = np.random.default_rng(22)
    S, N, lo = 6, 6, 0
    top_repeats = checked = better = 0
    for case in range(300):
        x = _shared_leader_rows(rng, S)
        n = int(rng.integers(2, S + 1))
        plain, nr = nbest_np(x, [n], 8), nbest_nr_np(x, [n], N, repeat_min_id=lo)
        assert plain["count"][0] == 8 and nr["count"][0] == N
        top_repeats += not is_valid(plain["seq"][0, 0, :n].tolist(), (), lo)
        if not plain["tie"][0] and not nr["tie"][0]:
            keep = [j for j in range(7) if plain["total"][0, j] > plain["total"][0, 7] and is_valid(plain["seq"][0, j, :n].tolist(), (), lo)][:N]
            assert np.array_equal(plain["seq"][0, keep], nr["seq"][0, :len(keep)]) and same_bits(plain["total"][0, keep], nr["total"][0, :len(keep)]), case
            checked += bool(keep)
        scan = pick_np(x, [n], (), True, lo)["seq"][0, :n]
        t = 0.0
        for p, i in enumerate(scan):
            t = t + float(x[0, p, i])
        assert is_valid(scan.tolist(), (), lo) and nr["total"][0, 0] >= t
        better += nr["total"][0, 0] > t
    print(f"shared leaders: the plain list's top caption repeats a word in {top_repeats} of 300 images; {checked} lists compared with the plain list's valid entries; "
          f"entry 0 beats the scan's caption in {better}")
    assert top_repeats >= 100 and checked >= 100


def _lib():
    from boficap_amd import hip
    assert os.path.exists(hip.LIB_PATH), "build the library first (python -m boficap_amd.build)"
    return hip, hip.lib()


def test_declarations_agree():
    """The entry point in header, ctypes table and library; BOFI_NBEST_NR_MAX; the per-call record and the ABI version as they were; test_nbest.py's pattern still
    finds one bofi_vocab_nbest( declaration."""
    from boficap_amd import build, hip
    header = open(os.path.join(ROOT, "include", "boficap_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    found = re.findall(r"\bbofi_vocab_nbest_norepeat\s*\(([^;{]*?)\)\s*;", code, flags=re.S)
    assert len(found) == 1 and found[0].count(",") + 1 == len(hip.SIGNATURES["bofi_vocab_nbest_norepeat"][1]) == 17
    assert len(re.findall(r"\bbofi_vocab_nbest\s*\(([^;{]*?)\)\s*;", code, flags=re.S)) == 1
    assert int(re.search(r"#define\s+BOFI_NBEST_NR_MAX\s+(\d+)", code).group(1)) == hip.NBEST_NR_MAX == 6
    assert C.sizeof(hip.BofiCallOpts) == 128 and hip.ABI_VERSION == 5
    kernels = open(os.path.join(build.CSRC, "bofi_kernels.h")).read()
    assert "launch_vocab_nbest_norepeat" in kernels and "vocab_nbest_norepeat_check" in kernels
    for stated in ("K = N + 2", "then r' ascending, then j ascending", "N + 1 are not enough", "strictly above the N-th total", "count may be 0"):
        assert stated in header, stated
    _, lib = _lib()
    assert hasattr(lib, "bofi_vocab_nbest_norepeat") and callable(hip.vocab_nbest_norepeat) and lib.bofi_abi_version() == 5


def test_entry_point_refuses_bad_arguments_without_a_device():
    """Each returns BOFI_ERR_ARG (1) from the argument check, with a message: the pointers are never read, nothing is launched.  rows = 0 is BOFI_OK."""
    hip, lib = _lib()
    p = C.c_void_p(0x1000)
    need = lib.bofi_vocab_nbest_workspace(40)
    good = dict(x=p, ldx=9491, rows=40, V=9491, S=20, ntok=None, ntok_bias=0, pad=0, ban=None, lo=7, N=5, seq_n=p, total=p, count=p, work=p, work_bytes=need)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.bofi_vocab_nbest_norepeat(a["x"], a["ldx"], a["rows"], a["V"], a["S"], a["ntok"], a["ntok_bias"], a["pad"], a["ban"], a["lo"], a["N"], a["seq_n"],
                                           a["total"], a["count"], a["work"], a["work_bytes"], None)
        if rc == 1:
            assert lib.bofi_last_error().startswith(b"vocab_nbest_norepeat: "), (kw, lib.bofi_last_error())
        return rc

    assert call(x=None) == 1 and call(seq_n=None) == 1 and call(total=None) == 1 and call(count=None) == 1
    assert call(rows=41) == 1 and call(rows=-20) == 1
    assert call(V=1) == 1 and call(ldx=9490) == 1
    assert call(S=0, rows=0) == 1 and call(S=65, rows=65) == 1 and b"S in 1..64" in lib.bofi_last_error()
    assert call(N=0) == 1 and call(N=7) == 1 and b"N in 1..6" in lib.bofi_last_error()
    assert call(N=8) == 1 and call(N=-1) == 1
    assert call(lo=-1) == 1 and b"repeat_min_id" in lib.bofi_last_error()
    assert call(work=None) == 1 and call(work_bytes=need - 1) == 1 and call(work_bytes=-1) == 1 and b"workspace" in lib.bofi_last_error()
    assert call(rows=0) == 0 and call(rows=0, work=None, work_bytes=0, S=64, N=6, lo=0) == 0


def test_engine_keywords_are_validated_on_the_host():
    from boficap_amd import hip
    from boficap_amd.engine import BofiEngine
    on = BofiEngine._nbest_no_repeat
    assert on(0, False) is None and on(5, False) is None and on(5, 0) is None and on(0, None) is None
    assert on(5, True) == 7 and on(6, 1, 0) == 0 and on(1, True, 12) == 12
    with pytest.raises(hip.BofiHipError, match="needs nbest") as e:
        on(0, True)
    assert "nbest_no_repeat" in str(e.value)
    for bad in (7, 8):
        with pytest.raises(hip.BofiHipError, match=r"1\.\.6") as e:
            on(bad, True)
        assert "nbest_no_repeat" in str(e.value)
    with pytest.raises(hip.BofiHipError, match="repeat_min_id"):
        on(3, True, -1)
    # the list and the constrained decode still exclude each other, and the refusal points to the option
    with pytest.raises(hip.BofiHipError, match="no_repeat") as e:
        BofiEngine._nbest_refusals(None, False, 0, True, False, False, True)
    assert "nbest_no_repeat" in str(e.value)
    assert BofiEngine._nbest_width(8) == 8                      # (the plain list keeps its width)


def test_eval_options_resolve_and_refuse():
    from boficap_amd import eval_utils as E
    assert E.nbest_no_repeat_of({}) is False and E.nbest_no_repeat_of({"nbest_no_repeat": 0}, 9) is False
    assert E.nbest_no_repeat_of({"nbest_no_repeat": 1, "sample_n_method": "nbest"}, 6) is True
    assert E.nbest_no_repeat_of({"nbest_no_repeat": 1, "sample_n_method": "nbest"}, 1) is True
    for kw, n, word in (({}, 3, "sample_n_method"), ({"sample_n_method": "sample"}, 3, "sample_n_method"), ({"sample_n_method": "nbest"}, 7, "at most 6"),
                        ({"sample_n_method": "nbest"}, 8, "at most 6")):
        with pytest.raises(ValueError, match=word) as e:
            E.nbest_no_repeat_of(dict(kw, nbest_no_repeat=1), n)
        assert "nbest_no_repeat" in str(e.value)
    # the constrained decode with the list stays refused, with or without the key; the plain list keeps its 8
    for kw in ({"decoding_constraint": 1}, {"decoding_constraint": 1, "nbest_no_repeat": 1}):
        with pytest.raises(ValueError, match="decoding_constraint"):
            E.sample_n_method_of(dict(kw, sample_n_method="nbest"), "NAIC", 3)
    assert E.sample_n_method_of({"sample_n_method": "nbest"}, "NAIC", 8) == "nbest"


@pytest.mark.parametrize("args,word", [(["--nbest_no_repeat", "1", "--sample_n", "3"], "sample_n_method"),
                                       (["--nbest_no_repeat", "1", "--sample_n", "3", "--sample_n_method", "sample"], "sample_n_method"),
                                       (["--nbest_no_repeat", "1", "--sample_n", "7", "--sample_n_method", "nbest"], "at most 6"),
                                       (["--nbest_no_repeat", "1", "--sample_n", "3", "--sample_n_method", "nbest", "--decoding_constraint", "1"], "decoding_constraint"),
                                       (["--nbest_no_repeat", "2", "--sample_n", "3", "--sample_n_method", "nbest"], "invalid choice")])
def test_eval_tool_refuses_the_option_where_it_cannot_apply(args, word):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval.py"), *args, "--synthetic", "8"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 2 and word in r.stderr, r.stderr
    assert "nbest_no_repeat" in r.stderr
