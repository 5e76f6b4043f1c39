"""The N most probable captions of the NAIC filling pass, host side (no GPU): the rule of ``bofi_vocab_nbest`` (include/boficap_hip.h states it in words) RESTATED in
numpy (``nbest_np``: the candidates in ``order_np``'s order, the float64 recurrence, the tie order), held against a BRUTE FORCE over every caption -- what
tests/test_gpu_nbest.py holds the kernel and the engines to --, the prefix property, the declarations, and the refusals that need no device.  The reference's
``sample_n_method='bs'`` returns the N best of a beam; for a pass that scores every position on its own the N best are no search."""
import ctypes as C
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_constrained_pick import order_np

NAN, INF = float("nan"), float("inf")


# ----------------------------------------------------------------------------- the rule, restated
def nbest_np(x, n, N, ban=(), pad=0):
    """The N-best lists of x [B, S, >= V] (all of x.shape[2] columns are the vocabulary) with n [B] live positions (clamped to 0 .. S): a dict of ``seq`` int64
    [B, N, S], ``total`` float64 [B, N], ``count`` int32 [B], and for the tests' own statistics ``tie`` bool [B] (two pairs of some step had the same total),
    ``degenerate`` bool [B] and ``cands`` (per image the list of its live rows' candidate counts)."""
    x = np.asarray(x)
    B, S, _ = x.shape
    ban = sorted({int(i) for i in ban})
    seq = np.full((B, N, S), pad, np.int64)
    total = np.full((B, N), -INF, np.float64)
    count = np.zeros(B, np.int32)
    tie, degenerate, cands = np.zeros(B, bool), np.zeros(B, bool), []
    for b in range(B):
        nb = min(max(int(n[b]), 0), S)
        rows = []
        for p in range(nb):
            order = [int(i) for i in order_np(x[b, p], ban)[:N]]
            first = order[0] if order else None
            if first is None or not np.isfinite(x[b, p, first]):
                degenerate[b] = True
            rows.append((first, [(r, i, float(x[b, p, i])) for r, i in enumerate(order) if r == 0 or np.isfinite(x[b, p, i])]))
        cands.append([len(c) for _, c in rows])
        if degenerate[b]:
            count[b], total[b, 0] = 1, NAN
            seq[b, 0, :nb] = [pad if first is None else first for first, _ in rows]
            continue
        L = [(0.0, [])]
        for _, c in rows:
            pairs = [(T + v, i, r, ids + [cid]) for i, (T, ids) in enumerate(L) for r, cid, v in c]      # (python floats: one float64 add per pair)
            pairs.sort(key=lambda t: (-t[0], t[1], t[2]))
            tie[b] |= len({t[0] for t in pairs}) < len(pairs)
            L = [(t[0], t[3]) for t in pairs[:N]]
        count[b] = len(L)
        for j, (T, ids) in enumerate(L):
            total[b, j] = T
            seq[b, j, :nb] = ids
    return dict(seq=seq, total=total, count=count, tie=tie, degenerate=degenerate, cands=cands)


def brute_np(x, n, ban=()):
    """Every caption of one image x [S, V] over the unbanned ids with its total, the float64 sum taken left to right: [(total, ids)], best total first."""
    ids = [i for i in range(x.shape[1]) if i not in set(ban)]
    out = []
    for cap in itertools.product(ids, repeat=n):
        T = 0.0
        for p, i in enumerate(cap):
            T = T + float(x[p, i])
        out.append((T, cap))
    out.sort(key=lambda t: -t[0])
    return out


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.int64), np.asarray(b, np.float64).view(np.int64))


# ----------------------------------------------------------------------------- tests
def test_hand_worked_case():
    """Two positions, three ids, N = 4.  Row 0: ids 2, 0, 1 at 0, -1, -3; row 1: ids 1, 2, 0 at -0.5, -0.5 (the tie goes to the lower id), -2."""
    x = np.array([[[-1.0, -3.0, 0.0], [-2.0, -0.5, -0.5]]], np.float32)
    r = nbest_np(x, [2], 4)
    assert r["count"].tolist() == [4] and r["total"][0].tolist() == [-0.5, -0.5, -1.5, -1.5]
    assert r["seq"][0].tolist() == [[2, 1], [2, 2], [0, 1], [0, 2]] and r["tie"][0]
    # n = 0: one empty caption of total 0; N = 1 is the per-row first id
    z = nbest_np(x, [0], 3, pad=5)
    assert z["count"].tolist() == [1] and z["total"][0].tolist() == [0.0, -INF, -INF] and (z["seq"] == 5).all()
    assert nbest_np(x, [2], 1)["seq"][0].tolist() == [[2, 1]]


def test_list_equals_the_brute_force_over_every_caption():
    """Values on a grid of eighths in [-8, 0] (sums exact, ties frequent), n_b in 0..4, V in 2..6, N in 1..8, with and without a ban: the totals are the brute force's N
    best totals, the captions strictly above the last total are the same set, entry 0 is the per-row first id, the rows are distinct, the totals do not increase, and
    count = min(N, product of the rows' candidate counts)."""
    rng = np.random.default_rng(20)
    ties = 0
    for case in range(600):
        V, S, N = int(rng.integers(2, 7)), 4, int(rng.integers(1, 9))
        n = int(rng.integers(0, 5))
        x = (-rng.integers(0, 65, (1, S, V)) / 8.0).astype(np.float32)
        if case % 3 == 0:
            x = (-rng.integers(0, 5, (1, S, V)) / 8.0).astype(np.float32)      # a coarse grid: many ties
        ban = tuple(int(i) for i in rng.choice(V, int(rng.integers(0, V - 1)), replace=False)) if case % 2 else ()
        r = nbest_np(x, [n], N, ban, pad=0)
        c = int(r["count"][0])
        all_caps = brute_np(x[0], n, ban)
        assert c == min(N, len(all_caps)) == min(N, int(np.prod([min(N, V - len(ban))] * n))) == min(N, int(np.prod(r["cands"][0])))
        assert r["total"][0, :c].tolist() == [t for t, _ in all_caps[:c]], (case, r["total"], all_caps[:c])
        assert (r["total"][0, c:] == -INF).all() and (r["seq"][0, c:] == 0).all() and (r["seq"][0, :, n:] == 0).all()
        got = [tuple(int(v) for v in r["seq"][0, j, :n]) for j in range(c)]
        assert len(set(got)) == c
        last = r["total"][0, c - 1]
        assert {cap for t, cap in all_caps if t > last} == {cap for cap, t in zip(got, r["total"][0, :c]) if t > last}, case
        assert all(float(sum(np.float64(x[0, p, i]) for p, i in enumerate(cap))) == t for cap, t in zip(got, r["total"][0, :c]))
        assert got[0] == tuple(int(order_np(x[0, p], ban)[0]) for p in range(n))
        assert (np.diff(r["total"][0, :c]) <= 0).all() and not r["degenerate"][0]
        ties += bool(r["tie"][0])
    assert ties > 100


@pytest.mark.parametrize("grid", [True, False])
def test_first_entries_of_the_n_list_are_the_shorter_list(grid):
    """N = 8 against N' = 1..7, bit for bit on seq, total and count -- on the grid and on float32 values NOT on a grid, where every float64 add rounds."""
    rng = np.random.default_rng(21 + grid)
    B, S, V = 40, 9, 12
    x = (-rng.integers(0, 17, (B, S, V)) / 8.0).astype(np.float32) if grid else np.log(rng.dirichlet(np.full(V, 0.3), (B, S)) + 1e-30).astype(np.float32)
    n = rng.integers(0, S + 1, B)
    n[0], n[1] = S, 1
    ban = (3, 7)
    full = nbest_np(x, n, 8, ban)
    assert (full["count"][n >= 2] == 8).all()
    for Np in range(1, 8):
        part = nbest_np(x, n, Np, ban)
        assert np.array_equal(part["count"], np.minimum(full["count"], Np))
        assert np.array_equal(part["seq"], full["seq"][:, :Np]) and same_bits(part["total"], full["total"][:, :Np]), Np


def test_bans_candidates_that_are_not_finite_and_the_degenerate_image():
    x = np.array([[[-1.0, -0.5, -2.0, -INF, -0.25], [-0.5, -1.0, -INF, -3.0, -INF]],
                  [[-1.0, NAN, -2.0, -3.0, -4.0], [-0.5, -1.0, -2.0, -3.0, -4.0]],
                  [[-1.0, -0.5, -2.0, -3.0, -4.0], [-INF, -INF, -INF, -INF, -INF]],
                  [[INF, -0.5, -2.0, -3.0, -4.0], [-0.5, -1.0, -2.0, -3.0, -4.0]]], np.float32)
    r = nbest_np(x, [2, 2, 2, 2], 4, ban=(4,), pad=9)
    # image 0: row 0 has ids 1, 0, 2 (and -inf at 3: ranked fourth, no candidate); row 1 has ids 0, 1, 3 (-inf at 2 ranks fourth: dropped)
    assert r["cands"][0] == [3, 3] and r["count"][0] == 4 and not r["degenerate"][0]
    assert r["seq"][0].tolist() == [[1, 0], [1, 1], [0, 0], [0, 1]] and r["total"][0].tolist() == [-1.0, -1.5, -1.5, -2.0]      # (the tie: i ascending first)
    assert 4 not in r["seq"][0]
    # a NaN leads its row; a row of -inf alone; a +inf at the head: count 1, the per-row first unbanned ids, total NaN
    for b, first in ((1, [1, 0]), (2, [1, 0]), (3, [0, 0])):
        assert r["degenerate"][b] and r["count"][b] == 1 and np.isnan(r["total"][b, 0]) and (r["total"][b, 1:] == -INF).all()
        assert r["seq"][b, 0].tolist() == first and (r["seq"][b, 1:] == 9).all()
    # -inf candidates of rank >= 1 are dropped: two rows of two candidates each
    y = np.array([[[-1.0, -INF, -2.0, -INF], [-1.0, -2.0, -INF, -INF]]], np.float32)
    q = nbest_np(y, [2], 3)
    assert q["cands"][0] == [2, 2] and q["seq"][0].tolist() == [[0, 0], [0, 1], [2, 0]]      # (ties: -3 twice, i ascending first)
    # everything banned but one id: one caption
    one = nbest_np(y, [2], 3, ban=(1, 2, 3))
    assert one["count"].tolist() == [1] and one["seq"][0, 0].tolist() == [0, 0]


def _lib():
    from boficap_amd import hip
    assert os.path.exists(hip.LIB_PATH), "build the library first (python -m boficap_amd.build)"
    return hip, hip.lib()


def test_declarations_agree():
    """The two entry points in header, ctypes table and library; BOFI_NBEST_MAX; the per-call record and the ABI version as they were: new symbols, not a field."""
    from boficap_amd import build, hip
    header = open(os.path.join(ROOT, "include", "boficap_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, arity in (("bofi_vocab_nbest", 16), ("bofi_vocab_nbest_workspace", 1)):
        found = re.findall(r"\b" + name + r"\s*\(([^;{]*?)\)\s*;", code, flags=re.S)
        assert len(found) == 1 and found[0].count(",") + 1 == len(hip.SIGNATURES[name][1]) == arity, name
    assert int(re.search(r"#define\s+BOFI_NBEST_MAX\s+(\d+)", code).group(1)) == hip.NBEST_MAX == 8
    assert C.sizeof(hip.BofiCallOpts) == 128 and hip.ABI_VERSION == 5
    assert "launch_vocab_nbest" in open(os.path.join(build.CSRC, "bofi_kernels.h")).read()
    for stated in ("then i ascending, then r ascending", "bit for bit", "strictly above the N-th total"):
        assert stated in header
    _, lib = _lib()
    assert hasattr(lib, "bofi_vocab_nbest") and callable(hip.vocab_nbest) and lib.bofi_abi_version() == 5
    assert lib.bofi_vocab_nbest_workspace(0) == 0 and lib.bofi_vocab_nbest_workspace(40) == lib.bofi_vocab_pick_workspace(40) > 0


def test_entry_point_refuses_bad_arguments_without_a_device():
    """Each returns BOFI_ERR_ARG (1) from the argument check, with a message: the pointers are never read, nothing is launched.  rows = 0 is BOFI_OK."""
    hip, lib = _lib()
    p = C.c_void_p(0x1000)
    need = lib.bofi_vocab_nbest_workspace(40)
    good = dict(x=p, ldx=9491, rows=40, V=9491, S=20, ntok=None, ntok_bias=0, pad=0, ban=None, N=5, seq_n=p, total=p, count=p, work=p, work_bytes=need)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.bofi_vocab_nbest(a["x"], a["ldx"], a["rows"], a["V"], a["S"], a["ntok"], a["ntok_bias"], a["pad"], a["ban"], a["N"], a["seq_n"], a["total"], a["count"],
                                  a["work"], a["work_bytes"], None)
        if rc == 1:
            assert b"vocab_nbest" in lib.bofi_last_error(), kw
        return rc

    assert call(x=None) == 1 and call(seq_n=None) == 1 and call(total=None) == 1 and call(count=None) == 1
    assert call(rows=41) == 1 and call(rows=-20) == 1
    assert call(V=1) == 1 and call(ldx=9490) == 1
    assert call(S=0, rows=0) == 1 and call(S=65, rows=65) == 1 and b"S in 1..64" in lib.bofi_last_error()
    assert call(N=0) == 1 and call(N=9) == 1 and b"N in 1..8" in lib.bofi_last_error()
    assert call(work=None) == 1 and call(work_bytes=need - 1) == 1 and call(work_bytes=-1) == 1 and b"workspace" in lib.bofi_last_error()
    assert call(rows=0) == 0 and call(rows=0, work=None, work_bytes=0, S=64, N=8) == 0


def test_engine_keywords_are_validated_on_the_host():
    from boficap_amd import hip
    from boficap_amd.engine import BofiEngine
    width = BofiEngine._nbest_width
    assert width(None) == 0 and width(0) == 0 and width(1) == 1 and width(8) == 8
    for bad in (9, -1, 100):
        with pytest.raises(hip.BofiHipError, match="1..8"):
            width(bad)
    refuse = BofiEngine._nbest_refusals
    for args, word in (((True, 0, False, False, False, True), "ids_only"), ((False, hip.FLAG_MASK_PREDICT, False, False, False, True), "mask_predict"),
                       ((False, 0, True, False, False, True), "no_repeat"), ((False, 0, False, True, False, True), "block_trigrams"),
                       ((False, 0, False, False, True, True), "require_ids")):
        with pytest.raises(hip.BofiHipError, match=word) as e:
            refuse(None, *args)
        assert "nbest" in str(e.value)
    refuse(None, False, 0, False, False, False, True)


def test_eval_options_resolve_and_refuse():
    from boficap_amd import eval_utils as E
    assert E.sample_n_method_of({}) == "sample" and E.sample_n_method_of({"sample_n_method": "sample"}, "SAIC", 5) == "sample"
    assert E.sample_n_method_of({"sample_n_method": "nbest"}, "NAIC", 8) == "nbest"
    assert E.sample_n_method_of({"sample_n_method": "nbest"}, "SAIC", 1) == "nbest"       # (one caption per image: the key does nothing)
    with pytest.raises(ValueError, match="'sample'.*'nbest'"):
        E.sample_n_method_of({"sample_n_method": "bs"})
    for kw, mode, n, word in (({}, "SAIC", 3, "NAIC"), ({}, "NAIC", 9, "at most 8"), ({"refine_method": "mask_predict"}, "NAIC", 3, "mask_predict"),
                              ({"decoding_constraint": 1}, "NAIC", 3, "decoding_constraint"), ({"block_trigrams": 1}, "NAIC", 3, "block_trigrams")):
        with pytest.raises(ValueError, match=word) as e:
            E.sample_n_method_of(dict(kw, sample_n_method="nbest"), mode, n)
        assert "nbest" in str(e.value)
    vocab = {"7": "a", "8": "UNK", "9": "dog"}
    # banned ids go with the list; rules that couple neighbours do not; without the method sample_n > 1 refuses all four as before
    assert E.constraint_of({"suppress_UNK": 1, "ban_words": "dog", "sample_n_method": "nbest"}, vocab, "NAIC", 3) == {"ban_ids": [8, 9], "no_repeat": False}
    for kw in ({"decoding_constraint": 1}, {"block_trigrams": 1}, {"suppress_UNK": 1, "decoding_constraint": 1}):
        with pytest.raises(ValueError, match="sample_n"):
            E.constraint_of(dict(kw, sample_n_method="nbest"), vocab, "NAIC", 3)
    for method in ({}, {"sample_n_method": "sample"}):
        with pytest.raises(ValueError, match="sample_n"):
            E.constraint_of(dict(method, suppress_UNK=1), vocab, "NAIC", 3)
    with pytest.raises(ValueError, match="sample_n"):          # required words still refuse N captions per image
        E.required_of({"require_words": ["dog"], "sample_n_method": "nbest"}, vocab, [0], "NAIC", 3)
    with pytest.raises(ValueError, match="'sample' and 'nbest'"):
        E.sample_n_predictions(None, np.zeros((2, 3, 4), np.float32), 3, method="bs")
    with pytest.raises(ValueError, match="NAIC"):
        E.sample_n_predictions(None, np.zeros((2, 3, 4), np.float32), 3, mode="SAIC", method="nbest")


@pytest.mark.parametrize("args,word", [(["--sample_n_method", "nbest", "--sample_n", "3", "--inference_mode", "SAIC"], "NAIC"),
                                       (["--sample_n_method", "nbest", "--sample_n", "9"], "at most 8"),
                                       (["--sample_n_method", "nbest", "--sample_n", "3", "--refine_rounds", "2", "--refine_method", "mask_predict"], "mask_predict"),
                                       (["--sample_n_method", "nbest", "--sample_n", "3", "--decoding_constraint", "1"], "decoding_constraint"),
                                       (["--sample_n_method", "nbest", "--sample_n", "3", "--block_trigrams", "1"], "block_trigrams"),
                                       (["--sample_n_method", "nbest", "--sample_n", "3", "--require_words", "a"], "sample_n"),
                                       (["--sample_n_method", "bs", "--sample_n", "3"], "invalid choice")])
def test_eval_tool_refuses_the_list_where_it_cannot_be_made(args, word):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval.py"), *args, "--synthetic", "8"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 2 and word in r.stderr, r.stderr
