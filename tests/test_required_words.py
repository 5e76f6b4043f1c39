"""Required words of the NAIC decode, host side (no GPU): the rule of ``bofi_vocab_require`` (include/boficap_hip.h states it in words) RESTATED in numpy
(``require_np``: the backward recurrence in float64 and the forward walk), held against a hand-worked case and against a BRUTE FORCE over every injective placement
that applies the stated preference order directly -- what tests/test_gpu_required_words.py holds the kernel and the engine to --, the declarations, and the refusals
that need no device.  The reference has no such option: its lexically constrained decoding would be a constrained beam on the autoregressive path."""
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

NAN, INF = float("nan"), float("inf")
KEEP = 255


# ----------------------------------------------------------------------------- the rule, restated
def classify_np(row, V, ban=()):
    """The entries of one word row: the id of a required word, -1 for an empty entry, -2 for a skipped one (>= V, banned, a repeat of an earlier entry)."""
    ban = {int(i) for i in ban}
    out = []
    for j, w in enumerate(int(v) for v in row):
        if w < 0:
            out.append(-1)
        elif w >= V or w in ban or w in [int(v) for v in row[:j]]:
            out.append(-2)
        else:
            out.append(w)
    return out


def gains_np(x, n, f, seq, no_repeat=False, min_id=7):
    """gain float64 [n, K] and eligible bool [n, K] of one image: x [S, V], f the classified word row, seq the ids on entry."""
    V, K = x.shape[1], len(f)
    gain, ok = np.zeros((n, K), np.float64), np.zeros((n, K), bool)
    for p in range(n):
        here = int(seq[p])
        for j, w in enumerate(f):
            if w < 0:
                continue
            if here == w:
                ok[p, j] = True
                continue
            a = np.float64(x[p, w])
            b = np.float64(x[p, here]) if 0 <= here < V else np.float64(NAN)      # (an id outside the vocabulary has no value)
            if np.isfinite(a) and np.isfinite(b):
                gain[p, j], ok[p, j] = a - b, True
            if no_repeat and w >= min_id and ((p > 0 and int(seq[p - 1]) == w) or (p + 1 < n and int(seq[p + 1]) == w)):
                ok[p, j] = False
    return gain, ok


def require_np(x, n, words, seq, ban=(), no_repeat=False, min_id=7, chosen=None):
    """``bofi_vocab_require`` on x [B, S, V] with n [B] live positions (clamped to 0 .. S), words int [B, K] and the ids on entry seq [B, S]: a dict of ``seq`` int64
    [B, S], ``chosen`` float32 [B, S] (x at every placed word; what ``chosen`` held -- zeros without it -- elsewhere), ``pos`` int32 [B, K], ``moved`` int32 [B] and
    ``margin`` float64 [B]: the smallest gap, along the forward walk, between the chosen option's value and the next-best option's -- inf where their counts differ or
    where there was one option, else the difference of the totals."""
    x, words = np.asarray(x), np.asarray(words)
    B, S, V = x.shape
    K = words.shape[1]
    out = np.array(seq, np.int64, copy=True)
    ch = np.zeros((B, S), np.float32) if chosen is None else np.array(chosen, np.float32, copy=True)
    pos = np.zeros((B, K), np.int32)
    moved = np.zeros(B, np.int32)
    margin = np.full(B, INF)
    M = 1 << K
    for b in range(B):
        nb = min(max(int(n[b]), 0), S)
        f = classify_np(words[b], V, ban)
        gain, ok = gains_np(x[b], nb, f, out[b], no_repeat, min_id)
        cnt = np.zeros((nb + 1, M), np.int64)
        tot = np.zeros((nb + 1, M), np.float64)
        opts = [[None] * M for _ in range(nb)]                  # the options of every node, in order: (choice, count, total)
        choice = np.full((nb, M), KEEP, np.int64)
        for p in range(nb - 1, -1, -1):
            for m in range(M):
                o = [(j, 1 + cnt[p + 1, m ^ (1 << j)], gain[p, j] + tot[p + 1, m ^ (1 << j)]) for j in range(K) if (m >> j) & 1 and ok[p, j]]
                o.append((KEEP, cnt[p + 1, m], tot[p + 1, m]))
                best = o[0]
                for c in o[1:]:
                    if c[1] > best[1] or (c[1] == best[1] and c[2] > best[2]):      # strictly greater only: the first best option stays
                        best = c
                opts[p][m] = o
                choice[p, m], cnt[p, m], tot[p, m] = best
        m = sum(1 << j for j, w in enumerate(f) if w >= 0)
        pos[b] = [-3 if w >= 0 else w for w in f]
        for p in range(nb):
            if not m:
                break
            o, c = opts[p][m], int(choice[p, m])
            mine = next(v for v in o if v[0] == c)
            for v in o:
                if v[0] != c:
                    margin[b] = min(margin[b], INF if v[1] != mine[1] else float(mine[2] - v[2]))
            if c == KEEP:
                continue
            pos[b, c] = p
            moved[b] += int(out[b, p] != f[c])
            out[b, p], ch[b, p] = f[c], x[b, p, f[c]]
            m ^= 1 << c
    return dict(seq=out, chosen=ch, pos=pos, moved=moved, margin=margin)


def brute_np(x, n, f, seq, no_repeat=False, min_id=7):
    """The placement of one image WITHOUT a recurrence: every injective map of a subset of the required words to eligible live positions, preferred first by the number
    of words placed, then by the total gain (the inputs are multiples of 2^-3: every sum is exact in any order), then -- reading left to right -- by a position taking a
    word over keeping its id, the earliest-listed word first.  Returns the position of every word (None: not placed)."""
    gain, ok = gains_np(x, n, f, seq, no_repeat, min_id)
    req = [j for j, w in enumerate(f) if w >= 0]
    best, best_key = None, None
    for where in itertools.product([None] + list(range(n)), repeat=len(req)):
        used = [p for p in where if p is not None]
        if len(set(used)) != len(used) or any(p is not None and not ok[p, j] for j, p in zip(req, where)):
            continue
        total = sum(gain[p, j] for j, p in zip(req, where) if p is not None)
        takes = [len(f)] * n                                     # per position: the word it takes, K for "keeps its id"
        for j, p in zip(req, where):
            if p is not None:
                takes[p] = j
        key = (-len(used), -total, takes)
        if best_key is None or key < best_key:
            best, best_key = dict(zip(req, where)), key
    return best


# ----------------------------------------------------------------------------- tests
def _hand_case():
    S, V, K = 5, 12, 4
    x = np.full((4, S, V), -4.0, np.float32)
    seq = np.array([[9, 9, 8, 3, 5], [9, 10, 9, 5, 5], [9, 9, 9, 9, 9], [9, 5, 5, 5, 5]], np.int64)
    for b in range(4):
        for p in range(S):
            x[b, p, seq[b, p]] = -0.5                           # every standing id at -0.5
    x[0, :4, 10] = [-1.0, -0.75, -2.0, -0.75]
    x[0, :4, 8] = [-3.0, -3.0, -0.5, -3.0]
    x[1, :3, 11] = [-0.625, -0.5, NAN]
    x[1, :3, 10] = [-1.5, -0.5, -1.0]
    x[3, 0, 10] = x[3, 0, 11] = -1.0
    words = np.array([[10, 8, -1, -1], [11, 10, 10, 99], [7, -1, -1, -1], [10, 11, -1, -1]], np.int32)
    return x, [4, 3, 0, 1], words, seq


def test_require_np_on_a_hand_worked_case():
    """S = 5, V = 12, K = 4; every standing id has -0.5; worked by hand.

    Image 0, n = 4, seq 9 9 8 3, words 10 and 8.  Word 8 stands at position 2 (gain 0 there, -2.5 elsewhere); word 10 gains -0.5, -0.25, -1.5, -0.25.  Both are placed;
    the best total is 0 - 0.25, with 10 at position 1 or 3: an exact tie.  Walk: position 0 keeps (10 there: -0.5; keep: -0.25).  Position 1: "takes 10" (-0.25 + 0) and
    "keeps" (10 at position 3: -0.25) tie -- the first option in the order wins: 10 at position 1.  Position 2 takes 8 (0 against -2.5).  9 10 8 3 | pos 1 2 | moved 1
    (position 2 already held its word) | margin 0.
    Image 1, n = 3, seq 9 10 9, words 11, 10, 10 again (skipped), 99 (>= V: skipped).  11 gains -0.125, 0.0, NaN (ineligible at 2); 10 gains -1, 0 (it stands at 1),
    -0.5.  Placements of both: 11@0 10@1 = -0.125; 11@1 10@2 = -0.5; 11@1 10@0 = -1; 11@0 10@2 = -0.625.  11 10 9 | pos 0 1 -2 -2 | moved 1.  Position 0: -0.125
    against keep -0.5 and "takes 10" -1: gap 0.375; position 1: 0 against -0.5.  margin 0.375.  With no_repeat, 10 is ineligible at positions 0 and 2 (their neighbour
    holds it): the same result, and every other option now places fewer words: margin inf.
    Image 2: n = 0 -- the word is required but unplaceable: -3.  Image 3: n = 1, two words with equal gains for one position: the earlier-listed one takes it."""
    x, n, words, seq = _hand_case()
    r = require_np(x, n, words, seq)
    assert r["seq"].tolist() == [[9, 10, 8, 3, 5], [11, 10, 9, 5, 5], [9, 9, 9, 9, 9], [10, 5, 5, 5, 5]]
    assert r["pos"].tolist() == [[1, 2, -1, -1], [0, 1, -2, -2], [-3, -1, -1, -1], [0, -3, -1, -1]]
    assert r["moved"].tolist() == [1, 1, 0, 1]
    assert r["margin"].tolist() == [0.0, 0.375, INF, 0.0]
    want = np.zeros((4, 5), np.float32)
    want[0, 1], want[0, 2], want[1, 0], want[1, 1], want[3, 0] = -0.75, -0.5, -0.625, -0.5, -1.0
    assert np.array_equal(r["chosen"], want)
    rep = require_np(x, n, words, seq, no_repeat=True, chosen=np.full((4, 5), 7.0, np.float32))
    assert np.array_equal(rep["seq"], r["seq"]) and np.array_equal(rep["pos"], r["pos"]) and rep["margin"].tolist() == [0.0, INF, INF, 0.0]
    assert rep["chosen"][0].tolist() == [7.0, -0.75, -0.5, 7.0, 7.0]            # (what stood in row_chosen stays where no word was placed)
    # a banned word is skipped (image 1: 11 alone now takes position 1, where it costs nothing)
    ban = require_np(x, n, words, seq, ban=[10])
    assert ban["pos"].tolist() == [[-2, 2, -1, -1], [1, -2, -2, -2], [-3, -1, -1, -1], [-2, 0, -1, -1]] and ban["seq"][3, 0] == 11 and ban["seq"][1].tolist() == [9, 11, 9, 5, 5]
    assert classify_np([3, 3, -5, 12, 11], 12, ban=[11]) == [3, -2, -1, -2, -2]


def _random_case(rng, S, K, V=16):
    vals = np.array([-0.125, -0.25, -0.25, -0.5, -0.5, -1.0], np.float32)      # few multiples of 2^-3: exact ties are frequent
    x = rng.choice(vals, size=(S, V)).astype(np.float32)
    bad = rng.random((S, V)) < 0.06
    x[bad] = rng.choice(np.array([NAN, INF, -INF], np.float32), size=int(bad.sum()))
    words = rng.integers(5, 12, size=K)                         # around min_id = 7, with duplicates
    words[rng.random(K) < 0.15] = -1
    words[rng.random(K) < 0.08] = V + 3
    seq = rng.integers(5, 12, size=S)                           # the same range: entries of seq equal required words, also next to each other
    return x, int(rng.integers(0, S + 1)), words.astype(np.int32), seq.astype(np.int64)


def test_require_np_equals_the_brute_force():
    """Every injective placement enumerated, S <= 7, K <= 3, V = 16; inputs multiples of 2^-3 with NaN and +-inf rows, ties, words already standing in seq and next to
    each other, with and without the adjacency rule and a ban."""
    rng = np.random.default_rng(20260)
    tied = placed_standing = barred = 0
    for it in range(600):
        S, K = int(rng.integers(1, 8)), int(rng.integers(1, 4))
        x, n, words, seq = _random_case(rng, S, K)
        rep, ban = bool(it & 1), ([int(words[0])] if it % 7 == 0 and words[0] >= 0 else [])
        r = require_np(x[None], [n], words[None], seq[None], ban=ban, no_repeat=rep)
        f = classify_np(words, 16, ban)
        want = brute_np(x, n, f, seq, rep)
        got = {j: (int(r["pos"][0, j]) if r["pos"][0, j] >= 0 else None) for j, w in enumerate(f) if w >= 0}
        assert got == want, (it, S, K, n, words, seq, rep, ban)
        assert [int(v) for j, v in enumerate(r["pos"][0]) if f[j] < 0] == [w for w in f if w < 0]
        after = seq.copy()
        for j, p in want.items():
            if p is not None:
                after[p] = f[j]
                placed_standing += int(seq[p] == f[j])
        assert np.array_equal(r["seq"][0], after) and r["moved"][0] == int((after != seq).sum())
        tied += int(r["margin"][0] == 0.0)
        if rep:
            _, ok_free = gains_np(x, min(n, S), f, seq, False)
            _, ok_rep = gains_np(x, min(n, S), f, seq, True)
            barred += int((ok_free & ~ok_rep).sum())
            for p in range(1, n):                                # a placement never creates an adjacent repeat of a word
                assert not (after[p] == after[p - 1] and after[p] >= 7 and (after[p] != seq[p] or after[p - 1] != seq[p - 1])), (it, seq, after)
    print(f"tied {tied}, words placed where they stood {placed_standing}, pairs barred by the adjacency rule {barred}")
    assert tied >= 60 and placed_standing >= 60 and barred >= 60      # a tenth of the 600 cases each: the cases are not vacuous


def test_require_table_is_checked_on_the_host():
    from boficap_amd import hip
    t = hip.require_table([[3, 4], [], [5, 5, -1, 6]], 3, 10)
    assert t.dtype == torch.int32 and t.tolist() == [[3, 4], [-1, -1], [5, 6]]      # (a row's duplicates and -1 entries are dropped; K is the longest row's)
    assert hip.require_table([7, 8], 2, 10).tolist() == [[7, 8], [7, 8]]                      # one flat list: every image
    assert hip.require_table(np.array([[1, -1], [2, 3]]), 2, 10).tolist() == [[1, -1], [2, 3]]
    assert hip.require_table(torch.tensor([[1, -1], [2, 3]]), 2, 10).tolist() == [[1, -1], [2, 3]]
    for off in (None, [], [[], []], [[-1, -1], [-1]], np.full((2, 3), -1)):
        assert hip.require_table(off, 2, 10) is None
    for bad, word in (([[10]], "0..9"), ([[-2]], "0..9"), ([list(range(9))], "at most 8"), ([[3]], "ban_ids"), ([[1], [2]], "rows")):
        with pytest.raises(hip.BofiHipError, match=word):
            hip.require_table(bad, 1, 10, ban_ids=[9] if word == "at most 8" else [3])
    assert hip.REQUIRE_MAX == 8


def _lib():
    from boficap_amd import hip
    assert os.path.exists(hip.LIB_PATH), "build the library first (python -m boficap_amd.build)"
    return hip, hip.lib()


def test_declarations_agree():
    """The entry point in header, ctypes table, build list and library; BOFI_REQUIRE_MAX; the per-call record and the ABI version as they were: a new symbol, not a field."""
    from boficap_amd import build, hip
    header = open(os.path.join(ROOT, "include", "boficap_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    found = re.findall(r"\bbofi_vocab_require\s*\(([^;{]*?)\)\s*;", code, flags=re.S)
    assert len(found) == 1 and found[0].count(",") + 1 == len(hip.SIGNATURES["bofi_vocab_require"][1]) == 17
    assert int(re.search(r"#define\s+BOFI_REQUIRE_MAX\s+(\d+)", code).group(1)) == hip.REQUIRE_MAX == 8
    assert "record stays 128 bytes" in header and C.sizeof(hip.BofiCallOpts) == 128 and hip.ABI_VERSION == 5
    assert [n for n, _ in hip.BofiCallOpts._fields_][-3:] == ["pick_ban", "pick_no_repeat", "pick_repeat_min_id"]
    assert "force.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "force.hip"))
    assert "launch_vocab_require" in open(os.path.join(build.CSRC, "bofi_kernels.h")).read()
    _, lib = _lib()
    assert hasattr(lib, "bofi_vocab_require") and callable(hip.vocab_require) and callable(hip.require_table) and lib.bofi_abi_version() == 5


def test_entry_point_refuses_bad_arguments_without_a_device():
    """Each returns BOFI_ERR_ARG (1) from the argument check, with a message: the pointers are never read, nothing is launched.  rows = 0 is BOFI_OK."""
    hip, lib = _lib()
    p = C.c_void_p(0x1000)
    good = dict(x=p, ldx=9491, rows=40, V=9491, S=20, ntok=None, ntok_bias=0, words=p, K=4, ban=None, no_repeat=1, min_id=7, seq=p, chosen=None, pos=p, moved=None)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.bofi_vocab_require(a["x"], a["ldx"], a["rows"], a["V"], a["S"], a["ntok"], a["ntok_bias"], a["words"], a["K"], a["ban"], a["no_repeat"], a["min_id"],
                                    a["seq"], a["chosen"], a["pos"], a["moved"], None)
        if rc == 1:
            assert b"vocab_require" in lib.bofi_last_error(), kw
        return rc

    assert call(x=None) == 1 and call(seq=None) == 1 and call(words=None) == 1 and call(pos=None) == 1
    assert call(rows=41) == 1 and call(rows=-20) == 1
    assert call(V=1) == 1 and call(V=0) == 1
    assert call(ldx=9490) == 1
    assert call(S=0, rows=0) == 1 and call(S=65, rows=65) == 1
    assert call(K=0) == 1 and call(K=9) == 1 and b"K in 1..8" in lib.bofi_last_error()
    assert call(no_repeat=2) == 1 and call(no_repeat=-1) == 1
    assert call(min_id=-1) == 1
    assert call(rows=0) == 0 and call(rows=0, S=64, K=8) == 0


class _Cfg:
    tgt_vocab, seq_length = 10, 20


class _Eng:
    """The engine's keyword validation needs no device: the methods are called on a stand-in that carries the configuration alone."""
    cfg, device = _Cfg, "cpu"


def test_engine_keywords_are_validated_on_the_host():
    from boficap_amd import hip
    from boficap_amd.engine import BofiEngine, DecodePipeline
    table = BofiEngine._require_table
    assert table(_Eng, None, 2) is None and table(_Eng, [], 2) is None and table(_Eng, [[-1], [-1, -1]], 2) is None
    assert table(_Eng, [3, 4], 2).tolist() == [[3, 4], [3, 4]]
    for bad, ban, word in (([10], None, "0..9"), ([list(range(9))] * 2, None, "at most 8"), ([3], [3], "ban_ids"), ([[1]], None, "rows")):
        with pytest.raises(hip.BofiHipError, match=word):
            table(_Eng, bad, 2, ban)
    for args, word in (((True, 0, False), "ids_only"), ((False, hip.FLAG_MASK_PREDICT, False), "mask_predict"), ((False, 0, True), "block_trigrams")):
        with pytest.raises(hip.BofiHipError, match=word) as e:
            BofiEngine._require_refusals(*args)
        assert "require_ids" in str(e.value)
    BofiEngine._require_refusals(False, 0, False)

    class _Pipe:
        fused_vocab, refine_method, block_trigrams, root_vocab, ban_ids = False, "feed_back", False, 10, (3,)
    split = DecodePipeline._require_split
    assert split(_Pipe, None) == (None, None) and split(_Pipe, []) == (None, None) and split(_Pipe, [-1]) == (None, None)
    assert split(_Pipe, [4, 5, 4]) == ([4, 5], None)
    flat, per_batch = split(_Pipe, [[[1]], None])
    assert flat is None and list(per_batch) == [[[1]], None]
    for bad, word in (([3], "ban_ids"), ([10], "0..9"), (np.zeros((2, 2), np.int64), "per-batch")):
        with pytest.raises(hip.BofiHipError, match=word):
            split(_Pipe, bad)
    for attr, value, word in (("fused_vocab", True, "fused_vocab"), ("refine_method", "mask_predict", "mask_predict"), ("block_trigrams", True, "block_trigrams")):
        P = type("P", (_Pipe,), {attr: value})
        with pytest.raises(hip.BofiHipError, match=word) as e:
            split(P, [4])
        assert "require_ids" in str(e.value)
        assert split(P, None) == (None, None)                   # off: nothing to refuse


def test_eval_options_resolve_and_refuse():
    from boficap_amd import eval_utils as E
    vocab = {"7": "a", "8": "UNK", "9": "dog", "10": "frisbee", "11": "dog"}
    keys = [0, 1, 2]
    assert E.required_of({}, vocab, keys) is None and E.required_of({"require_words": ""}, vocab, keys) is None
    assert E.required_of({"require_words": {"5": ["dog"]}}, vocab, keys) is None
    assert E.required_of({"require_words": "dog,frisbee,dog"}, vocab, keys) == ([[9, 10]] * 3, [["dog", "frisbee"]] * 3)      # (the lowest id of a word; duplicates dropped)
    ids, words = E.required_of({"require_words": {"1": ["a"], 2: "dog,a"}}, vocab, keys)
    assert ids == [[], [7], [9, 7]] and words == [[], ["a"], ["dog", "a"]]
    with pytest.raises(ValueError, match="'cat'"):
        E.required_of({"require_words": ["dog", "cat"]}, vocab, keys)
    with pytest.raises(ValueError, match="at most 8"):
        E.required_of({"require_words": [str(i) for i in range(9)]}, {str(i): str(i) for i in range(20)}, keys)
    with pytest.raises(ValueError, match="banned"):
        E.required_of({"require_words": ["dog"]}, vocab, keys, ban_ids=[9])
    with pytest.raises(ValueError, match="vocabulary"):
        E.required_of({"require_words": ["dog"]}, None, keys)
    for kw, mode, n, word in (({}, "SAIC", 1, "NAIC"), ({"fused_vocab": True}, "NAIC", 1, "fused_vocab"), ({"refine_method": "mask_predict"}, "NAIC", 1, "mask_predict"),
                              ({}, "NAIC", 5, "sample_n"), ({"block_trigrams": 1}, "NAIC", 1, "block_trigrams")):
        with pytest.raises(ValueError, match=word) as e:
            E.required_of(dict(kw, require_words=["dog"]), vocab, keys, mode, n)
        assert "require_words" in str(e.value)
        assert E.required_of(kw, vocab, keys, mode, n) is None  # off: nothing to refuse
    pos = torch.tensor([[3, -3, -1], [-3, 0, 5]], dtype=torch.int32)
    assert E.required_entry(["dog", "a"], pos[0]) == [["dog", 3], ["a", None]] and E.required_entry([], pos[0]) == []
    rates = E.required_rates([["dog", "a"], ["a", "dog", "frisbee"]], list(pos), 3, 12)
    assert rates == {"required_rate": 3 / 5, "required_moved_rate": 0.25}


@pytest.mark.parametrize("args,word", [(["--require_words", "a", "--inference_mode", "SAIC"], "NAIC"), (["--require_words", "a", "--fused_vocab"], "fused_vocab"),
                                       (["--require_words", "a", "--refine_rounds", "2", "--refine_method", "mask_predict"], "mask_predict"),
                                       (["--require_words", "a", "--sample_n", "3"], "sample_n"), (["--require_words", "a", "--block_trigrams", "1"], "block_trigrams"),
                                       (["--require_words_json", "x.json", "--fused_vocab"], "fused_vocab"),
                                       (["--require_words", "a", "--require_words_json", "x.json"], "give one")])
def test_eval_tool_refuses_required_words_where_they_cannot_apply(args, word):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval.py"), *args, "--synthetic", "8"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 2 and "--require_words" in r.stderr and word in r.stderr, r.stderr[-400:]
