"""block_trigrams on the constrained pick of the NAIC decode, host side (no GPU): the rule RESTATED in numpy (``pick3_np``, on top of test_constrained_pick's
``order_np``) on a hand-worked case, the whole decode restated on the oracle with exact figures on the golden cases -- what tests/test_gpu_trigram_pick.py holds the
kernel and the engine to --, the declarations, and the refusals that need no device.  The reference has the option on its autoregressive path only and as an additive
penalty (AttModel.py:316, 362-388); the blocked SET here is its own, the block is hard (include/boficap_hip.h, bofi_vocab_pick, states the rule)."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import boficap_oracle as O
from conftest import ROOT
from test_constrained_pick import MARGIN, order_np, pick_np, plain_of

NAN, INF = float("nan"), float("inf")


# ----------------------------------------------------------------------------- the rule, restated
def blocked_np(p, s, min_id=7):
    """The ids that are trigram-blocked at position s, given the picks p[0 .. s-1]."""
    if s < 3 or p[s - 2] < min_id or p[s - 1] < min_id:
        return set()
    return {p[j] for j in range(2, s) if p[j - 2] == p[s - 2] and p[j - 1] == p[s - 1] and p[j] >= min_id}


def pick3_np(x, n, ban=(), no_repeat=False, trigrams=True, min_id=7, pad=0, old=None):
    """``pick_np`` with the trigram rule: position s takes the first id of the order that is not banned, not excluded by ``no_repeat`` and not in ``blocked_np``.  Returns
    pick_np's dict plus ``rank`` int64 [B, S]: the 1-based place of each pick in its row's order over the unbanned ids (0 past n)."""
    x = np.asarray(x)
    B, S, _ = x.shape
    ban = sorted({int(i) for i in ban})
    seq = np.full((B, S), pad, np.int64)
    chosen = np.zeros((B, S), np.float32)
    changed = np.zeros(B, np.int32)
    margin = np.full(B, INF)
    rank = np.zeros((B, S), np.int64)
    for b in range(B):
        nb = min(max(int(n[b]), 0), S)
        p = []
        for s in range(nb):
            order = order_np(x[b, s], ban)
            excl = blocked_np(p, s, min_id) if trigrams else set()
            if no_repeat and s > 0 and p[-1] >= min_id:
                excl = excl | {p[-1]}
            elig = [int(i) for i in order if int(i) not in excl]
            pick, nxt = elig[0], elig[1] if len(elig) > 1 else None
            seq[b, s], chosen[b, s] = pick, x[b, s, pick]
            rank[b, s] = 1 + int(np.nonzero(order == pick)[0][0])
            if nxt is not None:
                with np.errstate(invalid="ignore"):
                    m = float(np.float64(x[b, s, pick]) - np.float64(x[b, s, nxt]))
                margin[b] = NAN if (m != m or margin[b] != margin[b]) else min(margin[b], m)
            p.append(pick)
        if old is not None:
            changed[b] = int((seq[b, :nb] != np.asarray(old)[b, :nb]).sum())
    return dict(seq=seq, chosen=chosen, changed=changed, margin=margin, rank=rank)


def repeated_trigrams(seq, n, min_id=7):
    """Positions s >= 2 whose word trigram (seq[s-2], seq[s-1], seq[s]), all ids >= min_id, stood earlier in the same caption."""
    count = 0
    for b in range(len(n)):
        seen = set()
        for s in range(2, int(n[b])):
            t = tuple(int(v) for v in seq[b, s - 2:s + 1])
            if min(t) >= min_id:
                count += t in seen
                seen.add(t)
    return count


def adjacent_repeats(seq, n, min_id=7):
    return sum(int(seq[b, s] == seq[b, s - 1] and seq[b, s] >= min_id) for b in range(len(n)) for s in range(1, int(n[b])))


# ----------------------------------------------------------------------------- the whole decode, restated on the oracle
@functools.lru_cache(maxsize=None)
def restate3(name, no_repeat):
    """The decode of golden case ``name`` with block_trigrams (and ``no_repeat``), T = 0 and T = 1 feed-back rounds (the constrained ids fed back), computed once and
    shared: a list indexed by T of dicts with ``seq``, ``chosen``, ``rank``, ``lp`` (the last pass's log-probs), ``changed`` (against that pass's own plain argmax),
    ``two`` (the pick of the same tensor WITHOUT the trigram rule), ``safe`` [B] (every decision of every pass so far has a margin above MARGIN) and ``min_margin``."""
    base = plain_of(name)
    cfg, n = base["cfg"], base["n"]
    out, ids, lp = [], None, base["lp"]
    safe = np.ones(len(n), bool)
    worst = INF
    for T in (0, 1):
        if T:
            with torch.no_grad():
                ph = O.decode_na(base["w"], cfg, base["memory"], base["ext"], base["src_mask"], base["syn_mask"], glat_input=torch.from_numpy(ids))
                lp = F.log_softmax(O.logit(base["w"], ph), dim=2).numpy()
        argmax = pick_np(lp, n, pad=cfg.pad_idx)["seq"]
        p = pick3_np(lp, n, (), no_repeat, True, 7, cfg.pad_idx, old=argmax)
        safe = safe & (p["margin"] > MARGIN)
        worst = min(worst, float(np.nanmin(p["margin"])))
        ids = p["seq"]
        out.append(dict(seq=ids, chosen=p["chosen"], rank=p["rank"], lp=lp, changed=p["changed"], two=pick_np(lp, n, (), no_repeat, 7, cfg.pad_idx)["seq"], safe=safe.copy(),
                        min_margin=worst, plain=argmax))
    return out


# (case, no_repeat, T) -> (repeated trigrams without the rule, positions the rule changes, safe images, images)
FIGURES = {("full_b8", False, 0): (47, 19, 8, 8), ("full_b8", False, 1): (48, 19, 8, 8), ("full_b8", True, 0): (35, 33, 8, 8), ("full_b8", True, 1): (36, 33, 6, 8),
           ("tiny_saic_multi", False, 0): (70, 30, 6, 6), ("tiny_saic_multi", False, 1): (47, 22, 6, 6), ("tiny_saic_multi", True, 0): (43, 48, 6, 6),
           ("tiny_saic_multi", True, 1): (22, 38, 6, 6)}


# ----------------------------------------------------------------------------- tests
def _hand_case():
    """x [5, 8, 12] of the hand-worked case and its live counts."""
    S, V = 8, 12
    x = np.full((5, S, V), -5.0, np.float32)
    for b in (0, 1, 4):                                         # 9 leads, then 8, then 10
        x[b, :, 9], x[b, :, 8], x[b, :, 10] = -0.1, -0.2, -0.3
    x[0, 6, :] = -5.0
    x[0, 6, 9], x[0, 6, 8], x[0, 6, 10] = NAN, NAN, -0.3         # a NaN row: 8, 9 (the NaNs, by id), then 10
    x[0, 7, :] = -INF                                           # an all -inf row: the ids in their own order
    x[1, 6, :] = -INF
    x[2, 0::2, 9], x[2, 0::2, 8] = -0.1, -0.2                   # even rows: 9, then 8; odd rows: 3 (not a word), then 10
    x[2, 1::2, 3], x[2, 1::2, 10] = -0.1, -0.2
    x[3] = NAN                                                  # n = 0: never read
    return x, [8, 8, 8, 0, 3]


def test_pick3_np_on_a_hand_worked_case():
    """S = 8, V = 12, min_id 7; worked by hand.  Rows of images 0, 1 and 4 prefer 9, then 8, then 10 (a = 9, b = 8, c = 10).

    Image 0, trigrams alone: a a a, then position 3 has the bigram (a, a) behind it, which a followed at j = 2: a is blocked -> b.  Position 4: (a, b) is new -> a; position 5:
    (b, a) is new -> a.  Position 6: (a, a) was followed by a (j = 2) and by b (j = 3): both blocked, and its row is the NaN row whose order is 8, 9 (NaN, by id), 10 -> c.
    Position 7, all -inf: nothing follows (a, c) yet -> id 0.        9 9 9 8 9 9 10 0
    Image 0, no_repeat too: 9; 8 (9 barred); 9; 8 ((8, 9) new, 9 barred); position 4: (9, 8) was followed by 9 -> blocked, 8 is barred -> 10; 9; the NaN row with 9 barred and
    nothing blocked -> 8; 0.                                          9 8 9 8 10 9 8 0
    Image 1 under a ban of ids 0..7 (row 6 all -inf: its unbanned order is 8, 9, 10, 11; 8 and 9 are blocked -> 10); position 7: (9, 10) is new -> 9.   9 9 9 8 9 9 10 9
    Image 2: 9 3 9 3 ...: every trigram holds id 3 < 7 -- nothing is ever blocked.  With min_id 0 it is: position 4 (9, 3) -> 9 blocked -> 8; position 5 (3, 8) new -> 3; position 6
    (8, 3) new -> 9; position 7 (3, 9) was followed by 3 -> 10.      9 3 9 3 8 3 9 10
    Image 3: n = 0.  Image 4: n = 3: 9 9 9, nothing blockable, then pad."""
    x, n = _hand_case()
    r = pick3_np(x, n, pad=1)
    assert r["seq"][0].tolist() == [9, 9, 9, 8, 9, 9, 10, 0]
    assert r["rank"][0].tolist() == [1, 1, 1, 2, 1, 1, 3, 1]
    assert r["chosen"][0, [3, 6, 7]].tolist() == [np.float32(-0.2), np.float32(-0.3), -INF]
    assert r["seq"][2].tolist() == [9, 3, 9, 3, 9, 3, 9, 3]
    assert r["seq"][3].tolist() == [1] * 8 and r["seq"][4].tolist() == [9, 9, 9, 1, 1, 1, 1, 1] and r["margin"][3] == INF
    assert np.isnan(r["margin"][0]) and abs(r["margin"][4] - 0.1) < 1e-6
    both = pick3_np(x, n, no_repeat=True, pad=1, old=np.full((5, 8), 9))
    assert both["seq"][0].tolist() == [9, 8, 9, 8, 10, 9, 8, 0]
    assert both["seq"][4].tolist() == [9, 8, 9, 1, 1, 1, 1, 1] and both["changed"].tolist() == [5, 4, 4, 0, 1]      # (image 1: 9 8 9 8 10 9 0 9)
    assert both["seq"][2].tolist() == [9, 3, 9, 3, 9, 3, 9, 3]
    banned = pick3_np(x, n, ban=range(8))
    assert banned["seq"][1].tolist() == [9, 9, 9, 8, 9, 9, 10, 9] and banned["seq"][0].tolist() == [9, 9, 9, 8, 9, 9, 10, 8]
    assert banned["rank"][1, 6] == 3                            # (the place among the UNBANNED ids)
    assert pick3_np(x, n, min_id=0)["seq"][2].tolist() == [9, 3, 9, 3, 8, 3, 9, 10]
    # the blocked set on its own: from s = 3, j from 2, words only
    assert blocked_np([9, 9, 9], 3) == {9} and blocked_np([9, 9], 2) == set() and blocked_np([9, 9, 9, 8, 9, 9], 6) == {9, 8}
    assert blocked_np([9, 3, 9, 3], 4) == set() and blocked_np([9, 3, 9, 3], 4, min_id=0) == {9} and blocked_np([8, 9, 3, 8, 9], 5) == set()
    # the rule off is pick_np, and no emitted caption repeats a trigram
    for rep in (False, True):
        off, want = pick3_np(x, n, ban=[8], no_repeat=rep, trigrams=False, pad=1), pick_np(x, n, ban=[8], no_repeat=rep, pad=1)
        assert np.array_equal(off["seq"], want["seq"]) and np.array_equal(off["chosen"].view(np.int32), want["chosen"].view(np.int32))
    assert repeated_trigrams(r["seq"], n) == 0 and repeated_trigrams(pick_np(x, n)["seq"], n) == 3 + 3      # (9 9 9 9 9 9 8 0 and 9 9 9 9 9 9 0 9)
    assert adjacent_repeats(both["seq"], n) == 0


@pytest.mark.parametrize("name", ["tiny_saic_multi", "full_b8"])
def test_restated_decode_figures(name):
    """Exact figures of the restated decode: without the rule the T = 0 decode under no_repeat still repeats 35 (full_b8, 78 live positions) / 43 (tiny_saic_multi, 112) word
    trigrams, with it none, and 33 / 48 positions change; the emitted id reaches the 5th best of its row in both cases (the 7th on full_b8 with trigrams alone) -- two
    candidates per row do not serve this decode.  With MARGIN = 1e-3 every image is safe in seven of the eight (case, no_repeat, T) combinations; full_b8, no_repeat, T = 1
    has 6 of 8 (smallest margin 1.5e-4)."""
    base = plain_of(name)
    n, pad = base["n"], base["cfg"].pad_idx
    assert int(n.sum()) == {"full_b8": 78, "tiny_saic_multi": 112}[name]
    for rep in (False, True):
        for T, r in enumerate(restate3(name, rep)):
            before, moved, safe, images = FIGURES[(name, rep, T)]
            print(f"{name} no_repeat={rep} T={T}: repeated trigrams {repeated_trigrams(r['two'], n)} -> {repeated_trigrams(r['seq'], n)}, {int((r['seq'] != r['two']).sum())} positions "
                  f"change, deepest pick {int(r['rank'].max())}, safe {int(r['safe'].sum())} of {len(n)}, min margin {r['min_margin']:.6f}")
            assert repeated_trigrams(r["two"], n) == before and repeated_trigrams(r["seq"], n) == 0
            assert int((r["seq"] != r["two"]).sum()) == moved
            assert (int(r["safe"].sum()), len(n)) == (safe, images)
            if rep:
                assert adjacent_repeats(r["seq"], n) == 0
            for b in range(len(n)):
                assert (r["seq"][b, n[b]:] == pad).all()
            if T == 0:
                assert np.array_equal(r["plain"], base["seq"])
    assert int(restate3(name, True)[0]["rank"].max()) == 5
    if name == "full_b8":
        assert int(restate3(name, False)[0]["rank"].max()) == 7
        assert 1.4e-4 < restate3(name, True)[1]["min_margin"] < 1.6e-4


def _lib():
    from boficap_amd import hip
    assert os.path.exists(hip.LIB_PATH), "build the library first (python -m boficap_amd.build)"
    return hip, hip.lib()


def test_declarations_agree():
    """The K form's entry point and its size query in header, ctypes table and library; the flag's value in header and hip.py, a bit no other flag uses; the per-call record
    and the ABI version as they were."""
    from boficap_amd import hip
    header = open(os.path.join(ROOT, "include", "boficap_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, arity in (("bofi_vocab_pick", 18), ("bofi_vocab_pick_workspace", 1), ("bofi_vocab_constrain", 15)):
        found = re.findall(r"\b" + name + r"\s*\(([^;{]*?)\)\s*;", code, flags=re.S)
        assert len(found) == 1 and found[0].count(",") + 1 == len(hip.SIGNATURES[name][1]) == arity, name
    flags = {k: int(v) for k, v in re.findall(r"#define\s+(BOFI_FLAG_\w+)\s+(\d+)", code)}
    assert flags["BOFI_FLAG_PICK_TRIGRAMS"] == hip.FLAG_PICK_TRIGRAMS == 32768
    others = [v for k, v in flags.items() if k not in ("BOFI_FLAG_PICK_TRIGRAMS", "BOFI_FLAG_REFINE_SHIFT")]
    assert all(v & 32768 == 0 for v in others) and (15 << flags["BOFI_FLAG_REFINE_SHIFT"]) & 32768 == 0
    assert hip.ABI_VERSION == 5 and C.sizeof(hip.BofiCallOpts) == 128
    assert [n for n, _ in hip.BofiCallOpts._fields_][-3:] == ["pick_ban", "pick_no_repeat", "pick_repeat_min_id"]
    _, lib = _lib()
    assert hasattr(lib, "bofi_vocab_pick") and callable(hip.vocab_pick) and lib.bofi_abi_version() == 5
    sizes = [lib.bofi_vocab_pick_workspace(r) for r in (0, 1, 40, 1280)]
    assert sizes[0] == 0 and sizes[1] in (16, 32) and sizes[2] == 40 * sizes[1] and sizes[3] == 1280 * sizes[1]      # int32 [rows, K], K = 4 or 8


def test_entry_point_refuses_bad_arguments_without_a_device():
    """Each returns BOFI_ERR_ARG (1) from the argument check, with a message: the pointers are never read, nothing is launched.  rows = 0 is BOFI_OK."""
    hip, lib = _lib()
    p = C.c_void_p(0x1000)
    need = lib.bofi_vocab_pick_workspace(40)
    good = dict(x=p, ldx=9491, rows=40, V=9491, S=20, ntok=None, ntok_bias=0, pad_idx=0, ban=None, no_repeat=1, tri=1, min_id=7, seq=p, chosen=None, changed=None, work=p,
                work_bytes=need)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.bofi_vocab_pick(a["x"], a["ldx"], a["rows"], a["V"], a["S"], a["ntok"], a["ntok_bias"], a["pad_idx"], a["ban"], a["no_repeat"], a["tri"], a["min_id"], a["seq"],
                                 a["chosen"], a["changed"], a["work"], a["work_bytes"], None)
        if rc == 1:
            assert b"vocab_pick" in lib.bofi_last_error(), kw
        return rc

    assert call(x=None) == 1 and call(seq=None) == 1
    assert call(rows=41) == 1 and call(rows=-20) == 1
    assert call(V=1) == 1 and call(V=0) == 1
    assert call(ldx=9490) == 1
    assert call(S=0, rows=0) == 1 and call(S=65, rows=65) == 1
    assert call(no_repeat=2) == 1 and call(no_repeat=-1) == 1
    assert call(min_id=-1) == 1
    assert call(tri=2) == 1 and call(tri=-1) == 1 and b"block_trigrams" in lib.bofi_last_error()
    assert call(work=None) == 1 and b"workspace" in lib.bofi_last_error()
    assert call(work_bytes=need - 1) == 1 and call(work_bytes=0) == 1 and call(work_bytes=-8) == 1
    assert call(rows=0) == 0 and call(rows=0, work=None, work_bytes=0) == 0


def test_eval_options_resolve_and_refuse():
    from boficap_amd import eval_utils
    vocab = {"7": "a", "8": "UNK", "9": "dog", "10": "UNK"}
    assert eval_utils.constraint_of({"block_trigrams": 0}, vocab) == {}
    assert eval_utils.constraint_of({"block_trigrams": 1}, vocab) == {"ban_ids": [], "no_repeat": False, "block_trigrams": True}
    assert eval_utils.constraint_of({"block_trigrams": 1}, None) == {"ban_ids": [], "no_repeat": False, "block_trigrams": True}      # (no word to resolve: no vocabulary needed)
    assert eval_utils.constraint_of({"suppress_UNK": 1, "decoding_constraint": 1, "block_trigrams": 1}, vocab) == {"ban_ids": [8, 10], "no_repeat": True, "block_trigrams": True}
    assert eval_utils.constraint_of({"suppress_UNK": 1}, vocab) == {"ban_ids": [8, 10], "no_repeat": False}              # off: the keywords as they were
    for kw, mode, n, word in (({"block_trigrams": 1}, "SAIC", 1, "NAIC"), ({"block_trigrams": 1, "fused_vocab": True}, "NAIC", 1, "fused_vocab"),
                              ({"block_trigrams": 1, "refine_method": "mask_predict"}, "NAIC", 1, "mask_predict"), ({"block_trigrams": 1}, "NAIC", 5, "sample_n")):
        with pytest.raises(ValueError, match=word) as e:
            eval_utils.constraint_of(kw, vocab, mode, n)
        assert "block_trigrams" in str(e.value)


@pytest.mark.parametrize("args,word", [(["--block_trigrams", "1", "--inference_mode", "SAIC"], "NAIC"), (["--block_trigrams", "1", "--fused_vocab"], "fused_vocab"),
                                       (["--block_trigrams", "1", "--refine_rounds", "2", "--refine_method", "mask_predict"], "mask_predict"),
                                       (["--block_trigrams", "1", "--sample_n", "3"], "sample_n")])
def test_eval_tool_refuses_block_trigrams_where_it_cannot_apply(args, word):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval.py"), *args, "--synthetic", "8"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 2 and "--block_trigrams" in r.stderr and word in r.stderr, r.stderr[-400:]
