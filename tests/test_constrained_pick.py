"""The constrained pick of the NAIC decode (banned ids, no adjacent repeated word), host side (no GPU): the declarations agree, the rule RESTATED in numpy
(``pick_np``) on a hand-worked case, the whole decode restated on the oracle's memory_of / core_naic / decode_na / logit -- what tests/test_gpu_constrained_pick.py
holds the kernel and the engine to --, and the refusals that need no device.  The reference applies its suppress_UNK / decoding_constraint on its autoregressive
paths only, so this module is where the rule is pinned (include/boficap_hip.h, bofi_vocab_constrain, states it in words)."""
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
from test_mask_predict import _case, _fill_mask

NAN, INF = float("nan"), float("inf")
VARIANTS = {"ban": (True, False), "no_repeat": (False, True), "both": (True, True)}       # name -> (ban the plain decode's most frequent id, no_repeat)
MARGIN = 1e-3


# ----------------------------------------------------------------------------- the rule, restated
def order_np(row, ban=()):
    """The unbanned ids of ``row`` in the pick order: NaN before every number, then by value descending (float64 comparisons), ties -- +0.0 against -0.0, NaN
    against NaN -- by lower id."""
    r = np.asarray(row, np.float64)
    nan = np.isnan(r)
    order = np.lexsort((np.arange(len(r)), -np.where(nan, 0.0, r), ~nan))      # NaNs, then values; (-(+0.0) and -(-0.0) compare equal: the id decides)
    if len(ban):
        order = order[~np.isin(order, np.fromiter(ban, np.int64, len(ban)))]
    return order


def pick_np(x, n, ban=(), no_repeat=False, min_id=7, pad=0, old=None):
    """The constrained pick of x [B, S, >= V] (its first V = x.shape[2] columns are the vocabulary) with n [B] live positions (clamped to 0 .. S): a dict of
    ``seq`` int64 [B, S] (the pick, then ``pad``), ``chosen`` float32 [B, S] (x at the pick; NaN-free zeros past n: the kernel leaves those untouched), ``changed``
    int32 [B] against ``old`` [B, S] (when given) and ``margin`` float64 [B]: the smallest x[pick] - x[next eligible id] over the image's decisions (inf for n = 0;
    NaN when a NaN was involved)."""
    x = np.asarray(x)
    B, S, _ = x.shape
    ban = sorted({int(i) for i in ban})
    seq = np.full((B, S), pad, np.int64)
    chosen = np.zeros((B, S), np.float32)
    changed = np.zeros(B, np.int32)
    margin = np.full(B, INF)
    for b in range(B):
        nb = min(max(int(n[b]), 0), S)
        prev = -1
        for s in range(nb):
            order = order_np(x[b, s], ban)
            if no_repeat and s > 0 and prev >= min_id:
                order = order[order != prev]
            pick, nxt = int(order[0]), int(order[1]) if len(order) > 1 else None
            seq[b, s], chosen[b, s] = pick, x[b, s, pick]
            if nxt is not None:
                with np.errstate(invalid="ignore"):
                    m = float(np.float64(x[b, s, pick]) - np.float64(x[b, s, nxt]))
                margin[b] = NAN if (m != m or margin[b] != margin[b]) else min(margin[b], m)
            prev = pick
        if old is not None:
            changed[b] = int((seq[b, :nb] != np.asarray(old)[b, :nb]).sum())
    return dict(seq=seq, chosen=chosen, changed=changed, margin=margin)


# ----------------------------------------------------------------------------- the whole decode, restated on the oracle
def _adjacent_repeats(seq, n, min_id=7):
    return sum(int(seq[b, s] == seq[b, s - 1] and seq[b, s] >= min_id) for b in range(len(n)) for s in range(1, int(n[b])))


@functools.lru_cache(maxsize=None)
def plain_of(name):
    """The plain decode of a golden case at T = 0 (strict Q1): layout, live counts, ids and the id it emits most often."""
    cfg, sd, att, masks = _case(name)
    w = O.as_torch(sd)
    with torch.no_grad():
        memory, src_mask = O.memory_of(w, cfg, att, masks)
        _, pn, pl, ps, dg = O.core_naic(w, cfg, memory, src_mask)
        B, S = memory.size(0), cfg.seq_length
        last = dg["last"].numpy()
        syn_mask = _fill_mask(cfg, last, B, False)
        lp = F.log_softmax(O.logit(w, O.decode_na(w, cfg, memory, dg["ext_syn"][:, 1:-1], src_mask, syn_mask, glat_input=None)), dim=2).numpy()
    n = np.clip(last - 1, 0, S)
    p = pick_np(lp, n, pad=cfg.pad_idx)
    live = np.concatenate([p["seq"][b, :n[b]] for b in range(B)])
    ids, counts = np.unique(live, return_counts=True)
    return dict(cfg=cfg, sd=sd, att=att, masks=masks, w=w, memory=memory, src_mask=src_mask, syn_mask=syn_mask, ext=dg["ext_syn"][:, 1:-1], phrase_num=pn, phrase_length=pl,
                phrase_syn=ps, last=last, n=n, lp=lp, seq=p["seq"], top_id=int(ids[np.argmax(counts)]), top_count=int(counts.max()))


@functools.lru_cache(maxsize=None)
def restate(name, variant):
    """The constrained decode of golden case ``name`` with T = 0 and T = 1 feed-back rounds (the constrained ids fed back), computed once and shared: a list indexed by T
    of dicts with ``seq``, ``chosen``, ``lp`` (the last pass's log-probs), ``changed`` (the last pass's counts against that pass's own plain argmax), ``safe`` [B] (every
    decision of every pass so far has a margin above MARGIN) and ``min_margin``."""
    base = plain_of(name)
    cfg, n = base["cfg"], base["n"]
    ban = (base["top_id"],) if VARIANTS[variant][0] else ()
    rep = VARIANTS[variant][1]
    out, ids, lp = [], None, base["lp"]
    safe = np.ones(len(n), bool)
    worst = INF
    for T in (0, 1):
        if T:
            with torch.no_grad():
                ph = O.decode_na(base["w"], cfg, base["memory"], base["ext"], base["src_mask"], base["syn_mask"], glat_input=torch.from_numpy(ids))
                lp = F.log_softmax(O.logit(base["w"], ph), dim=2).numpy()
        argmax = pick_np(lp, n, pad=cfg.pad_idx)["seq"]
        p = pick_np(lp, n, ban, rep, 7, cfg.pad_idx, old=argmax)
        safe = safe & (p["margin"] > MARGIN)
        worst = min(worst, float(np.nanmin(p["margin"])))
        ids = p["seq"]
        out.append(dict(seq=ids, chosen=p["chosen"], lp=lp, changed=p["changed"], safe=safe.copy(), min_margin=worst, plain=argmax, ban=ban, no_repeat=rep))
    return out


# ----------------------------------------------------------------------------- tests
def _lib():
    from boficap_amd import hip
    assert os.path.exists(hip.LIB_PATH), "build the library first (python -m boficap_amd.build)"
    return hip, hip.lib()


def test_declarations_agree():
    """The kernel's entry point, the counts' entry point and the per-call record's three new fields: header, ctypes table, build list, ABI version."""
    from boficap_amd import build, hip
    header = open(os.path.join(ROOT, "include", "boficap_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, arity in (("bofi_vocab_constrain", 15), ("bofi_engine_pick_changed", 4)):
        found = re.findall(r"\b" + name + r"\s*\(([^;{]*?)\)\s*;", code, flags=re.S)
        assert len(found) == 1 and found[0].count(",") + 1 == len(hip.SIGNATURES[name][1]) == arity, name
    body = re.search(r"typedef\s+struct\s+bofi_call_opts\s*\{(.*?)\}\s*bofi_call_opts_t\s*;", code, flags=re.S).group(1)
    fields = re.findall(r"(\w+)\s*;", body)
    assert fields == [n for n, _ in hip.BofiCallOpts._fields_]
    assert fields[-3:] == ["pick_ban", "pick_no_repeat", "pick_repeat_min_id"]           # appended at the record's end: a zero tail is today's decode
    pinned = re.findall(r"static_assert\(sizeof\(bofi_call_opts_t\) == (\d+)", open(os.path.join(build.CSRC, "engine.hip")).read())
    assert len(pinned) == 1 and C.sizeof(hip.BofiCallOpts) == int(pinned[0]) == 128
    o = hip.BofiCallOpts()
    assert (o.pick_ban, o.pick_no_repeat, o.pick_repeat_min_id) == (None, 0, 0)
    assert "constrain.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "constrain.hip"))
    assert "launch_vocab_constrain" in open(os.path.join(build.CSRC, "bofi_kernels.h")).read()
    assert hip.ABI_VERSION == 5
    _, lib = _lib()
    assert hasattr(lib, "bofi_vocab_constrain") and callable(hip.vocab_constrain) and lib.bofi_abi_version() == 5


def test_pick_np_on_a_hand_worked_case():
    """S = 6, V = 12, min_id 7; worked by hand.  Image 0 (n = S): a tie to the lower id, +0.0 against -0.0, one NaN, two NaNs, an all -inf row, and a pad-free
    full row.  Image 1 (n = 4, pad tail): the chain a a a -> a b a, and a prev below min_id that repeats.  Image 2: n = 0; image 3: n = 1."""
    S, V = 6, 12
    x = np.full((4, S, V), -5.0, np.float32)
    x[0, 0, [9, 8]] = -1.0                                      # tie: 8 (the lower id)
    x[0, 1, 10], x[0, 1, 7] = -0.0, 0.0                         # +0.0 == -0.0: 7
    x[0, 2, 11], x[0, 2, 3] = 3.0, NAN                          # a NaN beats every number: 3
    x[0, 3, 9], x[0, 3, 4] = NAN, NAN                           # two NaNs: the lower id, 4
    x[0, 4, :] = -INF                                           # all -inf: id 0
    x[0, 5, 8], x[0, 5, 9] = -0.5, -0.25                        # 9
    z = np.array([[[1.0, INF, NAN, INF]]], np.float32)          # a NaN comes before +inf too
    assert order_np(z[0, 0]).tolist() == [2, 1, 3, 0] and pick_np(z, [1], ban=[2])["seq"][0].tolist() == [1]
    plain = pick_np(x[:1], [S])
    assert plain["seq"][0].tolist() == [8, 7, 3, 4, 0, 9]
    assert plain["chosen"][0, [0, 1, 4, 5]].tolist() == [-1.0, 0.0, -INF, -0.25] and np.isnan(plain["chosen"][0, 2:4]).all()
    assert np.isnan(plain["margin"][0])                         # (a NaN took part)
    # the banned best id, and the banned best two
    assert pick_np(x[:1], [S], ban=[8])["seq"][0].tolist() == [9, 7, 3, 4, 0, 9]
    b2 = pick_np(x[:1], [S], ban=[8, 9, 0])
    assert b2["seq"][0].tolist() == [1, 7, 3, 4, 1, 1] and b2["chosen"][0, 0] == -5.0 and b2["chosen"][0, 4] == -INF      # (what is left ties at -5 / -inf: id 1, as 0 is banned)
    # a a a -> a b a; positions 2, 3: prev = 2 < min_id may repeat
    x[1, 0, 9], x[1, 0, 8] = -0.1, -0.2
    x[1, 1, 9], x[1, 1, 8] = -0.1, -0.3
    x[1, 2, 9], x[1, 2, 10] = -0.1, -0.4
    x[1, 3, 9], x[1, 3, 10] = -0.1, -0.6
    x[1, 4, 9] = -0.1                                           # past n: not read
    chain = pick_np(x[1:2], [4], no_repeat=True, pad=0)
    assert chain["seq"][0].tolist() == [9, 8, 9, 10, 0, 0]      # 9; 8 (9 is barred); 9 again; 9 is barred: the best other id, 10
    y = np.full((1, S, V), -5.0, np.float32)
    y[0, :, 2] = -0.1                                           # id 2 < min_id everywhere
    y[0, :, 9] = -0.2
    low = pick_np(y, [4], no_repeat=True)
    assert low["seq"][0].tolist() == [2, 2, 2, 2, 0, 0] and abs(low["margin"][0] - 0.1) < 1e-6
    assert pick_np(y, [4], no_repeat=True, min_id=0)["seq"][0].tolist() == [2, 9, 2, 9, 0, 0]
    # n = 0, n = 1, n = S, clamping, the counts and the pad tail
    r = pick_np(x, [S, 4, 0, 1], ban=[8], no_repeat=True, pad=5, old=np.full((4, S), 9))
    assert r["seq"][2].tolist() == [5] * S and r["seq"][3].tolist() == [0] + [5] * (S - 1) and r["seq"][1, 4:].tolist() == [5, 5]
    assert r["seq"][0].tolist() == [9, 7, 3, 4, 0, 9] and r["seq"][1, :4].tolist() == [9, 0, 9, 10]      # (image 1, position 1: 9 barred, 8 banned, the rest ties: id 0)
    assert r["changed"].tolist() == [4, 2, 0, 1] and r["margin"][2] == INF
    assert pick_np(x, [99, -3, 0, 1])["seq"][1].tolist() == [0] * S
    assert (r["chosen"][2] == 0).all() and (r["chosen"][1, 4:] == 0).all()


def test_pick_np_chain_detail():
    """The chain of the hand-worked case once more with every candidate spelled out: a = 9 leads at all four positions; b differs per position."""
    V = 12
    x = np.full((1, 4, V), -9.0, np.float32)
    x[0, :, 9] = -0.1
    x[0, 0, 8], x[0, 1, 8], x[0, 2, 10], x[0, 3, 11] = -0.2, -0.3, -0.4, -0.5
    assert pick_np(x, [4])["seq"][0].tolist() == [9, 9, 9, 9]
    c = pick_np(x, [4], no_repeat=True, old=np.full((1, 4), 9))
    assert c["seq"][0].tolist() == [9, 8, 9, 11] and c["changed"].tolist() == [2]
    assert c["chosen"][0].tolist() == [np.float32(-0.1), np.float32(-0.3), np.float32(-0.1), np.float32(-0.5)]
    assert abs(c["margin"][0] - 0.1) < 1e-6                     # position 0: a against b, 0.1


@pytest.mark.parametrize("name", ["tiny_saic_multi", "full_b8"])
def test_restated_decode_is_not_vacuous_and_safe(name):
    """The plain decode repeats adjacent words and emits the banned id; under 'both' at least a third of the live positions change and no adjacent repeat of a word
    remains; every image is safe at T = 0 in all three variants and at most one image per case is unsafe at T = 1.
    Measured: 59 of 78 positions change on full_b8 and 83 of 112 on tiny_saic_multi; the smallest T = 0 margin is 0.0020."""
    base = plain_of(name)
    n, live = base["n"], int(base["n"].sum())
    assert _adjacent_repeats(base["seq"], n) >= 1
    assert base["top_count"] >= 1
    for variant, (ban_on, rep_on) in VARIANTS.items():
        for T, r in enumerate(restate(name, variant)):
            seq = r["seq"]
            for b in range(len(n)):
                assert (seq[b, n[b]:] == base["cfg"].pad_idx).all()
                if ban_on:
                    assert base["top_id"] not in seq[b, :n[b]].tolist()
            if rep_on:
                assert _adjacent_repeats(seq, n) == 0
            print(f"{name} {variant} T={T}: {int(r['changed'].sum())} of {live} positions changed, min margin {r['min_margin']:.5f}, unsafe images {int((~r['safe']).sum())}")
            if T == 0:
                assert r["safe"].all(), (variant, r["min_margin"])
                assert np.array_equal(r["plain"], base["seq"])
            else:
                assert int((~r["safe"]).sum()) <= 1, (variant, r["min_margin"])
    unsafe = np.zeros(len(n), bool)
    for variant in VARIANTS:
        unsafe |= ~restate(name, variant)[1]["safe"]
    assert int(unsafe.sum()) <= 1                               # ... and it is the same image in every variant
    both = restate(name, "both")[0]
    assert 3 * int(both["changed"].sum()) >= live
    assert int((both["seq"] != base["seq"]).sum()) == int(both["changed"].sum())


def test_entry_point_refuses_bad_arguments_without_a_device():
    """Each returns BOFI_ERR_ARG (1) from the argument check, with a message: the pointers are never read, nothing is launched.  rows = 0 is BOFI_OK."""
    hip, lib = _lib()
    p = C.c_void_p(0x1000)
    good = dict(x=p, ldx=9491, rows=40, V=9491, S=20, ntok=None, ntok_bias=0, pad_idx=0, ban=None, no_repeat=1, min_id=7, seq=p, chosen=None, changed=None)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.bofi_vocab_constrain(a["x"], a["ldx"], a["rows"], a["V"], a["S"], a["ntok"], a["ntok_bias"], a["pad_idx"], a["ban"], a["no_repeat"], a["min_id"], a["seq"],
                                      a["chosen"], a["changed"], None)
        if rc == 1:
            assert b"vocab_constrain" in lib.bofi_last_error(), kw
        return rc

    assert call(x=None) == 1 and call(seq=None) == 1
    assert call(rows=41) == 1 and call(rows=-20) == 1
    assert call(V=1) == 1 and call(V=0) == 1
    assert call(ldx=9490) == 1
    assert call(S=0, rows=0) == 1 and call(S=65, rows=65) == 1
    assert call(no_repeat=2) == 1 and call(no_repeat=-1) == 1
    assert call(min_id=-1) == 1
    assert call(rows=0) == 0
    assert lib.bofi_engine_pick_changed(None, p, 1, None) == 1


def test_ban_list_is_checked_on_the_host():
    from boficap_amd import hip
    t = hip.ban_bits([0, 31, 32, 256], 257)
    assert t.dtype == torch.int32 and t.numel() == 9
    w = t.numpy().view(np.uint32)
    assert w[0] == (1 | (1 << 31)) and w[1] == 1 and w[8] == 1 and not w[2:8].any()
    assert hip.ban_bits([], 64).numpy().any() == False          # noqa: E712  (the empty list: no bit)
    for bad in ([-1], [257], [3, 9999]):
        with pytest.raises(hip.BofiHipError, match="0..256"):
            hip.ban_bits(bad, 257)
    with pytest.raises(hip.BofiHipError, match="at least two"):
        hip.ban_bits(range(1, 10), 10)
    assert hip.ban_bits(range(2, 10), 10).numel() == 1          # two ids stay: allowed


def test_eval_options_resolve_and_refuse():
    from boficap_amd import eval_utils
    vocab = {"7": "a", "8": "UNK", "9": "dog", "10": "UNK"}
    assert eval_utils.constraint_of({}, vocab) == {}
    assert eval_utils.constraint_of({"suppress_UNK": 1}, vocab) == {"ban_ids": [8, 10], "no_repeat": False}
    assert eval_utils.constraint_of({"ban_words": "dog,cat", "decoding_constraint": 1}, vocab) == {"ban_ids": [9], "no_repeat": True}
    assert eval_utils.constraint_of({"suppress_UNK": 1}, {"7": "a"}) == {}              # no UNK in the vocabulary: nothing banned, nothing launched
    assert eval_utils.constraint_of({"suppress_UNK": 0, "decoding_constraint": 0, "ban_words": ""}, vocab, "SAIC", 5) == {}
    for kw, mode, n, word in (({"suppress_UNK": 1}, "SAIC", 1, "NAIC"), ({"decoding_constraint": 1, "fused_vocab": True}, "NAIC", 1, "fused_vocab"),
                              ({"ban_words": ["dog"], "refine_method": "mask_predict"}, "NAIC", 1, "mask_predict"), ({"decoding_constraint": 1}, "NAIC", 5, "sample_n")):
        with pytest.raises(ValueError, match=word):
            eval_utils.constraint_of(kw, vocab, mode, n)


@pytest.mark.parametrize("args,word", [(["--suppress_UNK", "1", "--inference_mode", "SAIC"], "NAIC"), (["--decoding_constraint", "1", "--fused_vocab"], "fused_vocab"),
                                       (["--ban_words", "a,b", "--refine_rounds", "2", "--refine_method", "mask_predict"], "mask_predict"),
                                       (["--decoding_constraint", "1", "--sample_n", "3"], "sample_n")])
def test_eval_tool_refuses_constraints_where_they_cannot_apply(args, word):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval.py"), *args, "--synthetic", "8"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 2 and "--decoding_constraint" in r.stderr and word in r.stderr, r.stderr[-400:]
