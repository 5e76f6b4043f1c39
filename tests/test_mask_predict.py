"""Mask-predict refinement of the filling pass, host side (no GPU): the declarations agree, and the RESTATEMENT of the rules -- the step between two
passes in numpy, and the whole decode on the oracle's memory_of / core_naic / decode_na / logit -- that tests/test_gpu_mask_predict.py holds the
kernel and the engine to.  The reference has no refinement loop, so this module is where parity is pinned (include/boficap_hip.h,
BOFI_FLAG_MASK_PREDICT, states the same rules in words)."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import torch
import torch.nn.functional as F

import boficap_oracle as O
from conftest import ROOT, load_golden

NAN = float("nan")


# ----------------------------------------------------------------------------- the step, restated
def conf_rank(c, n):
    """rank(s) = #{j < n : c[j] comes before c[s]} for s < len(c): NaN before every number, then by value, ties and NaNs by position."""
    c = np.asarray(c, np.float32)
    S = len(c)
    rank = np.zeros(S, np.int64)
    for s in range(S):
        for j in range(n):
            nj, ns = bool(np.isnan(c[j])), bool(np.isnan(c[s]))
            if nj != ns:
                before = nj
            elif nj:
                before = j < s
            else:
                before = bool(c[j] < c[s]) or (bool(c[j] == c[s]) and j < s)
            rank[s] += before
    return rank


def step_np(state, fresh, mask, last, t, T, bos, pad):
    """One step behind pass ``t`` of ``T`` + 1.  state = (y int64, c float32, e float32, r int32) [B, S] (anything before pass 0), fresh = (y, c, e) of the
    pass, mask int32 [B, S] of pass t (ignored at t = 0).  Returns (state', mask', next_ids): mask' / next_ids are those of pass t + 1, or None after the
    last pass (the outputs seq / row statistics / emitted_round are then state')."""
    y, c, e, r = (np.array(a, copy=True) for a in state)
    fy, fc, fe = fresh
    B, S = fy.shape
    nm = np.zeros((B, S), np.int32)
    nxt = np.zeros((B, S), np.int64)
    for b in range(B):
        n = min(max(int(last[b]) - 1, 0), S)
        for s in range(S):
            if s >= n or t == 0 or mask[b, s] != 0:
                y[b, s], c[b, s], e[b, s] = fy[b, s], fc[b, s], fe[b, s]
                r[b, s] = t if s < n else 0
        if t < T:
            k = n * (T + 1 - (t + 1)) // (T + 1)
            rank = conf_rank(c[b], n)
            for s in range(S):
                nm[b, s] = 1 if (s < n and rank[s] < k) else 0
                nxt[b, s] = bos if nm[b, s] else y[b, s]
    return (y, c, e, r), (nm if t < T else None), (nxt if t < T else None)


# ----------------------------------------------------------------------------- the whole decode, restated on the oracle
def _fill_mask(cfg, last, B, fix_q1):
    S = cfg.seq_length
    syn_mask = torch.zeros(B, S, S, dtype=torch.bool)
    for i in range(B):
        n = int(last[i] if fix_q1 else last[B - 1]) - 1            # quirk Q1 as core_naic has it
        syn_mask[i, :, :max(n, 0)] = True
    return syn_mask


@functools.lru_cache(maxsize=None)
def _case(name):
    """(cfg, state dict, att_feats, att_masks or None) of a golden case, from seeds."""
    import json
    from boficap_amd import weights as W
    from boficap_amd.config import FULL, TINY, TINY_N2
    with open(os.path.join(ROOT, "tests", "golden", "manifest.json")) as f:
        m = json.load(f)[name]
    cfg = {"TINY": TINY, "FULL": FULL, "TINY_N2": TINY_N2}[m["config"]]
    sd = W.make_state_dict(cfg, seed=m["seed"], gen_scale=m["gen_scale"])
    if m.get("patch") == "len_row_shared":
        sd = W.with_len_row_shared(sd, cfg)
    assert W.digest(sd) == m["digest"]
    g = load_golden(name)
    if name == "full_b8":
        att = torch.from_numpy(W.synthetic_att_feats(m["pool_size"], 36, cfg.att_feat_size, seed=m["pool_seed"])[g["pool_index"]])
        masks = None
    else:
        att = torch.from_numpy(g["att_feats"])
        masks = torch.from_numpy(g["att_masks"]) if "att_masks" in g else None
    return cfg, sd, att, masks


@functools.lru_cache(maxsize=None)
def restate(name, T, method="mask_predict", margin=1e-3):
    """The decode of golden case ``name`` with ``T`` extra passes (strict Q1), computed once and shared: a dict with the slot layout, ``seq``, the last pass's
    ``lp``, and for mask-predict ``round`` / ``chosen`` / ``plogp`` of the state and ``safe`` [B]: in this run every selection boundary (the gap between
    the k-th and (k+1)-th lowest confidence, all rounds) and every top-2 log-prob gap at a position being emitted exceeds ``margin``.
    ``method`` 'feed_back' restates the other refinement on the same passes (all of the previous ids as input)."""
    cfg, sd, att, masks = _case(name)
    w = O.as_torch(sd)
    with torch.no_grad():
        memory, src_mask = O.memory_of(w, cfg, att, masks)
        _, pn, pl, ps, dg = O.core_naic(w, cfg, memory, src_mask)
        B, S = memory.size(0), cfg.seq_length
        last = dg["last"].numpy()
        syn_mask = _fill_mask(cfg, last, B, False)
        state = (np.zeros((B, S), np.int64), np.zeros((B, S), np.float32), np.zeros((B, S), np.float32), np.zeros((B, S), np.int32))
        mask, ids = np.zeros((B, S), np.int32), None
        safe = np.ones(B, bool)
        gaps = np.full(B, np.inf)
        for t in range(T + 1):
            phrase = O.decode_na(w, cfg, memory, dg["ext_syn"][:, 1:-1], src_mask, syn_mask, glat_input=None if ids is None else torch.from_numpy(ids))
            lp = F.log_softmax(O.logit(w, phrase), dim=2)
            fy = torch.max(lp, 2)[1].long()
            for b in range(B):
                fy[b, max(int(last[b]) - 1, 0):] = cfg.pad_idx
            fc = lp.gather(2, fy.unsqueeze(2)).squeeze(2).numpy()
            fe = (lp.exp() * lp).sum(2).numpy()
            if method == "feed_back":
                ids = fy.numpy()
                state = (ids, fc, fe, np.zeros((B, S), np.int32))
                continue
            top = torch.topk(lp, 2, dim=2)[0]
            top_gap = (top[..., 0] - top[..., 1]).numpy()
            for b in range(B):
                n = min(max(int(last[b]) - 1, 0), S)
                for s in range(n):
                    if (t == 0 or mask[b, s]) and not top_gap[b, s] > margin:
                        safe[b] = False
            state, mask, ids = step_np(state, (fy.numpy(), fc, fe), mask, last, t, T, cfg.bos_idx, cfg.pad_idx)
            if t < T:
                for b in range(B):
                    n = min(max(int(last[b]) - 1, 0), S)
                    k = int(mask[b].sum())
                    if 0 < k < n:
                        srt = np.sort(state[1][b, :n])              # (NaNs last: a NaN makes the gap NaN and the image unsafe)
                        gap = float(srt[k] - srt[k - 1])
                        gaps[b] = min(gaps[b], gap) if gap == gap else NAN
                        if not gap > margin:
                            safe[b] = False
    return dict(cfg=cfg, sd=sd, att=att, masks=masks, phrase_num=pn, phrase_length=pl, phrase_syn=ps, last=last, seq=torch.from_numpy(np.asarray(state[0])), lp=lp,
                chosen=state[1], plogp=state[2], round=state[3], safe=safe, min_selection_gap=gaps)


# ----------------------------------------------------------------------------- tests
def test_declarations_agree():
    """The step's entry point, the flag and the per-call record that carries refine_round: header, ctypes table and build list."""
    from boficap_amd import build, hip
    header = open(os.path.join(ROOT, "include", "boficap_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, arity in (("bofi_mask_predict_step", 21),):
        found = re.findall(r"\b" + name + r"\s*\(([^;{]*?)\)\s*;", code, flags=re.S)
        assert len(found) == 1 and found[0].count(",") + 1 == len(hip.SIGNATURES[name][1]) == arity, name
    # the per-call record: the header's field list is the ctypes mirror's, in order, and its size is the one the engine's graph key asserts
    body = re.search(r"typedef\s+struct\s+bofi_call_opts\s*\{(.*?)\}\s*bofi_call_opts_t\s*;", code, flags=re.S).group(1)
    assert re.findall(r"(\w+)\s*;", body) == [n for n, _ in hip.BofiCallOpts._fields_]
    pinned = re.findall(r"static_assert\(sizeof\(bofi_call_opts_t\) == (\d+)", open(os.path.join(build.CSRC, "engine.hip")).read())
    assert len(pinned) == 1 and C.sizeof(hip.BofiCallOpts) == int(pinned[0])
    assert "refine_round" in dict(hip.BofiCallOpts._fields_)
    assert re.search(r"#define\s+BOFI_FLAG_MASK_PREDICT\s+16384\b", header) and hip.FLAG_MASK_PREDICT == 16384
    assert "refine.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "refine.hip"))
    assert "launch_mask_predict_step" in open(os.path.join(build.CSRC, "bofi_kernels.h")).read()
    assert hip.ABI_VERSION == 5
    flags = [v for k, v in vars(hip).items() if k.startswith("FLAG_") and k != "FLAG_REFINE_SHIFT"]
    assert all(hip.FLAG_MASK_PREDICT & v == 0 for v in flags if v != hip.FLAG_MASK_PREDICT) and hip.FLAG_MASK_PREDICT & (15 << hip.FLAG_REFINE_SHIFT) == 0


def test_step_restatement_on_a_hand_worked_case():
    """n = 5 of S = 6, T = 3: k = 3, 2, 1.  One NaN (ranks first), ties (-0.5 at positions 0 and 3, later 0, 2, 3: the lower position goes first), and position 4
    masked again in pass 2 after pass 1 re-emitted it.  Pass p leaves id 10 p + 10 + s and sum p log p = -(10 p + s) at position s; worked by hand."""
    BOS, PAD, T = 1, 0, 3
    last = np.array([6])
    conf = [[-0.5, NAN, -2.0, -0.5, -1.0, -0.1],
            [-9.0, -0.3, -0.5, -9.0, -3.0, -0.2],
            [-0.1, -7.0, -7.0, -7.0, -0.4, -0.3],
            [-8.0, -8.0, -0.05, -8.0, -8.0, -0.6]]
    want_mask = [[0, 1, 1, 0, 1, 0], [1, 0, 0, 0, 1, 0], [0, 0, 1, 0, 0, 0]]
    want_next = [[10, BOS, BOS, 13, BOS, PAD], [BOS, 21, 22, 13, BOS, PAD], [30, 21, BOS, 13, 34, PAD]]
    want_y = [[10, 11, 12, 13, 14, PAD], [10, 21, 22, 13, 24, PAD], [30, 21, 22, 13, 34, PAD], [30, 21, 42, 13, 34, PAD]]
    want_c = [conf[0], [-0.5, -0.3, -0.5, -0.5, -3.0, -0.2], [-0.1, -0.3, -0.5, -0.5, -0.4, -0.3], [-0.1, -0.3, -0.05, -0.5, -0.4, -0.6]]
    want_r = [[0] * 6, [0, 1, 1, 0, 1, 0], [2, 1, 1, 0, 2, 0], [2, 1, 3, 0, 2, 0]]
    want_e_final = [-20.0, -11.0, -32.0, -3.0, -24.0, -35.0]
    assert [5 * (T + 1 - t) // (T + 1) for t in (1, 2, 3)] == [3, 2, 1]
    state = tuple(np.full((1, 6), v, d) for v, d in ((77, np.int64), (5.0, np.float32), (5.0, np.float32), (9, np.int32)))      # (pass 0 must not read it)
    mask = np.ones((1, 6), np.int32)
    for t in range(T + 1):
        fy = np.array([[10 * t + 10 + s for s in range(5)] + [PAD]], np.int64)
        fe = np.array([[-(10.0 * t + s) for s in range(6)]], np.float32)
        state, mask, nxt = step_np(state, (fy, np.array([conf[t]], np.float32), fe), mask, last, t, T, BOS, PAD)
        assert state[0][0].tolist() == want_y[t], t
        np.testing.assert_array_equal(state[1][0], np.array(want_c[t], np.float32))
        assert state[3][0].tolist() == want_r[t], t
        if t < T:
            assert mask[0].tolist() == want_mask[t] and nxt[0].tolist() == want_next[t], t
        else:
            assert mask is None and nxt is None
    assert state[2][0].tolist() == want_e_final
    # the order itself: NaNs first and among themselves by position, -inf before finite numbers, equal values by position, +-0 equal
    assert conf_rank([0.0, NAN, -np.inf, -0.0, NAN, -1.0], 6).tolist() == [4, 0, 2, 5, 1, 3]
    assert conf_rank([3.0, 1.0, 2.0], 2).tolist() == [1, 0, 1]         # (only the first n positions are counted)


def test_restated_decode_on_the_tiny_model():
    """The whole restatement on the tiny model (CPU oracle): the schedule's counts, the pad tail, and T passes that leave pass 0's tokens where round 0 stands."""
    for T in (1, 3):
        r = restate("tiny_saic_multi", T)
        base = restate("tiny_saic_multi", 0)
        cfg = r["cfg"]
        for b, la in enumerate(r["last"]):
            n = int(la) - 1
            rd, seq = r["round"][b], r["seq"][b].numpy()
            assert n == int(r["phrase_length"][b].sum())
            assert (seq[n:] == cfg.pad_idx).all() and (rd[n:] == 0).all()
            assert int((rd[:n] == T).sum()) == n // (T + 1)
            for t in range(1, T + 1):
                assert int((rd[:n] == t).sum()) <= n * (T + 1 - t) // (T + 1)
            keep = rd[:n] == 0
            assert (seq[:n][keep] == base["seq"][b].numpy()[:n][keep]).all()
    assert (restate("tiny_saic_multi", 0)["round"] == 0).all()


def test_eval_cli_refuses_refinement_with_saic():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval.py"), "--inference_mode", "SAIC", "--refine_method", "mask_predict"],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 2, (p.returncode, p.stderr[-400:])
    assert "--inference_mode NAIC" in p.stderr and "refine" in p.stderr
