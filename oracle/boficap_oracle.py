"""CPU oracle for the BoFiCap bound+fill hot path.  TEST INFRASTRUCTURE ONLY.

This is a plain float32 restatement (torch CPU tensors, functional style, dense masks) of the
reference's algorithm.  It is the checker for ``tests/``, ``__graft_entry__.smoke()`` and the
``cpu_baseline`` leg of ``bench.py``; nothing in ``boficap_amd/`` may import it, and the product
path never routes through it.

Parity status: PINNED.  ``oracle/make_golden.py`` imports the real reference in the build
container, runs it on weights from ``boficap_amd.weights.make_state_dict`` and asserts that this
oracle reproduces every tensor; the outputs are committed under ``tests/golden/`` and
``tests/test_oracle_golden.py`` re-checks the oracle against them without the reference.

Every function cites the reference lines it restates (paths relative to ``/root/reference``;
TM = captioning/models/TransformerModel.py, AM = captioning/models/AttModel.py,
CM = captioning/models/CaptionModel.py).  Weights are a flat dict keyed like the reference's
``state_dict()``.
"""
from __future__ import annotations

import math
import time
from typing import Dict, Optional

import torch
import torch.nn.functional as F

LENGTH_DIM, SYN_DIM, SYN_LOWER, SYN_UPPER = 20, 10, 4, 6      # TM:329-332 / TM:39-42
NEG_INF = float("-inf")

Weights = Dict[str, torch.Tensor]


def as_torch(sd) -> Weights:
    return {k: (v if torch.is_tensor(v) else torch.from_numpy(v)).float() for k, v in sd.items()}


# ----------------------------------------------------------------------------- building blocks
def layer_norm(x, w: Weights, p: str, eps: float = 1e-6):
    """TM:1346-1349 -- unbiased std, eps added to std (NOT nn.LayerNorm)."""
    mean = x.mean(-1, keepdim=True)
    std = x.std(-1, keepdim=True)
    return w[p + ".a_2"] * (x - mean) / (std + eps) + w[p + ".b_2"]


def linear(x, w: Weights, p: str):
    return F.linear(x, w[p + ".weight"], w[p + ".bias"])


def attention(w: Weights, p: str, q_in, kv_in, mask, h: int):
    """TM:1446-1467 + TM:1421-1432.  mask: bool [B,1|Lq,Lk], True = may attend."""
    B, Lq, d = q_in.shape
    dk = d // h
    q = linear(q_in, w, p + ".linears.0").view(B, -1, h, dk).transpose(1, 2)
    k = linear(kv_in, w, p + ".linears.1").view(B, -1, h, dk).transpose(1, 2)
    v = linear(kv_in, w, p + ".linears.2").view(B, -1, h, dk).transpose(1, 2)
    scores = torch.matmul(q, k.transpose(-2, -1)) / math.sqrt(dk)
    scores = scores.masked_fill(mask.unsqueeze(1) == 0, NEG_INF)
    p_attn = F.softmax(scores, dim=-1)          # a fully masked row is NaN, as in the reference
    ctx = torch.matmul(p_attn, v).transpose(1, 2).contiguous().view(B, Lq, d)
    return linear(ctx, w, p + ".linears.3")


def feed_forward(w: Weights, p: str, x):
    """TM:1477-1478 (dropout off)."""
    return linear(F.relu(linear(x, w, p + ".w_1")), w, p + ".w_2")


def embed(w: Weights, p: str, ids, d: int):
    """TM:1486-1487."""
    return w[p + ".lut.weight"][ids] * math.sqrt(d)


def add_pe(w: Weights, x):
    """TM:1505-1507 (dropout off)."""
    return x + w["model.pos_embed.pe"][:, : x.size(1)]


# ----------------------------------------------------------------------------- encoder (a1, a2)
def prepare_feature(w: Weights, cfg, att_feats, att_masks: Optional[torch.Tensor]):
    """TM:1674-1690 + AM:113-120 + AM:46-51.  Returns (embedded regions, src mask [B,1,R])."""
    if att_masks is not None:
        max_len = int(att_masks.long().sum(1).max())
        att_feats = att_feats[:, :max_len].contiguous()
        att_masks = att_masks[:, :max_len].contiguous()
    x = F.relu(linear(att_feats, w, "att_embed.0"))
    if att_masks is not None:
        # pack_padded_sequence -> module -> pad_packed_sequence: rows past each image's length
        # come back as exact zeros (AM:46-49), not relu(bias)
        lens = att_masks.long().sum(1)
        keep = torch.arange(x.size(1))[None, :] < lens[:, None]
        x = x * keep.unsqueeze(-1).to(x.dtype)
        src_mask = att_masks.bool().unsqueeze(-2)
    else:
        src_mask = torch.ones(x.shape[:2], dtype=torch.bool).unsqueeze(-2)
    return x, src_mask


def encode(w: Weights, cfg, x, src_mask):
    """TM:1332-1336, 1374-1377."""
    for l in range(cfg.N_enc):
        p = f"model.encoder.layers.{l}"
        n = layer_norm(x, w, p + ".sublayer.0.norm")
        x = x + attention(w, p + ".self_attn", n, n, src_mask, cfg.h)
        x = x + feed_forward(w, p + ".feed_forward", layer_norm(x, w, p + ".sublayer.1.norm"))
    return layer_norm(x, w, "model.encoder.norm")


def memory_of(w: Weights, cfg, att_feats, att_masks=None):
    x, src_mask = prepare_feature(w, cfg, att_feats, att_masks)
    return encode(w, cfg, x, src_mask), src_mask


# ----------------------------------------------------------------------------- bounding network (a7, a8)
def bound_row0(w: Weights, cfg, input_embed, memory, src_mask, tgt_mask):
    """Bound layers + final norm, row 0 ([LEN]) only is returned (TM:367-375; layer TM:1025-1029)."""
    lp = "model.length_predictor"
    x = input_embed
    for l in range(cfg.N_len):
        p = f"{lp}.LengthPredictor.{l}"
        n = layer_norm(x, w, p + ".sublayer.0.norm")
        x = x + attention(w, p + ".self_attn", n, n, tgt_mask, cfg.h)
        n = layer_norm(x, w, p + ".sublayer.1.norm")
        x = x + attention(w, p + ".src_attn", n, memory, src_mask, cfg.h)
        x = x + feed_forward(w, p + ".ff", layer_norm(x, w, p + ".sublayer.2.norm"))
    return layer_norm(x, w, lp + ".norm")[:, 0, :]


def bound_heads(w: Weights, out):
    """TM:376-383 (dropout off): two 2-layer heads, log-softmax, first-max argmax."""
    lp = "model.length_predictor"
    len_logp = F.log_softmax(linear(F.relu(linear(out, w, lp + ".Length_classifier1")), w, lp + ".Length_classifier2"), dim=-1)
    syn_logp = F.log_softmax(linear(F.relu(linear(out, w, lp + ".Syntactic_classifier1")), w, lp + ".Syntactic_classifier2"), dim=-1)
    len_n = torch.max(len_logp, 1)[1].int()
    syn_n = torch.max(syn_logp, 1)[1].long()
    return len_n, len_logp, syn_n, syn_logp


def bound_step(w: Weights, cfg, input_embed, memory, src_mask, tgt_mask):
    """LengthPredictor_UIC.forward TM:357-383 with N_len >= 1."""
    return bound_heads(w, bound_row0(w, cfg, input_embed, memory, src_mask, tgt_mask))


def bound_step_na(w, cfg, extend_phrase_syn, memory, src_mask, tgt_mask):
    """TM:567-568."""
    return bound_step(w, cfg, add_pe(w, embed(w, "model.syn_embed", extend_phrase_syn, cfg.d_model)),
                      memory, src_mask, tgt_mask)


def bound_step_sa(w, cfg, word_seq, memory, src_mask, tgt_mask):
    """TM:515-518."""
    return bound_step(w, cfg, add_pe(w, embed(w, "model.tgt_embed", word_seq, cfg.d_model)),
                      memory, src_mask, tgt_mask)


# ----------------------------------------------------------------------------- decoder (a10)
def decode(w: Weights, cfg, x, memory, src_mask, tgt_mask):
    """TM:1386-1396, 1408-1413."""
    for l in range(cfg.N_dec):
        p = f"model.decoder.layers.{l}"
        n = layer_norm(x, w, p + ".sublayer.0.norm")
        x = x + attention(w, p + ".self_attn", n, n, tgt_mask, cfg.h)
        n = layer_norm(x, w, p + ".sublayer.1.norm")
        x = x + attention(w, p + ".src_attn", n, memory, src_mask, cfg.h)
        x = x + feed_forward(w, p + ".feed_forward", layer_norm(x, w, p + ".sublayer.2.norm"))
    return layer_norm(x, w, "model.decoder.norm")


def decode_na(w, cfg, memory, syn_seq, src_mask, tgt_mask, glat_input=None):
    """TM:570-587, input mode 'add'."""
    word_seq = torch.full(syn_seq.shape, cfg.bos_idx, dtype=torch.long) if glat_input is None else glat_input
    x = add_pe(w, embed(w, "model.tgt_embed", word_seq, cfg.d_model) + embed(w, "model.syn_embed", syn_seq, cfg.d_model))
    return decode(w, cfg, x, memory, src_mask, tgt_mask)


def decode_sa(w, cfg, memory, word_seq, syn_seq, src_mask, tgt_mask):
    """TM:520-530, input mode 'add'."""
    x = add_pe(w, embed(w, "model.tgt_embed", word_seq, cfg.d_model) + embed(w, "model.syn_embed", syn_seq, cfg.d_model))
    return decode(w, cfg, x, memory, src_mask, tgt_mask)


def logit(w, x):
    """TM:1668-1669."""
    return linear(x, w, "model.generator.proj")


# ----------------------------------------------------------------------------- NAIC bound loop (a9)
def core_naic(w: Weights, cfg, memory, src_mask, *, fix_q1: bool = False, trace=None):
    """TM:1823-1876, including quirk Q1 (the fill mask of EVERY row uses the last row's length,
    TM:1872-1873) unless ``fix_q1``.  Returns the fill output and the slot layout, plus
    diagnostics (iterations executed, ``last`` per image)."""
    B = memory.size(0)
    S = cfg.seq_length
    L = S + 2
    phrase_num = torch.zeros(B, dtype=torch.int)
    phrase_length = torch.zeros(B, L, dtype=torch.int)
    phrase_syn = torch.full((B, L), cfg.pad_idx, dtype=torch.long)
    ext_syn = torch.full((B, L), cfg.pad_idx, dtype=torch.long)
    tgt_mask = torch.zeros(B, L, L, dtype=torch.bool)
    last = torch.zeros(B, dtype=torch.int)
    finished = torch.zeros(B, dtype=torch.bool)
    reason = ["maxiter"] * B                                 # diagnostics only
    iters = 0
    for i in range(S):
        if i == 0:
            ext_syn[:, 0] = cfg.len_idx
            tgt_mask[:, :, 0] = True
            last[:] = 1
        out0 = bound_row0(w, cfg, add_pe(w, embed(w, "model.syn_embed", ext_syn, cfg.d_model)), memory, src_mask, tgt_mask)
        len_n, len_logp, syn_n, syn_logp = bound_heads(w, out0)                      # == TM:567-568
        if trace is not None:
            trace.append(dict(out0=out0.clone(), len_logp=len_logp.clone(), syn_logp=syn_logp.clone(),
                              active=~finished.clone(), ext_syn=ext_syn.clone(), last=last.clone()))
        iters += 1
        for j in range(B):
            if finished[j]:
                continue
            ln, sn, la = int(len_n[j]), int(syn_n[j]), int(last[j])
            if ln == 0 or sn < SYN_LOWER or sn > SYN_UPPER:
                finished[j] = True
                reason[j] = "len0" if ln == 0 else "syn"
                continue
            if ln + la >= S + 1:
                ln = S + 1 - la
                finished[j] = True
                reason[j] = "trunc"
            phrase_length[j, i] = ln
            phrase_syn[j, i] = sn
            phrase_num[j] += 1
            ext_syn[j, la:la + ln] = sn
            tgt_mask[j, la:, :la + ln] = True
            last[j] = la + ln
            tgt_mask[j, 0, :la + ln] = True
        if bool(finished.all()):
            break
    syn_mask = torch.zeros(B, S, S, dtype=torch.bool)
    for i in range(B):
        n = int(last[i] if fix_q1 else last[B - 1]) - 1      # Q1: stale loop variable j == B-1
        syn_mask[i, :, :max(n, 0)] = True
    phrase = decode_na(w, cfg, memory, ext_syn[:, 1:-1], src_mask, syn_mask)
    return phrase, phrase_num, phrase_length[:, :-2], phrase_syn[:, :-2], dict(iters=iters, last=last.clone(), ext_syn=ext_syn.clone(), reason=reason)


def layout_of(cfg, out):
    """(ext_syn int64 [B, S + 2], last numpy int64 [B]) of a decode's slot layout, as core_NAIC builds them (TransformerModel.py:1829-1869), from its exported
    phrase_length / phrase_syn."""
    import numpy as np
    pl, ps = out["phrase_length"].cpu().numpy(), out["phrase_syn"].cpu().numpy()
    B, S = pl.shape
    ext = np.full((B, S + 2), cfg.pad_idx, np.int64)
    ext[:, 0] = cfg.len_idx
    last = np.ones(B, np.int64)
    for b in range(B):
        for i in range(S):
            if pl[b, i] > 0:
                ext[b, last[b]:last[b] + pl[b, i]] = ps[b, i]
                last[b] += pl[b, i]
    return torch.from_numpy(ext), last


def sample_naic_refine(w: Weights, cfg, att_feats, att_masks=None, *, rounds: int = 2, fix_q1: bool = False):
    """Iterative refinement of the filling pass (BASELINE config 5).  NOT in the reference: parity unpinned.
    Defined on the reference's own hook decode_NA(..., glat_input) TM:570-574: round r > 0 decodes with the
    greedy ids of round r-1 (after the pad-tail rule) as word_seq, same slot layout and fill mask."""
    memory, src_mask = memory_of(w, cfg, att_feats, att_masks)
    _, phrase_num, phrase_length, phrase_syn, dg = core_naic(w, cfg, memory, src_mask, fix_q1=fix_q1)
    B, S = memory.size(0), cfg.seq_length
    syn_mask = torch.zeros(B, S, S, dtype=torch.bool)
    for i in range(B):
        n = int(dg["last"][i] if fix_q1 else dg["last"][B - 1]) - 1
        syn_mask[i, :, :max(n, 0)] = True
    seq = None
    for r in range(rounds + 1):
        phrase = decode_na(w, cfg, memory, dg["ext_syn"][:, 1:-1], src_mask, syn_mask, glat_input=seq)
        lp = F.log_softmax(logit(w, phrase), dim=2)
        seq = torch.max(lp, 2)[1].long()
        for b in range(B):
            seq[b, int(phrase_length[b].sum()):] = cfg.pad_idx
    return seq, lp, phrase_num, phrase_length, phrase_syn


def sample_naic(w: Weights, cfg, att_feats, att_masks=None, *, output_logsoftmax: int = 1,
                fix_q1: bool = False):
    """AM:307-338, 419-429 + AM:203-210 + CM:388-390, greedy, sample_n = 1.
    Returns the reference's 6-tuple (the last element is elapsed seconds)."""
    memory, src_mask = memory_of(w, cfg, att_feats, att_masks)
    t0 = time.time()
    phrase, phrase_num, phrase_length, phrase_syn, _ = core_naic(w, cfg, memory, src_mask, fix_q1=fix_q1)
    lg = logit(w, phrase)
    seq_logprob = F.log_softmax(lg, dim=2) if output_logsoftmax else lg
    seq = torch.max(seq_logprob, 2)[1].long()
    for b in range(seq.size(0)):
        seq[b, int(phrase_length[b].sum()):] = cfg.pad_idx
    return seq, seq_logprob, phrase_num, phrase_length, phrase_syn, time.time() - t0


# ----------------------------------------------------------------------------- SAIC (a16, next row f1)
def core_saic(w: Weights, cfg, memory, src_mask, *, output_logsoftmax: int = 1):
    """TM:1878-1986, greedy."""
    B = memory.size(0)
    S = cfg.seq_length
    L = S + 2
    V = w["model.generator.proj.weight"].size(0)
    phrase_num = torch.zeros(B, dtype=torch.int)
    phrase_length = torch.zeros(B, L, dtype=torch.int)
    phrase_syn = torch.full((B, L), cfg.pad_idx, dtype=torch.long)
    seq = torch.full((B, L), cfg.pad_idx, dtype=torch.long)
    seq_logprobs = torch.zeros(B, L, V)
    ext_len = torch.full((B, L), cfg.pad_idx, dtype=torch.long)
    ext_phrase = torch.full((B, L), cfg.pad_idx, dtype=torch.long)
    ext_syn = torch.full((B, L), cfg.pad_idx, dtype=torch.long)
    len_mask = torch.zeros(B, L, L, dtype=torch.bool)
    phrase_mask = torch.zeros(B, L, L, dtype=torch.bool)
    finished = torch.zeros(B, dtype=torch.bool)
    seq_last = torch.zeros(B, dtype=torch.int)
    phrase_last = torch.zeros(B, dtype=torch.int)
    iters = 0
    for i in range(1, S + 1):
        if i == 1:
            seq[:, 0] = cfg.bos_idx
            phrase_length[:, 0] = 1
            ext_len[:, 0] = cfg.len_idx
            len_mask[:, :, 0] = True
            phrase_last[:] = 1
        len_n, _, syn_n, _ = bound_step_sa(w, cfg, ext_len.clone(), memory, src_mask, len_mask)
        iters += 1
        for j in range(B):
            if finished[j]:
                continue
            ln, sn, pl = int(len_n[j]), int(syn_n[j]), int(phrase_last[j])
            if ln == 0 or sn < SYN_LOWER or sn > SYN_UPPER:
                finished[j] = True
                continue
            if ln + pl >= S + 1:
                ln = S + 1 - pl
                finished[j] = True
            phrase_length[j, i] = ln
            phrase_syn[j, i] = sn
            phrase_num[j] += 1
        for j in range(B):
            cur = int(phrase_length[j, i])
            if cur == 0:
                continue
            pl, sl, prev = int(phrase_last[j]), int(seq_last[j]), int(phrase_length[j, i - 1])
            ext_syn[j, pl:pl + cur] = phrase_syn[j, i]
            if cur <= prev:                                   # TM:1934-1936
                pre_pad = prev - cur
                ext_phrase[j, pl:pl + cur] = seq[j, sl + pre_pad: sl + pre_pad + cur]
            else:                                             # TM:1937-1947 positionwise stretch
                pre_less = prev - (cur % prev)
                times = cur // prev
                copied = 0
                for k in range(prev):
                    n = times if k < pre_less else times + 1
                    ext_phrase[j, pl + copied: pl + copied + n] = seq[j, sl + k]
                    copied += n
            phrase_mask[j, pl:, :pl + cur] = True
        phrase = decode_sa(w, cfg, memory, ext_phrase.clone()[:, 1:-1], ext_syn.clone()[:, 1:-1],
                           src_mask, phrase_mask[:, 1:-1, 1:-1])
        lg = logit(w, phrase)
        phrase_logprobs = F.log_softmax(lg, dim=2) if output_logsoftmax else lg
        if bool(phrase_logprobs.isnan().any()):               # TM:1956-1958
            return seq[:, 1:-1], seq_logprobs[:, 1:-1, :], phrase_num, phrase_length[:, 1:-1], phrase_syn[:, 1:-1], dict(iters=iters, nan=True)
        tok = torch.max(phrase_logprobs, 2)[1].long()
        for j in range(B):
            cur = int(phrase_length[j, i])
            if cur == 0:
                continue
            pl = int(phrase_last[j])
            seq[j, pl:pl + cur] = tok[j, pl - 1: pl - 1 + cur]
            seq_logprobs[j, pl:pl + cur] = phrase_logprobs[j, pl - 1: pl - 1 + cur]
            ext_len[j, pl:pl + cur] = tok[j, pl - 1: pl - 1 + cur]
            len_mask[j, pl:, :pl + cur] = True
            phrase_last[j] = pl + cur
            len_mask[j, 0, :pl + cur] = True
            seq_last[j] += int(phrase_length[j, i - 1])
        if bool(finished.all()):
            break
    return seq[:, 1:-1], seq_logprobs[:, 1:-1, :], phrase_num, phrase_length[:, 1:-1], phrase_syn[:, 1:-1], dict(iters=iters, nan=False)


def sample_saic(w: Weights, cfg, att_feats, att_masks=None, *, output_logsoftmax: int = 1):
    """AM:430-437."""
    memory, src_mask = memory_of(w, cfg, att_feats, att_masks)
    t0 = time.time()
    seq, lp, pn, pl, ps, _ = core_saic(w, cfg, memory, src_mask, output_logsoftmax=output_logsoftmax)
    return seq, lp, pn, pl, ps, time.time() - t0


# ----------------------------------------------------------------------------- XE training forward (a14) and criterion (a15)
def _teacher_forced_bound(w, cfg, input_embed, memory, src_mask, phrase_num, phrase_length):
    """get_predict_phrase_length_syn_SA / _NA, TM:476-513 / TM:532-565 (shared body): one predictor pass per
    phrase index with the mask grown per caption; pass i lands in slot i+1; returns ([N,L-1,20], [N,L-1,10], last)."""
    B, L = phrase_length.shape
    tgt_mask = torch.zeros(B, L, L, dtype=torch.bool)
    len_lp = torch.zeros(B, L, LENGTH_DIM)
    syn_lp = torch.zeros(B, L, SYN_DIM)
    last = torch.ones(B, dtype=torch.int)
    tgt_mask[:, :, 0] = True
    _, a, _, b = bound_step(w, cfg, input_embed, memory, src_mask, tgt_mask)
    len_lp[:, 1], syn_lp[:, 1] = a, b
    for i in range(1, int(phrase_num.max())):
        for j in range(B):
            if int(phrase_num[j]) <= i:
                continue
            la, pl = int(last[j]), int(phrase_length[j, i])
            tgt_mask[j, la:, :la + pl] = True
            last[j] = la + pl
            tgt_mask[j, 0, :la + pl] = True
        _, a, _, b = bound_step(w, cfg, input_embed, memory, src_mask, tgt_mask)
        len_lp[:, i + 1], syn_lp[:, i + 1] = a, b
    return len_lp[:, 1:, :], syn_lp[:, 1:, :], last


def glance_input(cfg, na_pred_tokens, labels, phrase_length, glat_p: float, uniform):
    """The glancing decoder input of EncoderDecoder_UIC.forward, TM:441-460: reveal the true token at a position with
    probability (share of mispredicted tokens of that caption) * glat_p, [BOS] elsewhere.  ``uniform``: the [N, S] draws
    the reference takes from torch.rand (TM:455) -- injected, so that both sides see the same numbers."""
    real = labels[:, 1:-1]
    N, S = real.shape
    tokens_length = phrase_length.sum(1) - 1
    phrase_mask = torch.zeros(N, S, dtype=torch.bool)
    for i in range(N):
        phrase_mask[i, 0:int(tokens_length[i])] = True
    same_num = ((na_pred_tokens == real) & phrase_mask).sum(1)
    mismatch_prob = (tokens_length - same_num) / tokens_length
    keep_prob = (mismatch_prob * glat_p).unsqueeze(-1) * phrase_mask.float()
    keep = uniform < keep_prob
    bos = torch.full(real.shape, cfg.bos_idx, dtype=torch.long)
    return bos.masked_fill(keep, 0) + real.masked_fill(~keep, 0)


def forward_uic(w: Weights, cfg, att_feats, labels, att_masks, phrase_num, phrase_length, phrase_syn,
                extend_phrase_syn_seq, extend_phrase_seq, extend_phrase_seq_mask, glat_p: float = -1.0, glat_uniform=None):
    """TransformerModel._forward TM:1713-1724,1759-1775 -> EncoderDecoder_UIC.forward TM:413-468, dropout off (eval mode);
    glat_p >= 0 takes the glancing pass TM:437-463 with the injected draws ``glat_uniform``.  Inputs may be [B, spi, ...];
    returns the six log-prob tensors."""
    if labels.dim() == 3:
        labels = labels.reshape(-1, labels.shape[2])
        phrase_num = phrase_num.reshape(-1)
        phrase_length = phrase_length.reshape(-1, phrase_length.shape[2])
        extend_phrase_syn_seq = extend_phrase_syn_seq.reshape(-1, extend_phrase_syn_seq.shape[2])
        extend_phrase_seq = extend_phrase_seq.reshape(-1, extend_phrase_seq.shape[2])
        extend_phrase_seq_mask = extend_phrase_seq_mask.reshape(-1, extend_phrase_seq.shape[1], extend_phrase_seq.shape[1])
    x, src_mask = prepare_feature(w, cfg, att_feats, att_masks)
    spi = labels.shape[0] // x.shape[0]
    if spi > 1:                                                         # TM:1703-1707, models/utils.py:3-14
        x = x.repeat_interleave(spi, dim=0)
        src_mask = src_mask.repeat_interleave(spi, dim=0)
    memory = encode(w, cfg, x, src_mask)
    d = cfg.d_model
    word_seq = labels.clone().long()
    word_seq[:, 0] = cfg.len_idx                                        # TM:478-479
    sa_len, sa_syn, _ = _teacher_forced_bound(w, cfg, add_pe(w, embed(w, "model.tgt_embed", word_seq, d)), memory, src_mask,
                                              phrase_num, phrase_length)
    sa_phrase = decode_sa(w, cfg, memory, extend_phrase_seq, extend_phrase_syn_seq[:, 1:-1], src_mask, extend_phrase_seq_mask)
    na_len, na_syn, last = _teacher_forced_bound(w, cfg, add_pe(w, embed(w, "model.syn_embed", extend_phrase_syn_seq, d)), memory,
                                                 src_mask, phrase_num, phrase_length)
    S = cfg.seq_length
    syn_mask = torch.zeros(labels.shape[0], S, S, dtype=torch.bool)
    for i in range(labels.shape[0]):
        syn_mask[i, :, :int(last[i]) - 1] = True                        # TM:562-564 (per-row index here)
    glanced = None
    if glat_p >= 0:                                                     # TM:437-460
        with torch.no_grad():
            pred = logit(w, decode_na(w, cfg, memory, extend_phrase_syn_seq[:, 1:-1], src_mask, syn_mask)).argmax(-1)
            glanced = glance_input(cfg, pred, labels.long(), phrase_length, glat_p, glat_uniform)
    na_phrase = decode_na(w, cfg, memory, extend_phrase_syn_seq[:, 1:-1], src_mask, syn_mask, glat_input=glanced)
    return (sa_len, sa_syn, F.log_softmax(logit(w, sa_phrase), dim=-1),
            na_len, na_syn, F.log_softmax(logit(w, na_phrase), dim=-1))


def ss_saic(w: Weights, cfg, memory, src_mask, labels, phrase_num, phrase_length, phrase_syn, ss_prob: float, draw):
    """Scheduled-sampling semi-autoregressive training pass, TransformerModel.ss_SAIC TM:1988-2121 (greedy, log-softmax): per phrase
    a bounding step on the words emitted so far, then -- per caption -- with probability ss_prob the model's own slot (half of the
    time with the previous emitted phrase copied position-wise as decoder input, otherwise [BOS] only), else the ground-truth slot
    and the previous ground-truth phrase; a full decode_SA pass; the new phrase's greedy tokens and log-probs are kept.
    ``draw()`` stands for ``random()`` (TM:2048,2049), called in the reference's order.  Gradients flow through the three
    returned tensors as in the reference.  Returns (len_logp [B, L-1, 20], syn_logp [B, L-1, 10], tok_logp [B, S, V], trace)."""
    B, L = phrase_length.shape
    S = L - 2
    V = w["model.generator.proj.weight"].size(0)
    labels, phrase_length, phrase_syn = labels.long(), phrase_length.long(), phrase_syn.long()
    ppn = torch.zeros(B, dtype=torch.int)
    ppl = torch.zeros(B, L, dtype=torch.long)
    pps = torch.full((B, L), cfg.pad_idx, dtype=torch.long)
    len_lps, syn_lps = [], []
    seq = torch.full((B, L), cfg.pad_idx, dtype=torch.long)
    seq_logprobs = torch.zeros(B, L, V)
    ext_len = torch.full((B, L), cfg.pad_idx, dtype=torch.long)
    ext_phrase = torch.full((B, L), cfg.pad_idx, dtype=torch.long)
    ext_syn = torch.full((B, L), cfg.pad_idx, dtype=torch.long)
    len_mask = torch.zeros(B, L, L, dtype=torch.bool)
    phrase_mask = torch.zeros(B, L, L, dtype=torch.bool)
    finished = torch.zeros(B, dtype=torch.bool)
    label_last = torch.zeros(B, dtype=torch.long)
    seq_last = torch.zeros(B, dtype=torch.long)
    phrase_last = torch.zeros(B, dtype=torch.long)
    choices = []

    def stretch(dst_row, pl, cur, src_row, s0, prev):        # the position-wise copy TM:2054-2067 / :2079-2092
        if cur <= prev:
            pre_pad = prev - cur
            dst_row[pl:pl + cur] = src_row[s0 + pre_pad: s0 + pre_pad + cur]
        else:
            pre_less, times, copied = prev - (cur % prev), cur // prev, 0
            for k in range(prev):
                n = times if k < pre_less else times + 1
                dst_row[pl + copied: pl + copied + n] = src_row[s0 + k]
                copied += n

    for i in range(1, L):
        if i == 1:
            seq[:, 0] = cfg.bos_idx
            ppl[:, 0] = 1
            ext_len[:, 0] = cfg.len_idx
            len_mask[:, :, 0] = True
            phrase_last[:] = 1
        len_n, len_lp, syn_n, syn_lp = bound_step_sa(w, cfg, ext_len.clone(), memory, src_mask, len_mask)
        len_lps.append(len_lp)
        syn_lps.append(syn_lp)
        for j in range(B):
            if finished[j]:
                continue
            ln, sn, pl = int(len_n[j]), int(syn_n[j]), int(phrase_last[j])
            if ln == 0 or sn < SYN_LOWER or sn > SYN_UPPER or int(phrase_length[j, i]) == 0:
                finished[j] = True
                continue
            if ln + pl >= L - 1:
                ln = L - 1 - pl
                finished[j] = True
            ppl[j, i], pps[j, i] = ln, sn
            ppn[j] += 1
        for j in range(B):
            if int(ppl[j, i]) == 0:
                continue
            pl = int(phrase_last[j])
            if draw() < ss_prob:
                cur = int(ppl[j, i])
                ext_syn[j, pl:pl + cur] = pps[j, i]
                if draw() < 0.5:                               # the previous EMITTED phrase as input
                    stretch(ext_phrase[j], pl, cur, seq[j], int(seq_last[j]), int(ppl[j, i - 1]))
                    choices.append((i, j, "own"))
                else:                                          # the slot's label only
                    ext_phrase[j, pl:pl + cur] = cfg.bos_idx
                    choices.append((i, j, "syn"))
            else:                                              # ground truth as input
                cur = min(int(phrase_length[j, i]), L - 1 - pl)
                ppl[j, i] = cur
                ext_syn[j, pl:pl + cur] = phrase_syn[j, i]
                stretch(ext_phrase[j], pl, cur, labels[j], int(label_last[j]), int(phrase_length[j, i - 1]))
                choices.append((i, j, "gt"))
            phrase_mask[j, pl:, :pl + cur] = True
        phrase = decode_sa(w, cfg, memory, ext_phrase.clone()[:, 1:-1], ext_syn.clone()[:, 1:-1], src_mask, phrase_mask[:, 1:-1, 1:-1])
        phrase_logprobs = F.log_softmax(logit(w, phrase), dim=2)
        if bool(phrase_logprobs.isnan().any()):
            raise FloatingPointError("ss_SAIC: NaN log-probs (a caption without any key); the reference returns a malformed tuple here (TM:2103-2105)")
        tok = torch.max(phrase_logprobs, 2)[1].long()
        rows = torch.zeros(B, L, dtype=torch.bool)
        for j in range(B):
            cur = int(ppl[j, i])
            if cur == 0:
                continue
            pl = int(phrase_last[j])
            seq[j, pl:pl + cur] = tok[j, pl - 1: pl - 1 + cur]
            rows[j, pl:pl + cur] = True
            ext_len[j, pl:pl + cur] = tok[j, pl - 1: pl - 1 + cur]
            len_mask[j, pl:, :pl + cur] = True
            phrase_last[j] = pl + cur
            len_mask[j, 0, :pl + cur] = True
            seq_last[j] += int(ppl[j, i - 1])
            label_last[j] += int(phrase_length[j, i - 1])
        # seq_logprobs[j, pl:pl+cur] = phrase_logprobs[j, pl-1:pl-1+cur] for the rows just placed (out of place, for autograd)
        shifted = torch.cat([torch.zeros(B, 1, V), phrase_logprobs, torch.zeros(B, 1, V)], 1)
        seq_logprobs = torch.where(rows.unsqueeze(-1), shifted, seq_logprobs)
        if bool(finished.all()):
            break
    n_it = len(len_lps)
    pad = lambda xs, width: torch.cat([torch.stack(xs, 1), torch.zeros(B, L - 1 - n_it, width)], 1)
    trace = dict(iters=n_it, choices=choices, seq=seq[:, 1:-1].clone(), predict_phrase_length=ppl.clone(), predict_phrase_num=ppn.clone())
    return pad(len_lps, len_lps[0].shape[-1]), pad(syn_lps, syn_lps[0].shape[-1]), seq_logprobs[:, 1:-1, :], trace


def forward_uic_ss(w: Weights, cfg, att_feats, labels, att_masks, phrase_num, phrase_length, phrase_syn, extend_phrase_syn_seq,
                   ss_prob: float, draw):
    """TransformerModel._forward with ss_prob > 0, TM:1760-1766: the SA branch from ss_saic, the NA branch teacher-forced without a
    glancing pass.  Dropout off.  Returns the six log-prob tensors and ss_saic's trace."""
    if labels.dim() == 3:
        labels = labels.reshape(-1, labels.shape[2])
        phrase_num = phrase_num.reshape(-1)
        phrase_length = phrase_length.reshape(-1, phrase_length.shape[2])
        phrase_syn = phrase_syn.reshape(-1, phrase_syn.shape[2])
        extend_phrase_syn_seq = extend_phrase_syn_seq.reshape(-1, extend_phrase_syn_seq.shape[2])
    x, src_mask = prepare_feature(w, cfg, att_feats, att_masks)
    spi = labels.shape[0] // x.shape[0]
    if spi > 1:
        x = x.repeat_interleave(spi, dim=0)
        src_mask = src_mask.repeat_interleave(spi, dim=0)
    memory = encode(w, cfg, x, src_mask)
    sa_len, sa_syn, sa_tok, trace = ss_saic(w, cfg, memory, src_mask, labels, phrase_num, phrase_length, phrase_syn, ss_prob, draw)
    na_len, na_syn, last = _teacher_forced_bound(w, cfg, add_pe(w, embed(w, "model.syn_embed", extend_phrase_syn_seq, cfg.d_model)), memory,
                                                 src_mask, phrase_num, phrase_length)
    S = cfg.seq_length
    syn_mask = torch.zeros(labels.shape[0], S, S, dtype=torch.bool)
    for i in range(labels.shape[0]):
        syn_mask[i, :, :int(last[i]) - 1] = True
    na_phrase = decode_na(w, cfg, memory, extend_phrase_syn_seq[:, 1:-1], src_mask, syn_mask)
    return (sa_len, sa_syn, sa_tok, na_len, na_syn, F.log_softmax(logit(w, na_phrase), dim=-1)), trace


def criterion_uic(outs, phrase_num, phrase_length, phrase_syn, labels, reduction="mean", self_dis=False):
    """LanguageModelCriterion_UIC.forward losses.py:319-369.  reduction 'mean' (:362-368) with the optional self-distillation term
    (:336-339, 366-368: KLDivLoss(NA, exp(SA).detach()) masked to the token positions, / token count).  reduction 'none' (:357-361)
    returns the per-caption value (six sums / the caption's token count) and None -- the reference's own 'none' branch ends in an
    UnboundLocalError (its return statement :369 names the 'mean' branch's variables), so this branch states :358 alone."""
    sa_len, sa_syn, sa_tok, na_len, na_syn, na_tok = outs
    if phrase_length.dim() == 3:
        phrase_num = phrase_num.reshape(-1)
        phrase_length = phrase_length.reshape(-1, phrase_length.shape[2])
        phrase_syn = phrase_syn.reshape(-1, phrase_syn.shape[2])
        labels = labels.reshape(-1, labels.shape[2])
    B = labels.shape[0]
    real = labels[:, 1:-1].long()
    tok_mask = torch.zeros(real.shape, dtype=torch.bool)
    for i in range(B):
        tok_mask[i, 0:int(phrase_length[i].sum()) - 1] = True
    sa_tok_loss = -sa_tok.gather(2, real.unsqueeze(2)).squeeze(2) * tok_mask
    na_tok_loss = -na_tok.gather(2, real.unsqueeze(2)).squeeze(2) * tok_mask
    len_lab, syn_lab = phrase_length[:, 1:].long(), phrase_syn[:, 1:].long()
    slot_mask = torch.zeros(len_lab.shape, dtype=torch.bool)
    for i in range(B):
        slot_mask[i, 0:int(phrase_num[i])] = True
    g = lambda lp, lab: -lp.gather(2, lab.unsqueeze(2)).squeeze(2) * slot_mask
    if reduction == "none":
        per = (sa_tok_loss.sum(1) + g(sa_len, len_lab).sum(1) + g(sa_syn, syn_lab).sum(1) + na_tok_loss.sum(1) + g(na_len, len_lab).sum(1)
               + g(na_syn, syn_lab).sum(1)) / tok_mask.sum(1)
        return per, None
    denom = tok_mask.sum()
    parts = [g(sa_len, len_lab).sum() / denom, sa_tok_loss.sum() / denom, g(sa_syn, syn_lab).sum() / denom,
             g(na_len, len_lab).sum() / denom, na_tok_loss.sum() / denom, g(na_syn, syn_lab).sum() / denom]
    loss = sum(parts)
    if self_dis:
        kl = torch.nn.functional.kl_div(na_tok, sa_tok.exp().detach(), reduction="none") * tok_mask.unsqueeze(2)
        loss = loss + kl.sum() / denom
    return loss, parts


# ----------------------------------------------------------------------------- self-critical losses (a16)
def new_self_critical(logprobs, seq, scores, sample_n: int):
    """StructureLosses.forward with structure_loss_type 'new_self_critical', reduction 'mean'
    (captioning/modules/losses.py:37-51, 70, 157-176; entropy_reward_weight 0, self_cider_reward_weight 0).
    ``scores``: [N] from the caption scorer (get_scores, external).  Returns (loss, reward [B, n] = the raw scores,
    as the reference stores them in out['reward'] before the baseline is subtracted)."""
    mask = (seq > 0).to(logprobs)
    mask = torch.cat([mask.new_full((mask.size(0), 1), 1), mask[:, :-1]], 1)        # losses.py:47-48
    sc = torch.as_tensor(scores).type_as(logprobs).view(-1, sample_n)                 # :50-51
    picked = logprobs.gather(2, seq.unsqueeze(2)).squeeze(2)                          # :70
    baseline = (sc.sum(1, keepdim=True) - sc) / (sc.shape[1] - 1)                     # :164
    adv = sc - baseline
    output = -picked * mask * adv.view(-1, 1)                                         # :172
    return torch.sum(output) / torch.sum(mask), sc                                    # :176


STRUCTURE_LOSS_TYPES = ("seqnll", "risk", "max_margin", "multi_margin", "softmax_margin", "real_softmax_margin", "new_self_critical")


def structure_loss(loss_type: str, input, seq, scores, sample_n: int, reduction: str = "mean", entropy_reward_weight: float = 0.0):
    """StructureLosses.forward for every ``structure_loss_type`` (captioning/modules/losses.py:38-179; self_cider_reward_weight 0).
    ``input``: [N, S, V] logits or log-softmax as the type expects; ``scores`` [N] from the caption scorer (get_scores, external).
    Returns (loss, reward [B, n] = the raw scores, stored before entropy / rescaling / baseline touch them, :51-52)."""
    if loss_type not in STRUCTURE_LOSS_TYPES:
        raise ValueError(loss_type)
    F = torch.nn.functional
    mask = (seq > 0).to(input)
    mask = torch.cat([mask.new_full((mask.size(0), 1), 1), mask[:, :-1]], 1)        # :47-48
    sc = torch.as_tensor(scores).type_as(input).view(-1, sample_n)                    # :50-51
    reward = sc
    if entropy_reward_weight > 0:                                                     # :53-57
        entropy = -(F.softmax(input, dim=2) * F.log_softmax(input, dim=2)).sum(2).detach()
        entropy = (entropy * mask).sum(1) / mask.sum(1)
        sc = sc + entropy_reward_weight * entropy.view(-1, sample_n)
    costs = -sc                                                                       # :59
    if loss_type in ("risk", "softmax_margin"):                                       # :60-62: rescaled to [0, 1] per image
        costs = costs - costs.min(1, keepdim=True)[0]
        costs = costs / costs.max(1, keepdim=True)[0]
    x = input.gather(2, seq.unsqueeze(2)).squeeze(2)                                  # :70
    if loss_type == "new_self_critical":                                              # :157-176
        adv = sc - (sc.sum(1, keepdim=True) - sc) / (sc.shape[1] - 1)
        out = -x * mask * adv.view(-1, 1)
        if reduction == "none":
            return out.sum(1) / mask.sum(1), reward
        return torch.sum(out) / torch.sum(mask), reward
    x = x * mask
    if loss_type == "risk":                                                           # :81-87: caption log-prob, not averaged
        x = x.sum(1).view(-1, sample_n)
        assert reduction == "mean"
        return (F.softmax(x.exp(), dim=1) * costs).sum(1).mean(), reward            # (the implicit dim of a 2-D softmax is 1)
    x = (x.sum(1) / mask.sum(1)).view(-1, sample_n)                                   # every other type: mean token value per caption
    if loss_type == "seqnll":                                                         # :72-79
        return F.cross_entropy(x, costs.min(1)[1], reduction=reduction), reward
    if loss_type in ("max_margin", "multi_margin"):                                   # :96-128
        costs_star, idx = costs.min(1, keepdim=True)
        hinge = F.relu(costs - costs_star - x.gather(1, idx) + x)
        assert reduction == "mean"
        return (hinge.max(1)[0] / 2).mean() if loss_type == "max_margin" else hinge.mean(), reward
    return F.cross_entropy(x + costs, costs.min(1)[1], reduction=reduction), reward  # softmax_margin :136-144, real_softmax_margin :146-155


def rl_kl_term(naic_logprobs, saic_logprobs, saic_seq):
    """LossWrapper UIC branch with rl_kl (captioning/modules/loss_wrapper.py:216-222): KL(SAIC || NAIC) per vocabulary
    entry, nn.KLDivLoss(reduction='none') = target * (log target - input), masked by the SAIC caption's tokens."""
    mask = saic_seq > 0
    target = torch.exp(saic_logprobs).detach()
    kl = torch.where(target > 0, target * (target.log() - naic_logprobs), torch.zeros_like(target))    # xlogy convention of KLDivLoss
    return torch.sum(kl * mask.unsqueeze(2)) / (torch.sum(mask) + 1e-6)


def loss_wrapper_uic_rl(saic_logprobs, saic_seq, naic_logprobs, naic_seq, saic_scores, naic_scores, sample_n: int,
                        structure_loss_weight: float = 1.0, lm_loss=0.0, rl_kl: bool = False):
    """LossWrapper.forward, train_mode 'UIC', struc_flag (captioning/modules/loss_wrapper.py:181-230): the sum of the two
    modes' mixed losses (+ the KL term).  Returns the dict entries 'loss', 'struc_loss', 'reward'."""
    ls, rs = new_self_critical(saic_logprobs, saic_seq, saic_scores, sample_n)
    ln, rn = new_self_critical(naic_logprobs, naic_seq, naic_scores, sample_n)
    loss = ((1 - structure_loss_weight) * lm_loss + structure_loss_weight * ls) + ((1 - structure_loss_weight) * lm_loss + structure_loss_weight * ln)
    if rl_kl:
        loss = loss + rl_kl_term(naic_logprobs, saic_logprobs, saic_seq)
    return dict(loss=loss, struc_loss=ls + ln, reward=rs + rn)
