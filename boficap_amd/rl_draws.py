"""The draw pass of the self-critical step with the reference's estimator (loss_wrapper.py:193-209 samples in train mode with the tape running
and differentiates that same pass): every token of both branches is drawn from the TRAINING forward's rows, phrase by phrase.  One process for both of its
callers -- ``loss_wrapper.reference_estimator_pass`` (LossWrapper) and ``XETrainer._rl_reference_step`` (rl_step) --, which own the training forward (eager or
as captured graphs), its seed, the scorer, the gradient pass and the optimiser."""
from dataclasses import dataclass

import torch

from . import hip, xe


@dataclass
class Draws:
    """What ``draw_pass`` drew.  ``seq_*`` int64 [N, S] ids, ``drawn_*`` float32 [N, S] their log-probs under the rows they were drawn from, ``mask_*`` bool
    [N, S] the drawn positions (s: semi-autoregressive, n: non-autoregressive branch); ``out`` the engine's last semi-autoregressive dict (phrase_num /
    phrase_length / phrase_syn of the finished layout), ``naic`` the non-autoregressive layout per sample, ``prep`` the index tensors of the finished
    captions (what the gradient pass reads), ``passes`` the training forwards spent."""
    seq_s: torch.Tensor
    seq_n: torch.Tensor
    drawn_s: torch.Tensor
    drawn_n: torch.Tensor
    mask_s: torch.Tensor
    mask_n: torch.Tensor
    out: dict
    naic: dict
    prep: dict
    passes: int


def prepared(cfg, layout: dict) -> dict:
    """The index tensors ``xe.sampled_logprobs_prepared`` reads for a ``layout`` of ``draw_pass``: the device collate of the semi-autoregressive captions
    so far (one launch) beside the non-autoregressive branch's (made once per step)."""
    prep = xe.rl_prepare_saic_device(cfg, layout["seq"], layout["phrase_length"], layout["phrase_syn"])
    prep["na_syn"], prep["na_klen"] = layout["na_syn"], layout["na_klen"]
    return prep


def picked(lp, seq):
    """float32 [N, S]: the log-probs ``lp`` [N, S, V] gives the ids ``seq``, off the tape."""
    return lp.detach().float().gather(2, seq[..., None]).squeeze(2)


def drawn_gap(picked_s, picked_n, d: Draws) -> float:
    """``reference_gap``: max |gradient pass's log-prob - drawn row's| at the drawn tokens of both branches (0.0: the pass differentiates the rows drawn from)."""
    g_s, g_n = (picked_s - d.drawn_s)[d.mask_s], (picked_n - d.drawn_n)[d.mask_n]
    return max(float(g_s.abs().max()) if g_s.numel() else 0.0, float(g_n.abs().max()) if g_n.numel() else 0.0)


@torch.no_grad()
def naic_layout(model, att_feats, att_masks, sample_n: int):
    """What ``draw_pass`` starts from, made before any training forward: the non-autoregressive slot layout (the engine's bounding loop: greedy heads, one
    layout per image, no gradient reaches it in the reference either) repeated per sample, and the features and region counts repeated likewise for the
    semi-autoregressive loop -> (layout dict, features [N, R, F], region counts [N] or None).  A function of its own because a trainer issues it AHEAD of its step's
    first launches (dropout step word, zero-grad, the weights' transposes): behind them the step measured 0.3 ms slower (profiles/r15_rl_draw_pass_ab.txt)."""
    eng = model.engine()
    feats_in, lens_in = model._as_input(att_feats), model._att_len(att_masks)
    N = feats_in.size(0) * sample_n
    if N > model.max_batch:
        raise hip.BofiHipError(f"{N} sampled rows exceed bofi_max_batch={model.max_batch}")
    r = eng.decode_naic(feats_in, lens_in, strict_q1=model.strict_reference)
    na = {k: r[k].repeat_interleave(sample_n, dim=0).contiguous() for k in ("phrase_num", "phrase_length", "phrase_syn")}
    feats_rep = feats_in.repeat_interleave(sample_n, dim=0).contiguous()
    lens_rep = None if lens_in is None else lens_in.repeat_interleave(sample_n).contiguous()
    return na, feats_rep, lens_rep


@torch.no_grad()
def draw_pass(model, laid, temperature: float, rows, draw_base: int) -> Draws:
    """Draw the captions of both modes on ``laid`` (``naic_layout``'s result) from the rows of ``rows(layout, first) -> (lp_saic, lp_naic)``: the caller's
    tape-free training forward of the captions so far -- ``layout`` = {seq, phrase_length, phrase_syn, na_syn, na_klen} (``prepared`` collates it), ``first``:
    the step's first forward (the one that runs the encoder).

      * non-autoregressive branch: the words of every laid-out slot are drawn from the first forward's fill rows;
      * semi-autoregressive branch: the engine's loop runs ONE iteration per call (bofi_call_opts_t.saic_it_begin / saic_it_end, layout only): its bounding step lays the next
        phrase out on the words so far (TransformerModel.py:1903-1948), ``rows`` gives that phrase's rows, its words are drawn from them and handed back to
        the engine (bofi_engine_saic_put_words), whose next bounding step reads them -- core_SAIC's own process (:1903-1984) with the training pass's fill
        distribution.
    A draw is one sample per slot from Categorical(logits = row / temperature) (CaptionModel.py:405-425) by the library's one-pass Gumbel-max sampler
    (bofi_vocab_sample: counter-hash uniforms, a NaN log-prob counts as -10), kept at the positions of the phrases it is for (bofi_rl_take_draws: ids, their
    log-probs under the rows, the drawn mask): no index list, no host synchronisation, two launches.  Draw d (1, 2, ...: phrase 1, the non-autoregressive
    branch, phrase 2, ...) uses the seed (draw_base + d) mod 2^64.
    What stays different from the reference: the bound heads decide on the engine (no dropout in the bounding steps); they are argmax decisions without gradient."""
    cfg, eng = model.cfg, model.engine()
    na, feats_rep, lens_rep = laid
    N, S, dev = feats_rep.size(0), cfg.seq_length, feats_rep.device
    draws = 0

    def draw(lp, plen, p0, p1, seq, drawn, mask):
        nonlocal draws
        lpf = lp if lp.dtype == torch.float32 and lp.is_contiguous() else lp.float().contiguous()
        n_, s_, V = lpf.shape
        tok = torch.empty(n_, s_, dtype=torch.int64, device=dev)
        draws += 1
        hip.check(hip.lib().bofi_vocab_sample(hip.ptr(lpf), n_ * s_, V, s_, 1, float(temperature), (draw_base + draws) & 0xFFFFFFFFFFFFFFFF, None, cfg.pad_idx,
                                              hip.ptr(tok), hip.stream_ptr()), "bofi_vocab_sample")
        hip.check(hip.lib().bofi_rl_take_draws(hip.ptr(lpf), hip.ptr(tok), hip.ptr(plen), n_, s_, V, int(p0), int(p1), hip.ptr(seq), hip.ptr(drawn), hip.ptr(mask),
                                               hip.stream_ptr()), "bofi_rl_take_draws")

    pos = torch.arange(S, device=dev)[None]
    layout = xe.rl_prepare_naic_device(cfg, na["phrase_length"], na["phrase_syn"], strict_q1=model.strict_reference)
    seq_s = layout["seq"] = torch.zeros(N, S, dtype=torch.int64, device=dev)
    seq_n = na["seq"] = torch.zeros(N, S, dtype=torch.int64, device=dev)
    drawn_s, drawn_n = torch.zeros(N, S, device=dev), torch.zeros(N, S, device=dev)
    mask_s = torch.zeros(N, S, dtype=torch.bool, device=dev)
    mask_n = pos < na["phrase_length"].long().sum(1)[:, None]
    na_plen = na["phrase_length"].to(torch.int32).contiguous()
    out, passes = None, 0
    for it in range(1, S + 1):
        # (the engine lays the next phrase out on the words so far and stops: the words are drawn here, from the training forward's rows)
        out = eng.decode_saic(feats_rep, lens_rep, it_range=(it, it), out=out, want_logprob=False, layout_only=True)
        layout["phrase_length"], layout["phrase_syn"] = out["phrase_length"], out["phrase_syn"]
        if int(out["bound_iters"]) < it:                          # no caption was open in this iteration: the loop is through
            break
        lp_s, lp_n = rows(layout, passes == 0)
        passes += 1
        draw(lp_s, out["phrase_length"], it - 1, it, seq_s, drawn_s, mask_s)           # phrase `it`'s positions
        eng.saic_put_words(seq_s)
        if it == 1:
            draw(lp_n, na_plen, 0, S, seq_n, drawn_n, None)                          # every laid-out position of the non-autoregressive branch
    return Draws(seq_s, seq_n, drawn_s, drawn_n, mask_s, mask_n, out, na, prepared(cfg, layout), passes)
