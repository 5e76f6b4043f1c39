"""Python handle on the C++/HIP decode engine (``bofi_engine_*`` in include/boficap_hip.h).

One engine = one model replica's packed weights + workspace in the HBM of the current device.
PyTorch is only used here to own device buffers and to name the HIP stream.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np
import torch

from . import hip
from .config import BofiConfig


def pick_concurrent_streams(n: int, device=None, candidates: int = 16, spin_cycles: int = 400_000, priorities=None):
    """``n`` HIP streams that really run side by side.

    ROCm multiplexes streams onto a few hardware queues and two streams on one queue serialise; which
    stream lands where depends on creation order.  Instead of guessing, time a spin kernel on pairs of
    candidate streams and keep a set whose members pairwise overlap.  Falls back to fewer streams than
    asked for if no such set exists (the caller then keeps fewer decodes in flight)."""
    import time
    dev = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
    with torch.cuda.device(dev):
        # (priorities: experiment -- candidate i is created with priorities[i % len]; 0 = default, -1 = high)
        cands = [torch.cuda.Stream(device=dev) if not priorities else torch.cuda.Stream(device=dev, priority=int(priorities[i % len(priorities)])) for i in range(candidates)]

        def span(streams):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for st in streams:
                with torch.cuda.stream(st):
                    torch.cuda._sleep(spin_cycles)
            torch.cuda.synchronize(dev)
            return time.perf_counter() - t0

        span(cands[:1])
        one = min(span(cands[:1]) for _ in range(3))
        chosen = [cands[0]]
        for c in cands[1:]:
            if len(chosen) >= n:
                break
            if all(min(span([c, s]) for _ in range(2)) < 1.5 * one for s in chosen):
                chosen.append(c)
    return chosen


def pick_stream_beside(main, device=None, candidates: int = 12, spin_cycles: int = 400_000):
    """A new HIP stream that really runs BESIDE ``main`` (same probe as pick_concurrent_streams: a freshly created stream may share main's
    hardware queue -- which one it gets depends on how many streams the process has made before -- and then serialises behind it).  Falls back
    to the last candidate if none overlaps."""
    import time
    dev = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
    with torch.cuda.device(dev):
        def span(streams):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for st in streams:
                with torch.cuda.stream(st):
                    torch.cuda._sleep(spin_cycles)
            torch.cuda.synchronize(dev)
            return time.perf_counter() - t0

        span([main])
        one = min(span([main]) for _ in range(3))
        cand = None
        for _ in range(candidates):
            cand = torch.cuda.Stream(device=dev)
            if min(span([main, cand]) for _ in range(2)) < 1.5 * one:
                return cand
    return cand


ATT_EMBED_W = "att_embed.0.weight"


DIVERSE_KEYS = ("diverse_seq", "diverse_logp", "diverse_aug", "diverse_count")      # what decode_naic(diverse=N) adds to its dict (bofi_vocab_diverse's four outputs)


class BofiEngine:
    def __init__(self, cfg: BofiConfig, dtype: torch.dtype = torch.bfloat16, max_batch: int = 64,
                 max_regions: int = 36, device: Optional[torch.device] = None):
        cfg.validate()
        if cfg.d_k != 64:
            raise hip.BofiHipError("the HIP attention kernel is specialised for head dim 64 (d_model / num_att_heads)")
        if not torch.cuda.is_available():
            raise hip.BofiHipError("no HIP device: the decode engine has no CPU fallback")
        self.cfg = cfg
        self.dtype = dtype
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self.max_batch, self.max_regions = max_batch, max_regions
        self._lib = hip.lib()
        c = hip.BofiConfigC(
            vocab=cfg.tgt_vocab, feat=cfg.att_feat_padded, d_model=cfg.d_model, d_ff=cfg.d_ff, heads=cfg.h,
            n_enc=cfg.N_enc, n_dec=cfg.N_dec, seq_length=cfg.seq_length, pad_idx=cfg.pad_idx, bos_idx=cfg.bos_idx,
            eos_idx=cfg.eos_idx, len_idx=cfg.len_idx, head_hidden=cfg.head_hidden, max_batch=max_batch,
            max_regions=max_regions, dtype={torch.float32: hip.DT_F32, torch.bfloat16: hip.DT_BF16}[dtype], n_len=cfg.N_len)
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            hip.check(self._lib.bofi_engine_create(C.byref(c), C.byref(self._h)), "bofi_engine_create")
        self._finalized = False
        self._live_word = None

    def fork(self, max_batch: Optional[int] = None, ids_only: bool = False) -> "BofiEngine":
        """A second engine sharing this one's weights with its own workspace (one per in-flight batch); ``max_batch``: images per call the fork's
        workspace is sized for (default: this engine's) -- a pipeline that coalesces several loader batches per call forks larger.
        ``ids_only``: a workspace without the two vocabulary-wide float32 buffers (most of a fork's memory) -- such a fork serves ``decode_naic(ids_only=True)``
        launches that take the fused generator and refuses everything else (BOFI_FORK_IDS_ONLY)."""
        if not self._finalized:
            raise hip.BofiHipError("fork() needs loaded weights")
        f = object.__new__(BofiEngine)
        f.cfg, f.dtype, f.device, f.max_batch, f.max_regions = self.cfg, self.dtype, self.device, int(max_batch or self.max_batch), self.max_regions
        f._lib, f._finalized, f._parent = self._lib, True, getattr(self, "_parent", self)        # keeps the weights' owner alive
        f._live_word = None                                           # (the parent's watch_live_iterations word is not the fork's)
        f._kv_beside = getattr(self, "_kv_beside", 1)                 # (the form switch of set_bound_kv_beside is inherited: bofi_engine_fork copies it)
        f._h = C.c_void_p()
        with torch.cuda.device(self.device):
            hip.check(self._lib.bofi_engine_fork_ex(self._h, int(max_batch or 0), hip.FORK_IDS_ONLY if ids_only else 0, C.byref(f._h)), "bofi_engine_fork_ex")
        return f

    def stream(self) -> "torch.cuda.Stream":
        """The engine's own HIP stream wrapped for torch (one hardware queue per in-flight engine)."""
        return torch.cuda.ExternalStream(self._lib.bofi_engine_stream(self._h), device=self.device)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                self._lib.bofi_engine_destroy(h)
            except Exception:
                pass

    # ---------------------------------------------------------------- weights
    def load_state_dict(self, sd: Dict[str, object]) -> None:
        """``sd``: reference-schema state dict (torch tensors on any device, or numpy arrays)."""
        F, Fp = self.cfg.att_feat_size, self.cfg.att_feat_padded
        for name, v in sd.items():
            a = v.detach().to("cpu", torch.float32).contiguous().numpy() if torch.is_tensor(v) else np.ascontiguousarray(v, np.float32)
            if name == ATT_EMBED_W and Fp != F:                  # the engine's K dimension is the padded width: zero columns beyond att_feat_size
                if a.shape != (self.cfg.d_model, F):
                    raise hip.BofiHipError(f"{name}: [{self.cfg.d_model}, {F}] expected, got {a.shape}")
                a = np.ascontiguousarray(np.pad(a, ((0, 0), (0, Fp - F))))
            hip.check(self._lib.bofi_engine_set_weight(self._h, name.encode(), a.ctypes.data_as(C.c_void_p), a.size),
                      f"set_weight({name})")
        with torch.cuda.device(self.device):
            hip.check(self._lib.bofi_engine_finalize(self._h), "bofi_engine_finalize")
        self._finalized = True
        self._weights_changed()

    def refresh_from_device(self, named: Dict[str, torch.Tensor]) -> None:
        """Re-pack the weights from float32 tensors on the device (e.g. ``dict(model.named_parameters())``): kernels only,
        existing allocations, captured graphs and forks stay valid (``bofi_engine_refresh_device``)."""
        if not self._finalized:
            raise hip.BofiHipError("the first load goes through load_state_dict")
        items = [(k, v) for k, v in named.items() if k != "model.pos_embed.pe"]
        F, Fp = self.cfg.att_feat_size, self.cfg.att_feat_padded
        if Fp != F:                                              # att_embed's weight goes through this engine's padded float32 copy (zero columns beyond att_feat_size)
            for i, (k, v) in enumerate(items):
                if k == ATT_EMBED_W:
                    if not v.is_cuda or v.dtype != torch.float32 or tuple(v.shape) != (self.cfg.d_model, F):
                        raise hip.BofiHipError(f"{k}: float32 [{self.cfg.d_model}, {F}] on the HIP device expected")
                    pad = getattr(self, "_att_w_padded", None)
                    if pad is None or pad.device != v.device:
                        pad = self._att_w_padded = torch.zeros(self.cfg.d_model, Fp, dtype=torch.float32, device=v.device)
                    pad[:, :F].copy_(v.detach())
                    items[i] = (k, pad)
        # (a training loop refreshes after every optimiser step with the same tensors: the checked argument arrays are kept per set of addresses)
        # (the key holds everything the check looks at: the caching allocator hands addresses out again -- tensors of another dtype, size or name at
        # the same addresses must not ride on an old validation)
        key = tuple((k, v.data_ptr(), v.numel(), v.dtype, v.is_cuda, v.is_contiguous()) for k, v in items)
        cached = getattr(self, "_refresh_args", None)
        if cached is None or cached[0] != key:
            for k, v in items:
                if not v.is_cuda or v.dtype != torch.float32 or not v.is_contiguous():
                    raise hip.BofiHipError(f"{k}: contiguous float32 tensor on the HIP device expected")
            n = len(items)
            cached = self._refresh_args = (key, n, (C.c_char_p * n)(*[k.encode() for k, _ in items]), (C.c_void_p * n)(*[v.data_ptr() for _, v in items]),
                                           (C.c_int64 * n)(*[v.numel() for _, v in items]))
        _, n, names, ptrs, numels = cached
        with torch.cuda.device(self.device):
            hip.check(self._lib.bofi_engine_refresh_device(self._h, n, names, ptrs, numels, hip.stream_ptr()), "bofi_engine_refresh_device")
        self._weights_changed()

    def _weights_changed(self):
        if getattr(self, "_loop_mode_sticky", False):            # (a fallback taken because the OLD weights' fp16 copies were clamped: the new ones get their own verdict)
            self._loop_mode_sticky = False
            self.set_bound_loop(-1)

    # ---------------------------------------------------------------- calls
    def pad_feats(self, att_feats: torch.Tensor) -> torch.Tensor:
        """Dense [B, R, att_feat_size] features zero-padded with torch to the engine's [B, R, att_feat_padded] (plumbing, not the hot path: the box launch
        of csrc/regions.hip writes the padded width itself); anything else -- and every tensor when att_feat_size % 64 == 0 -- is returned as it is."""
        F, Fp = self.cfg.att_feat_size, self.cfg.att_feat_padded
        if Fp == F or att_feats.dim() != 3 or att_feats.size(2) != F:
            return att_feats
        return torch.nn.functional.pad(att_feats, (0, Fp - F))

    def _check_feats(self, att_feats, att_len):
        if att_feats.dim() != 3 or att_feats.size(2) != self.cfg.att_feat_padded:
            raise hip.BofiHipError(f"att_feats must be [B, R, {self.cfg.att_feat_padded}], got {tuple(att_feats.shape)}" + (
                "" if self.cfg.att_feat_padded == self.cfg.att_feat_size else f" (att_feat_size {self.cfg.att_feat_size} zero-padded to a multiple of 64: pad_feats)"))
        if not att_feats.is_cuda or not att_feats.is_contiguous():
            raise hip.BofiHipError("att_feats must be a contiguous tensor on the HIP device")
        if att_len is not None and (att_len.dtype != torch.int32 or not att_len.is_cuda or att_len.numel() != att_feats.size(0)):
            raise hip.BofiHipError("att_len must be an int32 device tensor of B elements")

    def decode_naic(self, att_feats: torch.Tensor, att_len: Optional[torch.Tensor] = None, *, strict_q1: bool = True,
                    want_logprob: bool = True, want_memory: bool = False, raw_logits: bool = False, graph: bool = False,
                    refine_rounds: int = 0, out: Optional[dict] = None, q1_group: int = 0, iter_cap: int = 0, phases: str = "", row_stats: bool = False,
                    ids_only: bool = False, refine_method: str = "feed_back", attn_topk: int = 0, attn_maps: bool = False, attn_heads: bool = False,
                    attn_layer: int = -1, ban_ids=None, no_repeat: bool = False, repeat_min_id: int = 7, block_trigrams: bool = False, require_ids=None,
                    nbest: Optional[int] = None, nbest_no_repeat: bool = False, require_phrases=None, require_any=None, diverse: Optional[int] = None,
                    diversity_lambda: float = 0.5, diverse_no_repeat: bool = False) -> dict:
        """Greedy NAIC bound+fill decode.  Returns a dict of device tensors: seq [B,S] int64,
        seq_logprob [B,S,V] float32 (or None), phrase_num [B] int32, phrase_length [B,S] int32,
        phrase_syn [B,S] int64, bound_iters [1] int32, memory [B,R,d] float32 (or None).
        Pass the previous result as ``out`` to reuse its buffers (required for graph replay).
        ``refine_rounds`` extra filling passes feed the previous ids back as decoder input (BASELINE config 5).
        ``q1_group`` > 0: the call carries B / q1_group independent batches (dynamic batching); quirk Q1 applies per batch,
        so each batch's outputs equal its own separate decode.
        ``iter_cap`` > 0 (the five-launch bounding iterations only; the persistent loop kernel -- ``bound_loop_active(R)`` -- ends by itself, ignores the
        budget and its result is always complete): enqueue that many bounding iterations instead of seq_length (bofi_call_opts_t.bound_iter_cap); the result is
        then the reference's iff ``bound_iters`` < iter_cap afterwards -- the caller checks and decodes again without the cap otherwise.
        ``phases``: "" = the whole decode; a subset of "ebf" = only the encode / bounding loop / filling pass + export of it (BOFI_FLAG_PHASE_*): a pipelining
        caller enqueues the three on the same engine in that order (its streams / events order them) with the same arguments.
        ``row_stats``: the vocabulary epilogue also leaves, per position, sum_v p log p and the log-prob of the emitted id in ``out['row_plogp']`` / ``out['row_chosen']``
        (float32 [B, S]; bofi_call_opts_t.row_plogp / row_chosen) -- what ``row_stats(out)`` / ``entropy_perplexity(out)`` otherwise read back out of the log-prob tensor.
        ``ids_only`` (BOFI_FLAG_IDS_ONLY; implies ``want_logprob=False``, not with ``raw_logits``): the distribution is not wanted at all -- ids, layout and ``row_stats``
        only.  Where the row-block generator runs, generator and vocabulary epilogue are then one launch that writes no logits; the ids are the first maxima of the
        raw logits.  ``row_stats(out)`` / ``sample_tokens(out)`` of such a result need ``row_stats=True`` / are not available: there is no distribution to read.
        ``refine_method``: what the ``refine_rounds`` extra passes are.  'feed_back' (default): all of the previous ids as decoder input.  'mask_predict'
        (BOFI_FLAG_MASK_PREDICT; ``refine_rounds`` >= 1, not with ``raw_logits``): pass t re-predicts the n (T + 1 - t) / (T + 1) least confident of an image's n
        positions from BOS and keeps the rest; ``out['refine_round']`` (int32 [B, S]) names the pass that emitted each token, ``row_stats`` are those of the
        emitting pass, and ``seq_logprob`` is the LAST pass's tensor (kept positions' rows are its re-prediction, not the distribution that emitted the token).
        ``attn_topk`` / ``attn_maps`` / ``attn_heads`` / ``attn_layer`` (bofi_call_opts_t.attn_*; one extra launch in the filling pass): the word-to-region attention of
        decoder layer ``attn_layer`` (-1: the last) -- ``out['attn']`` float32 [B, S, R], the heads' mean cross-attention probabilities per position (what the reference
        keeps as ``decoder.layers[-1].src_attn.attn``, averaged over heads); ``out['attn_heads']`` [B, H, S, R]; ``out['attn_top']`` int32 / ``out['attn_top_w']``
        float32 [B, S, K]: each position's K heaviest regions in descending order (-1 / 0 past an image's region count and on positions that carry no word).  With
        refinement rounds the maps are the LAST pass's (under 'mask_predict' a kept position's row is that pass's re-prediction, as ``seq_logprob``).
        ``ban_ids`` / ``no_repeat`` / ``repeat_min_id`` (bofi_call_opts_t.pick_*; bofi_vocab_constrain's two small launches behind every filling pass's vocabulary epilogue): the
        ids of ``ban_ids`` are never emitted, and with ``no_repeat`` no position repeats the word (an id >= ``repeat_min_id``; 7 is the first word id) of the position before it
        -- each live position takes the best id the two rules leave.  Feed-back rounds feed the constrained ids back; ``seq`` and ``row_chosen`` are those of the emitted ids;
        ``out['constrained']`` (int32 [B]) counts the positions the last pass's constrained pick changed.  Not with ``ids_only`` or ``refine_method='mask_predict'``.  An empty
        ``ban_ids`` without ``no_repeat`` is the plain decode: nothing is launched.
        ``block_trigrams`` (BOFI_FLAG_PICK_TRIGRAMS; bofi_vocab_pick's two launches in place of bofi_vocab_constrain's): in addition no word trigram (three ids >=
        ``repeat_min_id``) stands twice in a caption -- a position whose two predecessors repeat an earlier bigram does not take the id that followed it there (the
        reference's --block_trigrams as a hard block).  On by itself it turns the constrained pick on; ``ban_ids`` must then leave at least seq_length + 1 ids.
        ``require_ids`` (bofi_vocab_require: one small launch on the same stream BEHIND the decode call, outside a ``graph`` replay; no field of the call record): ids every
        caption must contain -- an int table [B, K] with -1 padding (a device tensor is passed through as it is: the kernel classifies every entry), a list of per-image id
        lists, or one flat list for every image; on the host: ids in 0..V-1, at most 8 per image, none of them in ``ban_ids``.  The words are placed on the live positions
        where they cost the least log-prob (first as many as can be placed, then the largest total of log p(word) - log p(id standing there); the header states the rule
        and its tie-break), read from ``seq_logprob`` (the engine's own workspace without it), under the call's ``ban_ids`` / ``no_repeat`` / ``repeat_min_id``: a
        placement never creates an adjacent repeat.  ``out['required_pos']`` int32 [B, K]: each word's position, -1 padding, -2 skipped (by the kernel: banned, out of
        range, repeated), -3 not placeable; ``out['required_moved']`` int32 [B]: positions whose id changed; ``seq`` and, with ``row_stats``, ``row_chosen`` are those of
        the emitted ids.  With feed-back refinement rounds the placement applies to the LAST pass only: earlier passes are fed the unforced ids.  In the phased form it
        follows the call whose ``phases`` contain 'f'.  Not with ``ids_only`` (no distribution), ``refine_method='mask_predict'`` or ``block_trigrams`` (a placement
        could create a blocked trigram).  None, an empty list or rows of -1 only: nothing is launched and no key is added.
        ``require_phrases`` (bofi_vocab_require_units in place of bofi_vocab_require: same placement behind the call, same keys, same refusals; not together with
        ``require_ids`` -- give one): multi-word UNITS every caption must contain, the ids of a unit side by side and in order -- per image a list of units, each a list of
        1..4 ids, or one flat list of units for every image (``hip.require_unit_table`` states the forms and what it refuses: among it, under ``no_repeat``, a unit that
        repeats a word and two units that could meet at a shared word); a device tensor int32 [B, K, L] with -1 padding is passed through as it is.  Each unit goes to the
        contiguous span where it costs the least log-prob (first as many units as can be placed, then the largest total gain; the header states the rule).
        ``out['required_pos']`` int32 [B, K] then holds each unit's START position (-1, -2, -3 as above).
        ``require_any`` (bofi_vocab_require_any in their place: same placement behind the call, same refusals; not together with ``require_ids`` or ``require_phrases``
        -- give one): required ALTERNATIVES -- per image a list of GROUPS, each a list of 1..4 alternatives, each a list of 1..4 ids ("dog", "dogs" or "puppy"), or one
        flat list of groups for every image (``hip.require_any_table`` states the forms and what it refuses: among it an alternative given twice and, under ``no_repeat``,
        two alternatives of different groups that could meet at a shared word); a device tensor int32 [B, K, A, L] with -1 padding is passed through as it is.  A group
        is satisfied by ANY ONE of its alternatives: the placement takes, per group, the alternative and the span that cost the least (first as many groups as can be
        satisfied, then the largest total gain; the header states the rule).  ``out['required_pos']`` int32 [B, K] holds the start of each group's placed alternative
        (-1 no alternative given, -2 all skipped, -3 not placeable), ``out['required_alt']`` int32 [B, K] that alternative's index in its group (-1: not placed),
        ``out['required_moved']`` as above.
        ``nbest`` = N in 1..8 (bofi_vocab_nbest: two small launches on the same stream BEHIND the decode call, outside a ``graph`` replay; no field of the call record):
        the N most probable captions of the last filling pass, exactly -- the pass scores every position on its own, so a caption's log-prob is a sum of per-position
        terms and a width-N merge over each row's N best ids finds the N best captions (the header states the rule, its tie order and what holds under ties).  Read
        from ``seq_logprob`` (the engine's own workspace without it; raw logits serve: the totals are then sums of logits), under the call's ``ban_ids``.
        ``out['nbest_seq']`` int64 [B, N, S] (pad_idx past an image's length and past its count), ``out['nbest_logp']`` float64 [B, N] (non-increasing; -inf past
        the count), ``out['nbest_count']`` int32 [B].  Entry 0 is the call's own ``seq`` on a NaN-free decode.  With feed-back rounds the list is the final pass's.
        Refused before anything is enqueued: ``ids_only`` or an ids-only fork (there are no rows), ``refine_method='mask_predict'`` (kept positions do not hold their
        row's first id), ``no_repeat`` / ``block_trigrams`` (a rule that couples neighbours needs per-last-id state: a width-N list is no longer exact) and
        ``require_ids``.  None or 0: nothing is launched and no key is added.
        ``nbest_no_repeat`` (with ``nbest`` = N in 1..6; a BofiHipError without it): the list is of the captions with NO ADJACENT REPEATED WORD -- an id >=
        ``repeat_min_id`` never follows itself -- exactly: bofi_vocab_nbest_norepeat, a list-Viterbi over each row's N + 2 best ids, in place of bofi_vocab_nbest, under the
        call's ``ban_ids`` and ``repeat_min_id``; same placement, same keys.  ``nbest_count`` may then be 0, and entry 0 need not be ``seq``: the decode's own outputs stay
        the plain decode's (``no_repeat=True``, the constrained decode, stays refused with the list).
        ``diverse`` = N in 1..8 (bofi_vocab_diverse: two small launches BEHIND the decode call, placed as ``nbest``'s and read from the same rows, under the call's
        ``ban_ids``): a Hamming-diverse SET of N captions of the last filling pass -- the reference's diverse beam search ('dbs', one beam per group) where it is no
        search: the groups are decoded one after another, group g is the exact maximiser of the sum of its positions' log-probs minus ``diversity_lambda`` (finite,
        >= 0; the reference's default 0.5) times the number of earlier groups that have the same id at the same position (the header states the rule and its ties).
        ``out['diverse_seq']`` int64 [B, N, S], ``out['diverse_logp']`` float64 [B, N] (each caption's own log-prob, comparable to ``nbest_logp``; not ordered),
        ``out['diverse_aug']`` float64 [B, N] (the maximised value), ``out['diverse_count']`` int32 [B] (N; 1 for a degenerate image).  Group 0 is the call's own
        ``seq``, which stays untouched.  ``diverse_no_repeat`` (with ``diverse`` = N in 1..6; a BofiHipError without it): every caption of the set is free of adjacent
        repeated words under the call's ``repeat_min_id`` -- a Viterbi over each row's N + 2 best ids; group 0 need then not be ``seq`` and ``diverse_count`` may be 0.
        Refused before anything is enqueued, naming ``diverse``: ``ids_only`` or an ids-only fork, ``refine_method='mask_predict'``, ``no_repeat`` /
        ``block_trigrams`` on the decode, any ``require_*`` option, ``nbest`` in the same call, N or lambda out of range.  None or 0: nothing is launched, no key."""
        mp = self._refine_flag(refine_method, refine_rounds, raw_logits)
        ban, pick_on, req, nbest, nb_min, dv = self._post_options(
            ban_ids, no_repeat, repeat_min_id, block_trigrams, require_ids, nbest, nbest_no_repeat, att_feats.size(0), ids_only, mp,
            want_logprob or (out is not None and out.get("seq_logprob") is not None), require_phrases, require_any, diverse, diversity_lambda, diverse_no_repeat)
        if ids_only:
            if raw_logits:
                raise hip.BofiHipError("ids_only: the raw logits are not produced")
            if out is not None and out.get("seq_logprob") is not None:
                raise hip.BofiHipError("ids_only: `out` carries a seq_logprob buffer")
            want_logprob = False
        self._check_feats(att_feats, att_len)
        B, R, _ = att_feats.shape
        S, V, dev = self.cfg.seq_length, self.cfg.tgt_vocab, att_feats.device
        if out is None:
            out = dict(
                seq=torch.empty(B, S, dtype=torch.int64, device=dev),
                seq_logprob=torch.empty(B, S, V, dtype=torch.float32, device=dev) if want_logprob else None,
                phrase_num=torch.empty(B, dtype=torch.int32, device=dev),
                phrase_length=torch.empty(B, S, dtype=torch.int32, device=dev),
                phrase_syn=torch.empty(B, S, dtype=torch.int64, device=dev),
                bound_iters=torch.empty(1, dtype=torch.int32, device=dev),
                memory=torch.empty(B, R, self.cfg.d_model, dtype=torch.float32, device=dev) if want_memory else None)
        if out.get("bound_saturated") is None:                   # fp16 saturation status of this decode's bounding loop (bofi_call_opts_t.sat_out): see ``saturated``
            out["bound_saturated"] = torch.zeros(1, dtype=torch.int32, device=dev)
        o = hip.BofiCallOpts(q1_group=int(q1_group), bound_iter_cap=int(iter_cap), sat_out=out["bound_saturated"].data_ptr(),
                             live_max=None if self._live_word is None else self._live_word.data_ptr())
        if not 0 <= refine_rounds <= 15:
            raise hip.BofiHipError("refine_rounds must be in 0..15")
        if row_stats and raw_logits:
            raise hip.BofiHipError("row_stats: of log-probs, not of raw logits")
        if row_stats and "row_plogp" not in out:
            out["row_plogp"] = torch.empty(B, S, dtype=torch.float32, device=dev)
            out["row_chosen"] = torch.empty(B, S, dtype=torch.float32, device=dev)
        if row_stats:
            o.row_plogp, o.row_chosen = out["row_plogp"].data_ptr(), out["row_chosen"].data_ptr()
        out["_row_stats_fused"] = bool(row_stats)
        out["_ids_only"] = bool(ids_only)
        if mp and out.get("refine_round") is None:
            out["refine_round"] = torch.empty(B, S, dtype=torch.int32, device=dev)
        if mp:
            o.refine_round = out["refine_round"].data_ptr()
        self._attn_opts(o, out, B, R, dev, attn_topk, attn_maps, attn_heads, attn_layer)
        self._pick_opts(o, ban, no_repeat, repeat_min_id, block_trigrams)
        if pick_on and (out.get("constrained") is None or out["constrained"].numel() != B):
            out["constrained"] = torch.zeros(B, dtype=torch.int32, device=dev)
        flags = ((hip.FLAG_STRICT_Q1 if strict_q1 else 0) | (hip.FLAG_RAW_LOGITS if raw_logits else 0) | (hip.FLAG_GRAPH if graph else 0)
                 | (refine_rounds << hip.FLAG_REFINE_SHIFT) | (hip.FLAG_IDS_ONLY if ids_only else 0) | mp | (hip.FLAG_PICK_TRIGRAMS if block_trigrams else 0))
        if phases:
            if set(phases) - set("ebf"):
                raise hip.BofiHipError("phases: a subset of 'ebf'")
            flags |= ((hip.FLAG_PHASE_ENCODE if "e" in phases else 0) | (hip.FLAG_PHASE_BOUND if "b" in phases else 0) | (hip.FLAG_PHASE_FILL if "f" in phases else 0))
        hip.check(self._lib.bofi_engine_decode_naic(
            self._h, hip.ptr(att_feats), hip.dtype_code(att_feats), hip.ptr(att_len), B, R, flags, hip.ptr(out["seq"]),
            hip.ptr(out["seq_logprob"]), hip.ptr(out["phrase_num"]), hip.ptr(out["phrase_length"]), hip.ptr(out["phrase_syn"]),
            hip.ptr(out["memory"]), hip.ptr(out["bound_iters"]), C.byref(o), hip.stream_ptr()), "bofi_engine_decode_naic")
        if req is None:
            out.pop("required_pos", None), out.pop("required_moved", None)      # (a reused `out` of a call that had the option)
        if req is None or req.dim() != 4:
            out.pop("required_alt", None)
        if not nbest:
            out.pop("nbest_seq", None), out.pop("nbest_logp", None), out.pop("nbest_count", None)      # (a reused `out` of a call that had the option)
        if dv is None:
            for k in DIVERSE_KEYS:
                out.pop(k, None)                                 # (a reused `out` of a call that had the option)
        if not phases or "f" in phases:
            self._post_passes(out, B, out["seq"], out["seq_logprob"], lambda: torch.sum(out["phrase_length"], 1, dtype=torch.int32), 0, ban, pick_on, req, nbest, nb_min,
                              no_repeat, repeat_min_id, out["row_chosen"] if row_stats else None, dv)
        return out

    def _post_options(self, ban_ids, no_repeat, repeat_min_id, block_trigrams, require_ids, nbest, nbest_no_repeat, B: int, ids_only, mp: int, own_rows: bool,
                      require_phrases=None, require_any=None, diverse=None, diversity_lambda=0.5, diverse_no_repeat=False):
        """The options of ``decode_naic`` / ``fill_naic`` whose work follows the call, resolved and refused before anything is enqueued: (ban, pick_on, req, nbest, nb_min, dv)
        -- the device bit table or None, "the constrained pick is on", the device table of required words ([B, K]), units ([B, K, L]) or alternatives ([B, K, A, L]) or None, the list's width (0: off) and the ``repeat_min_id``
        of a repeat-free list (None: the plain list), and the diverse set's (N, lambda, no_repeat, repeat_min_id) or None (``_diverse_options``).  ``ids_only`` None: the entry point has no such form (``fill_naic``; its pick refusal comes first, in its own words)."""
        ban = self._pick_ban(ban_ids, block_trigrams)
        pick_on = ban is not None or bool(no_repeat) or bool(block_trigrams)
        if ids_only is None and pick_on and mp:
            raise hip.BofiHipError("ban_ids / no_repeat / block_trigrams: not with refine_method='mask_predict'")
        req = self._require_table(require_ids, B, ban_ids)
        if req is not None:
            self._require_refusals(bool(ids_only), mp, block_trigrams)
        units = self._require_unit_table(require_phrases, B, ban_ids, no_repeat, repeat_min_id)
        if units is not None:
            if req is not None:
                raise hip.BofiHipError("require_ids and require_phrases: give one (single ids are units of length 1)")
            self._require_refusals(bool(ids_only), mp, block_trigrams, "require_phrases")
            req = units
        alts = self._require_any_table(require_any, B, ban_ids, no_repeat, repeat_min_id)
        if alts is not None:
            if req is not None:
                raise hip.BofiHipError("require_ids / require_phrases and require_any: give one (a word or a unit is a group of one alternative)")
            self._require_refusals(bool(ids_only), mp, block_trigrams, "require_any")
            req = alts
        nbest = self._nbest_width(nbest)
        nb_min = self._nbest_no_repeat(nbest, nbest_no_repeat, repeat_min_id)
        if nbest:
            self._nbest_refusals(bool(ids_only), mp, no_repeat, block_trigrams, req is not None, own_rows)
        dv = self._diverse_options(diverse, diversity_lambda, diverse_no_repeat, repeat_min_id)
        if dv is not None:
            self._diverse_refusals(bool(ids_only), mp, no_repeat, block_trigrams, req is not None, bool(nbest), own_rows)
        if ids_only is not None and pick_on and (ids_only or mp):
            raise hip.BofiHipError("ban_ids / no_repeat / block_trigrams: not with ids_only (no distribution to re-pick from) or refine_method='mask_predict'")
        return ban, pick_on, req, nbest, nb_min, dv

    def _post_passes(self, target: dict, B: int, seq, lp, ntok, ntok_bias: int, ban, pick_on: bool, req, nbest: int, nb_min, no_repeat, repeat_min_id, row_chosen,
                     dv=None) -> None:
        """Enqueue what follows a filling pass on the current stream, results into ``target`` (its buffers are reused when they fit): the constrained pick's count
        (bofi_engine_pick_changed), the required words (``_require_place``), the N-best list (``_nbest_list``), the diverse set (``_diverse_set``).  ``ntok()`` gives the images' lengths where one is needed."""
        if pick_on:
            if target.get("constrained") is None or target["constrained"].numel() != B:
                target["constrained"] = torch.zeros(B, dtype=torch.int32, device=seq.device)
            hip.check(self._lib.bofi_engine_pick_changed(self._h, hip.ptr(target["constrained"]), B, hip.stream_ptr()), "bofi_engine_pick_changed")
        if req is not None and req.dim() == 4:
            target["required_pos"], target["required_alt"], target["required_moved"] = self._require_any_place(
                req, seq, lp, ntok(), ntok_bias, ban, no_repeat, repeat_min_id, row_chosen, target.get("required_pos"), target.get("required_alt"),
                target.get("required_moved"))
        elif req is not None:
            target["required_pos"], target["required_moved"] = self._require_place(
                req, seq, lp, ntok(), ntok_bias, ban, no_repeat, repeat_min_id, row_chosen, target.get("required_pos"), target.get("required_moved"))
        if nbest:
            target["nbest_seq"], target["nbest_logp"], target["nbest_count"] = self._nbest_list(
                nbest, B, lp, ntok(), ntok_bias, ban, target.get("nbest_seq"), target.get("nbest_logp"), target.get("nbest_count"), repeat_min=nb_min)
        if dv is not None:
            target.update(zip(DIVERSE_KEYS, self._diverse_set(dv, B, lp, ntok(), ntok_bias, ban, *(target.get(k) for k in DIVERSE_KEYS))))

    @staticmethod
    def _diverse_options(diverse, diversity_lambda=0.5, diverse_no_repeat=False, repeat_min_id: int = 7):
        """``diverse`` / ``diversity_lambda`` / ``diverse_no_repeat`` of a decode: None when off (``diverse`` None or 0), else (N, lambda, no_repeat, repeat_min_id).
        BofiHipError naming ``diverse``: N outside 1..8 (1..6 with ``diverse_no_repeat``), a lambda that is negative, NaN or infinite, a negative ``repeat_min_id``
        under the repeat rule, ``diverse_no_repeat`` without ``diverse``."""
        if diverse is None or diverse is False or int(diverse) == 0:
            if diverse_no_repeat:
                raise hip.BofiHipError("diverse_no_repeat: needs diverse = N (it keeps adjacent repeats out of the diverse set; no_repeat=True is the constrained decode)")
            return None
        N, lam = hip.diverse_check(diverse, diversity_lambda, bool(diverse_no_repeat), repeat_min_id, "diverse")
        return N, lam, bool(diverse_no_repeat), int(repeat_min_id) if diverse_no_repeat else 0

    def _diverse_refusals(self, ids_only: bool, mp: int, no_repeat: bool, block_trigrams: bool, required: bool, nbest: bool, own_rows: bool) -> None:
        if ids_only:
            raise hip.BofiHipError("diverse: not with ids_only (the decode leaves no rows to decode the groups from)")
        if mp:
            raise hip.BofiHipError("diverse: not with refine_method='mask_predict' (kept positions do not hold their row's first id: group 0 would not be the caption)")
        if no_repeat or block_trigrams:
            raise hip.BofiHipError("diverse: not with no_repeat / block_trigrams (the set stands beside the plain decode); diverse_no_repeat=True keeps adjacent "
                                   "repeats out of the set")
        if required:
            raise hip.BofiHipError("diverse: not with require_ids / require_phrases / require_any (the set is of unforced captions)")
        if nbest:
            raise hip.BofiHipError("diverse: not with nbest in the same call (two sets of captions of one pass: ask for one)")
        if not own_rows and not self._lib.bofi_engine_logprob(self._h):
            raise hip.BofiHipError("diverse: this engine keeps no log-prob workspace (an ids-only fork): there are no rows to decode the groups from")

    def _diverse_set(self, dv, B: int, lp, ntok, ntok_bias, ban, seq_n=None, total=None, aug=None, count=None):
        """Enqueue bofi_vocab_diverse for ``dv`` (``_diverse_options``) on the current stream behind a decode; ``lp`` as ``_nbest_list``'s.  Returns (seq_n int64
        [B, N, S], total float64 [B, N], aug float64 [B, N], count int32 [B]); the buffers given are reused when they fit."""
        N, lam, nr, lo = dv
        S, V, dev = self.cfg.seq_length, self.cfg.tgt_vocab, ntok.device
        if seq_n is None or tuple(seq_n.shape) != (B, N, S):
            seq_n = torch.empty(B, N, S, dtype=torch.int64, device=dev)
        if total is None or tuple(total.shape) != (B, N):
            total = torch.empty(B, N, dtype=torch.float64, device=dev)
        if aug is None or tuple(aug.shape) != (B, N):
            aug = torch.empty(B, N, dtype=torch.float64, device=dev)
        if count is None or count.numel() != B:
            count = torch.empty(B, dtype=torch.int32, device=dev)
        need = int(self._lib.bofi_vocab_nbest_workspace(B * S))
        work = getattr(self, "_nbest_work", None)
        if work is None or work.numel() * 4 < need or work.device != dev:
            work = self._nbest_work = torch.empty(max(1, need // 4), dtype=torch.int32, device=dev)
        src = hip.ptr(lp) if lp is not None else self._lib.bofi_engine_logprob(self._h)
        if not src:
            raise hip.BofiHipError("diverse: this engine keeps no log-prob workspace (an ids-only fork)")
        hip.check(self._lib.bofi_vocab_diverse(src, V, B * S, V, S, hip.ptr(ntok), int(ntok_bias), int(self.cfg.pad_idx), hip.ptr(ban), N, lam, int(nr), lo, hip.ptr(seq_n),
                                               hip.ptr(total), hip.ptr(aug), hip.ptr(count), hip.ptr(work), work.numel() * 4, hip.stream_ptr()), "bofi_vocab_diverse")
        return seq_n, total, aug, count

    @staticmethod
    def _nbest_width(nbest) -> int:
        """``nbest`` of a decode as N, 0 when off (None or 0); BofiHipError outside 1..8."""
        if nbest is None or nbest is False:
            return 0
        n = int(nbest)
        if n != 0 and not 1 <= n <= hip.NBEST_MAX:
            raise hip.BofiHipError(f"nbest: N must lie in 1..{hip.NBEST_MAX} (0 / None: off), got {n}")
        return n

    @staticmethod
    def _nbest_no_repeat(nbest: int, nbest_no_repeat, repeat_min_id: int = 7) -> Optional[int]:
        """``nbest_no_repeat`` of a decode whose list width is ``nbest`` (0: off): None when the option is off, else the ``repeat_min_id`` the list is made under.
        BofiHipError without ``nbest``, with N > 6 or a negative ``repeat_min_id``."""
        if not nbest_no_repeat:
            return None
        if not nbest:
            raise hip.BofiHipError("nbest_no_repeat: needs nbest = N (it narrows the N-best list; no_repeat=True is the constrained decode)")
        if nbest > hip.NBEST_NR_MAX:
            raise hip.BofiHipError(f"nbest_no_repeat: N must lie in 1..{hip.NBEST_NR_MAX} (the list needs N + 2 of a row's 8 candidate ids), got {nbest}")
        if int(repeat_min_id) < 0:
            raise hip.BofiHipError(f"nbest_no_repeat: repeat_min_id must be >= 0, got {repeat_min_id}")
        return int(repeat_min_id)

    def _nbest_refusals(self, ids_only: bool, mp: int, no_repeat: bool, block_trigrams: bool, required: bool, own_rows: bool) -> None:
        if ids_only:
            raise hip.BofiHipError("nbest: not with ids_only (the decode leaves no rows to list from)")
        if mp:
            raise hip.BofiHipError("nbest: not with refine_method='mask_predict' (kept positions do not hold their row's first id: entry 0 would not be the caption)")
        if no_repeat or block_trigrams:
            raise hip.BofiHipError("nbest: not with no_repeat / block_trigrams (the N best under a rule that couples neighbours need per-last-id state: "
                                   "a width-N list is no longer exact); nbest_no_repeat=True lists the repeat-free captions beside the plain decode")
        if required:
            raise hip.BofiHipError("nbest: not with require_ids / require_phrases / require_any (the list is of unforced captions)")
        if not own_rows and not self._lib.bofi_engine_logprob(self._h):
            raise hip.BofiHipError("nbest: this engine keeps no log-prob workspace (an ids-only fork): there are no rows to list from")

    def _nbest_list(self, N: int, B: int, lp, ntok, ntok_bias, ban, seq_n=None, total=None, count=None, repeat_min: Optional[int] = None):
        """Enqueue bofi_vocab_nbest -- with ``repeat_min`` (``_nbest_no_repeat``) bofi_vocab_nbest_norepeat under that ``repeat_min_id`` -- on the current stream behind a
        decode: ``lp`` the decode's log-prob (or logit) tensor or None for the engine's own workspace.
        Returns (seq_n int64 [B, N, S], total float64 [B, N], count int32 [B]); the buffers given are reused when they fit."""
        S, V, dev = self.cfg.seq_length, self.cfg.tgt_vocab, ntok.device
        if seq_n is None or tuple(seq_n.shape) != (B, N, S):
            seq_n = torch.empty(B, N, S, dtype=torch.int64, device=dev)
        if total is None or tuple(total.shape) != (B, N):
            total = torch.empty(B, N, dtype=torch.float64, device=dev)
        if count is None or count.numel() != B:
            count = torch.empty(B, dtype=torch.int32, device=dev)
        need = int(self._lib.bofi_vocab_nbest_workspace(B * S))
        work = getattr(self, "_nbest_work", None)
        if work is None or work.numel() * 4 < need or work.device != dev:
            work = self._nbest_work = torch.empty(max(1, need // 4), dtype=torch.int32, device=dev)
        src = hip.ptr(lp) if lp is not None else self._lib.bofi_engine_logprob(self._h)
        if not src:
            raise hip.BofiHipError("nbest: this engine keeps no log-prob workspace (an ids-only fork)")
        if repeat_min is not None:
            hip.check(self._lib.bofi_vocab_nbest_norepeat(src, V, B * S, V, S, hip.ptr(ntok), int(ntok_bias), int(self.cfg.pad_idx), hip.ptr(ban), int(repeat_min), N,
                                                          hip.ptr(seq_n), hip.ptr(total), hip.ptr(count), hip.ptr(work), work.numel() * 4, hip.stream_ptr()),
                      "bofi_vocab_nbest_norepeat")
            return seq_n, total, count
        hip.check(self._lib.bofi_vocab_nbest(src, V, B * S, V, S, hip.ptr(ntok), int(ntok_bias), int(self.cfg.pad_idx), hip.ptr(ban), N, hip.ptr(seq_n), hip.ptr(total),
                                             hip.ptr(count), hip.ptr(work), work.numel() * 4, hip.stream_ptr()), "bofi_vocab_nbest")
        return seq_n, total, count

    def _require_table(self, require_ids, B: int, ban_ids=None):
        """``require_ids`` of a decode as the device table int32 [B, K] of bofi_vocab_require, None when nothing is required.  Host input goes through
        ``hip.require_table`` (ids in 0..V-1, at most 8 per image, none in ``ban_ids``: BofiHipError otherwise); a device tensor is passed through -- the kernel is total."""
        if isinstance(require_ids, torch.Tensor) and require_ids.is_cuda:
            if require_ids.dim() != 2 or require_ids.size(0) != B or not 1 <= require_ids.size(1) <= hip.REQUIRE_MAX:
                raise hip.BofiHipError(f"require_ids: a device table is [B, K] with 1 <= K <= {hip.REQUIRE_MAX}, got {tuple(require_ids.shape)} for {B} images")
            return require_ids.to(torch.int32).contiguous()
        t = hip.require_table(require_ids, B, self.cfg.tgt_vocab, ban_ids or ())
        return None if t is None else t.to(self.device)

    def _require_unit_table(self, require_phrases, B: int, ban_ids=None, no_repeat: bool = False, repeat_min_id: int = 7):
        """``require_phrases`` of a decode as the device table int32 [B, K, L] of bofi_vocab_require_units, None when nothing is required.  Host input goes through
        ``hip.require_unit_table`` (BofiHipError for what it refuses); a device tensor is passed through -- the kernel is total."""
        if isinstance(require_phrases, torch.Tensor) and require_phrases.is_cuda:
            t = require_phrases
            if t.dim() != 3 or t.size(0) != B or not 1 <= t.size(1) <= hip.REQUIRE_MAX or not 1 <= t.size(2) <= hip.REQUIRE_UNIT_MAX:
                raise hip.BofiHipError(f"require_phrases: a device table is [B, K, L] with 1 <= K <= {hip.REQUIRE_MAX} and 1 <= L <= {hip.REQUIRE_UNIT_MAX}, "
                                       f"got {tuple(t.shape)} for {B} images")
            return t.to(torch.int32).contiguous()
        t = hip.require_unit_table(require_phrases, B, self.cfg.tgt_vocab, ban_ids or (), bool(no_repeat), int(repeat_min_id))
        return None if t is None else t.to(self.device)

    def _require_any_table(self, require_any, B: int, ban_ids=None, no_repeat: bool = False, repeat_min_id: int = 7):
        """``require_any`` of a decode as the device table int32 [B, K, A, L] of bofi_vocab_require_any, None when nothing is required.  Host input goes through
        ``hip.require_any_table`` (BofiHipError for what it refuses); a device tensor is passed through -- the kernel is total."""
        if isinstance(require_any, torch.Tensor) and require_any.is_cuda:
            t = require_any
            if (t.dim() != 4 or t.size(0) != B or not 1 <= t.size(1) <= hip.REQUIRE_MAX or not 1 <= t.size(2) <= hip.REQUIRE_ALT_MAX
                    or not 1 <= t.size(3) <= hip.REQUIRE_UNIT_MAX):
                raise hip.BofiHipError(f"require_any: a device table is [B, K, A, L] with 1 <= K <= {hip.REQUIRE_MAX}, 1 <= A <= {hip.REQUIRE_ALT_MAX} and "
                                       f"1 <= L <= {hip.REQUIRE_UNIT_MAX}, got {tuple(t.shape)} for {B} images")
            return t.to(torch.int32).contiguous()
        t = hip.require_any_table(require_any, B, self.cfg.tgt_vocab, ban_ids or (), bool(no_repeat), int(repeat_min_id))
        return None if t is None else t.to(self.device)

    @staticmethod
    def _require_refusals(ids_only: bool, mp: int, block_trigrams: bool, what: str = "require_ids") -> None:
        if ids_only:
            raise hip.BofiHipError(f"{what}: not with ids_only (no distribution to place the words by)")
        if mp:
            raise hip.BofiHipError(f"{what}: not with refine_method='mask_predict'")
        if block_trigrams:
            raise hip.BofiHipError(f"{what}: not with block_trigrams (a placement could create a blocked trigram)")

    def _require_place(self, req, seq, lp, ntok, ntok_bias, ban, no_repeat, repeat_min_id, row_chosen, pos=None, moved=None):
        """Enqueue bofi_vocab_require -- bofi_vocab_require_units for a unit table -- on the current stream behind a decode: ``req`` int32 [B, K] (words) or [B, K, L]
        (units) on the device, ``lp`` the decode's log-prob (or logit) tensor or None
        for the engine's own workspace.  Returns (pos int32 [B, K], moved int32 [B]); the buffers given are reused when they fit."""
        if int(repeat_min_id) < 0:
            raise hip.BofiHipError("repeat_min_id must be >= 0")
        B, K = req.shape[:2]
        S, V = self.cfg.seq_length, self.cfg.tgt_vocab
        if pos is None or tuple(pos.shape) != (B, K):
            pos = torch.empty(B, K, dtype=torch.int32, device=seq.device)
        if moved is None or moved.numel() != B:
            moved = torch.empty(B, dtype=torch.int32, device=seq.device)
        src = hip.ptr(lp) if lp is not None else self._lib.bofi_engine_logprob(self._h)
        if not src:
            raise hip.BofiHipError("require_ids / require_phrases: this engine keeps no log-prob workspace (an ids-only fork)")
        if req.dim() == 3:
            hip.check(self._lib.bofi_vocab_require_units(src, V, B * S, V, S, hip.ptr(ntok), int(ntok_bias), hip.ptr(req), K, req.size(2), hip.ptr(ban),
                                                         1 if no_repeat else 0, int(repeat_min_id), hip.ptr(seq), hip.ptr(row_chosen), hip.ptr(pos), hip.ptr(moved),
                                                         hip.stream_ptr()), "bofi_vocab_require_units")
            return pos, moved
        hip.check(self._lib.bofi_vocab_require(src, V, B * S, V, S, hip.ptr(ntok), int(ntok_bias), hip.ptr(req), K, hip.ptr(ban), 1 if no_repeat else 0,
                                               int(repeat_min_id), hip.ptr(seq), hip.ptr(row_chosen), hip.ptr(pos), hip.ptr(moved), hip.stream_ptr()),
                  "bofi_vocab_require")
        return pos, moved

    def _require_any_place(self, req, seq, lp, ntok, ntok_bias, ban, no_repeat, repeat_min_id, row_chosen, pos=None, which=None, moved=None):
        """Enqueue bofi_vocab_require_any on the current stream behind a decode: ``req`` int32 [B, K, A, L] on the device, the rest as ``_require_place``.  Returns (pos
        int32 [B, K], which int32 [B, K], moved int32 [B]); the buffers given are reused when they fit."""
        if int(repeat_min_id) < 0:
            raise hip.BofiHipError("repeat_min_id must be >= 0")
        B, K, A, L = req.shape
        S, V = self.cfg.seq_length, self.cfg.tgt_vocab
        if pos is None or tuple(pos.shape) != (B, K):
            pos = torch.empty(B, K, dtype=torch.int32, device=seq.device)
        if which is None or tuple(which.shape) != (B, K):
            which = torch.empty(B, K, dtype=torch.int32, device=seq.device)
        if moved is None or moved.numel() != B:
            moved = torch.empty(B, dtype=torch.int32, device=seq.device)
        src = hip.ptr(lp) if lp is not None else self._lib.bofi_engine_logprob(self._h)
        if not src:
            raise hip.BofiHipError("require_any: this engine keeps no log-prob workspace (an ids-only fork)")
        hip.check(self._lib.bofi_vocab_require_any(src, V, B * S, V, S, hip.ptr(ntok), int(ntok_bias), hip.ptr(req), K, A, L, hip.ptr(ban), 1 if no_repeat else 0,
                                                   int(repeat_min_id), hip.ptr(seq), hip.ptr(row_chosen), hip.ptr(pos), hip.ptr(which), hip.ptr(moved),
                                                   hip.stream_ptr()), "bofi_vocab_require_any")
        return pos, which, moved

    def _pick_ban(self, ban_ids, block_trigrams: bool = False):
        """The device bit table of a ban list (``hip.ban_bits``: ids outside 0..V-1 and a list that leaves fewer than two ids raise), kept per engine and id set;
        None for no list or an empty one.  With ``block_trigrams`` the list must leave at least seq_length + 1 ids (a position can find up to seq_length ids excluded)."""
        if ban_ids is None:
            return None
        key = tuple(sorted({int(i) for i in ban_ids}))
        if not key:
            return None
        if block_trigrams and self.cfg.tgt_vocab - len(key) < self.cfg.seq_length + 1:
            raise hip.BofiHipError(f"ban_ids: {len(key)} of {self.cfg.tgt_vocab} ids banned -- with block_trigrams at least seq_length + 1 = {self.cfg.seq_length + 1} must stay")
        cache = self.__dict__.setdefault("_ban_tables", {})
        if key not in cache:
            cache[key] = hip.ban_bits(key, self.cfg.tgt_vocab, self.device)
        return cache[key]

    @staticmethod
    def _pick_opts(o: "hip.BofiCallOpts", ban, no_repeat, repeat_min_id, block_trigrams=False) -> None:
        """The constrained pick of a call into its record ``o``; nothing is set when it is off (the record's zero tail).  (``block_trigrams`` itself travels as a call
        flag, BOFI_FLAG_PICK_TRIGRAMS; it reads ``repeat_min_id`` from the record.)"""
        if ban is None and not no_repeat and not block_trigrams:
            return
        if int(repeat_min_id) < 0:
            raise hip.BofiHipError("repeat_min_id must be >= 0")
        o.pick_ban = None if ban is None else ban.data_ptr()
        o.pick_no_repeat, o.pick_repeat_min_id = (1 if no_repeat else 0), int(repeat_min_id)

    def _attn_opts(self, o: "hip.BofiCallOpts", out: dict, B: int, R: int, dev, attn_topk: int, attn_maps: bool, attn_heads: bool, attn_layer: int) -> None:
        """The attention outputs of a call, into its record ``o``: buffers in ``out`` (made when missing or of another shape)."""
        if not (attn_topk or attn_maps or attn_heads):
            return                                               # (off: the usual call)
        K = int(attn_topk)
        if not 0 <= K <= 8:
            raise hip.BofiHipError("attn_topk must be in 0..8")
        if not -1 <= int(attn_layer) < self.cfg.N_dec:
            raise hip.BofiHipError(f"attn_layer must be in 0..{self.cfg.N_dec - 1}, or -1 for the last decoder layer")
        S, H = self.cfg.seq_length, self.cfg.h
        o.attn_layer, o.attn_topk = int(attn_layer), K
        for field, key, on, shape, dt in (("attn_mean", "attn", attn_maps, (B, S, R), torch.float32), ("attn_heads", "attn_heads", attn_heads, (B, H, S, R), torch.float32),
                                          ("attn_top_idx", "attn_top", K > 0, (B, S, K), torch.int32), ("attn_top_w", "attn_top_w", K > 0, (B, S, K), torch.float32)):
            if on and (out.get(key) is None or tuple(out[key].shape) != shape):
                out[key] = torch.empty(shape, dtype=dt, device=dev)
            if on:
                setattr(o, field, out[key].data_ptr())

    @staticmethod
    def _refine_flag(refine_method: str, refine_rounds: int, raw_logits: bool) -> int:
        """BOFI_FLAG_MASK_PREDICT or 0 for a ``refine_method``; what the library would refuse is refused here, with the Python names."""
        if refine_method not in ("feed_back", "mask_predict"):
            raise hip.BofiHipError(f"refine_method {refine_method!r}: 'feed_back' or 'mask_predict'")
        if refine_method == "feed_back":
            return 0
        if not 1 <= refine_rounds <= 15:
            raise hip.BofiHipError("refine_method='mask_predict' needs refine_rounds in 1..15")
        if raw_logits:
            raise hip.BofiHipError("refine_method='mask_predict' ranks log-probs: not with raw logits (output_logsoftmax=0)")
        return hip.FLAG_MASK_PREDICT

    def set_decodes_in_flight(self, n: int) -> None:
        """A hint for the kernel choice (bofi_engine_set_decodes_in_flight): 1 = this engine's launches run alone on the device (shorter
        workgroup chains), 0 / > 1 = throughput forms (fewer weight bytes per row).  Part of the graph key: a captured launch is replayed under the hint it was captured with."""
        hip.check(self._lib.bofi_engine_set_decodes_in_flight(self._h, int(n)), "bofi_engine_set_decodes_in_flight")

    def ids_only_fused(self, B: int) -> bool:
        """Would ``decode_naic(ids_only=True)`` of B images take the fused generator -- what a ``fork(ids_only=True)`` can serve (bofi_engine_ids_only_fused)?"""
        return bool(self._lib.bofi_engine_ids_only_fused(self._h, int(B)))

    def bound_loop_active(self, R: int) -> bool:
        """Does a decode of R regions per image run the bounding loop as the persistent per-16-image kernel (bofi_engine_bound_loop_active)?"""
        return bool(self._lib.bofi_engine_bound_loop_active(self._h, int(R)))

    def set_bound_loop(self, mode: int) -> None:
        """The bounding loop's form for this engine's following decodes (bofi_engine_set_bound_loop): -1 = BOFI_BOUND_LOOP and the decodes-in-flight hint decide,
        0 = the five-launch bf16 iterations, 2 = the persistent fp16 loop kernel whatever the hint."""
        hip.check(self._lib.bofi_engine_set_bound_loop(self._h, int(mode)), "bofi_engine_set_bound_loop")
        self._loop_mode = int(mode)

    def set_bound_kv_beside(self, mode: int) -> None:
        """Where the decoder layers' cross K|V are projected (bofi_engine_set_bound_kv_beside): 1 (default) = beside the bounding loop, in extra workgroups of the loop
        kernel's launch, wherever ``bound_kv_beside_active`` says so; 0 = never (all of the stacked K|V in front of the loop).  Part of the graph key; forks made afterwards inherit it."""
        hip.check(self._lib.bofi_engine_set_bound_kv_beside(self._h, int(mode)), "bofi_engine_set_bound_kv_beside")
        self._kv_beside = int(mode)

    def bound_kv_beside_active(self, B: int, R: int, phases: str = "") -> bool:
        """Would a ``decode_naic`` of B images of R regions (``phases`` as there) project the decoder layers' cross K|V beside the bounding loop (bofi_engine_bound_kv_beside_active)?"""
        flags = (hip.FLAG_PHASE_ENCODE if "e" in phases else 0) | (hip.FLAG_PHASE_BOUND if "b" in phases else 0) | (hip.FLAG_PHASE_FILL if "f" in phases else 0)
        return bool(self._lib.bofi_engine_bound_kv_beside_active(self._h, int(B), int(R), flags))

    def saturated(self, out: dict) -> int:
        """fp16 saturation status of the decode that produced ``out`` (a device -> host read: call it where the caller synchronises anyway): 0 = clean; bit 0 = the
        persistent bounding-loop kernel clamped an activation to +-65 504 on its way into an fp16 MFMA operand; bit 1 = its fp16 weight copies were clamped when they
        were packed; bit 2 = a pair of workgroups that share a group's feed-forward weights lost its exchange (a safety net: never seen).  Either way the slot layout may differ from what bf16 operands (float32's exponent range) give: decode again under ``set_bound_loop(0)``
        -- ``decode_naic_checked`` does both."""
        w = out.get("bound_saturated")
        return int(w) if w is not None else 0

    def decode_naic_checked(self, att_feats, att_len=None, **kw) -> dict:
        """``decode_naic`` + the saturation check + the fallback: when the loop kernel reports a clamp, a warning is issued and the batch is decoded again
        with the five-launch bf16 bounding iterations; a clamp of the WEIGHT copies (bit 1) keeps this engine on that form until its weights change.  Synchronises (reads one word)."""
        r = self.decode_naic(att_feats, att_len, **kw)
        sat = self.saturated(r)
        if sat:
            r = self._redo_without_loop_kernel(sat, lambda: self.decode_naic(att_feats, att_len, **dict(kw, out=r)))
        return r

    def _redo_without_loop_kernel(self, sat: int, decode):
        import warnings
        what = ("clamped its weight copies to +-65 504 (a bounding layer outside fp16's range)" if sat & 2 else
                "clamped an activation to +-65 504 (a bounding layer outside fp16's range)" if sat & 1 else
                "lost a partner workgroup of a pair (exchange timed out: status bit 2)")
        warnings.warn("boficap_amd: the fp16 bounding-loop kernel " + what + "; this decode is repeated with the five-launch bf16 iterations" +
                      (" and the engine stays on them until its weights change" if sat & 2 else ""), RuntimeWarning, stacklevel=3)
        before = getattr(self, "_loop_mode", -1)
        self.set_bound_loop(0)
        try:
            r = decode()
        finally:
            if not sat & 2:
                self.set_bound_loop(before)
            else:
                self._loop_mode_sticky = True
        return r

    def watch_live_iterations(self, word: Optional[torch.Tensor]) -> None:
        """``word`` (int32 [1] on the device, or None to stop): every following decode_naic folds its live-iteration count into it by atomic
        max -- a pipeline of capped decodes (``iter_cap``) is verified with ONE read after the last of them (clear the word first)."""
        if word is not None and (word.dtype != torch.int32 or word.numel() != 1 or not word.is_cuda):
            raise hip.BofiHipError("watch_live_iterations: an int32 [1] device tensor")
        self._live_word = word                                  # (kept alive; decode_naic hands it to every call: bofi_call_opts_t.live_max)

    def row_stats(self, out: dict):
        """(sum_v p log p, log-prob of the emitted id) per position, float32 [B, S] each, of the decode that produced ``out`` --
        from its seq_logprob tensor, or from the engine's own workspace when that was not materialised."""
        seq = out["seq"]
        B, S = seq.shape
        if out.get("_row_stats_fused"):                          # the decode's own epilogue left them (decode_naic(row_stats=True))
            return out["row_plogp"], out["row_chosen"]
        if out.get("_ids_only"):
            raise hip.BofiHipError("an ids_only decode leaves no distribution: ask it for row_stats=True")
        lp = out.get("seq_logprob")
        src = hip.ptr(lp) if lp is not None else self._lib.bofi_engine_logprob(self._h)
        plogp = torch.empty(B, S, dtype=torch.float32, device=seq.device)
        chosen = torch.empty(B, S, dtype=torch.float32, device=seq.device)
        hip.check(self._lib.bofi_vocab_stats(src, hip.ptr(seq), B * S, self.cfg.tgt_vocab, hip.ptr(plogp), hip.ptr(chosen), hip.stream_ptr()),
                  "bofi_vocab_stats")
        return plogp, chosen

    def entropy_perplexity(self, out: dict, vocab_lower: int = 0):
        """Per-image entropy and perplexity exactly as eval computes them (captioning/utils/eval_utils.py:463-464)."""
        plogp, chosen = self.row_stats(out)
        denom = (out["seq"] > vocab_lower).to(torch.float32).sum(1) + 1
        return -plogp.sum(1) / denom, -chosen.sum(1) / denom

    def sample_tokens(self, out: dict, n: int = 1, temperature: float = 1.0, seed: int = 0) -> torch.Tensor:
        """``n`` sampled captions per image on the slot layout of ``out`` (sample_method 'sample', CaptionModel.py:405-425):
        int64 [B * n, S], image b's draws in rows b*n .. b*n+n-1."""
        seq = out["seq"]
        B, S = seq.shape
        if out.get("_ids_only"):
            raise hip.BofiHipError("an ids_only decode leaves no distribution to sample from")
        lp = out.get("seq_logprob")
        src = hip.ptr(lp) if lp is not None else self._lib.bofi_engine_logprob(self._h)
        ntok = out["phrase_length"].sum(1).to(torch.int32).contiguous()
        res = torch.empty(B * n, S, dtype=torch.int64, device=seq.device)
        hip.check(self._lib.bofi_vocab_sample(src, B * S, self.cfg.tgt_vocab, S, n, float(temperature), seed & 0xFFFFFFFFFFFFFFFF, hip.ptr(ntok),
                                              self.cfg.pad_idx, hip.ptr(res), hip.stream_ptr()), "bofi_vocab_sample")
        return res

    def decode_saic(self, att_feats: torch.Tensor, att_len: Optional[torch.Tensor] = None, *, raw_logits: bool = False,
                    want_logprob: bool = True, sample: Optional[tuple] = None, graph: bool = False, out: Optional[dict] = None,
                    it_range: Optional[tuple] = None, layout_only: bool = False, nbest: Optional[int] = None, diverse: Optional[int] = None) -> dict:
        """Semi-autoregressive decode (core_SAIC), greedy or -- ``sample=(temperature, seed)`` -- with every phrase's tokens
        drawn from Categorical(logits / temperature) (the bound heads stay greedy, as in the reference).  Same result
        layout as ``decode_naic``.  ``graph``: the launch sequence is captured once per argument set and replayed (pass the
        previous result as ``out`` and keep the inputs in place); the sampling seed is read from device memory, so replays
        draw anew.  ``it_range`` = (first, last) iterations of the loop (bofi_call_opts_t.saic_it_begin / saic_it_end): (1, c) enqueues c iterations,
        (c + 1, S) with the same arguments and ``out`` continues that decode where it stopped -- together the whole loop, exactly;
        ``out["bound_iters"]`` (live iterations so far) < c says the first part was all of it.  ``layout_only``: the enqueued iterations lay their phrases out and stop
        (BOFI_FLAG_SAIC_LAYOUT_ONLY: no decoder pass, no tokens) -- for a caller that draws the words itself and hands them back with ``saic_put_words``.
        ``nbest`` is refused here: a phrase's rows are conditioned on the phrases before it, so a caption's log-prob is no sum of independent per-position terms."""
        if diverse:
            raise hip.BofiHipError("diverse: not with decode_saic (a phrase's rows depend on the phrases before it: the per-position sums are not a caption's log-prob)")
        if self._nbest_width(nbest):
            raise hip.BofiHipError("nbest: not with decode_saic (a phrase's rows depend on the phrases before it: the per-position sums are not a caption's log-prob); "
                                   "decode_naic / fill_naic serve it")
        self._check_feats(att_feats, att_len)
        B, R, _ = att_feats.shape
        S, V, dev = self.cfg.seq_length, self.cfg.tgt_vocab, att_feats.device
        if it_range is not None and (out is None and it_range[0] > 1):
            raise hip.BofiHipError("a continued semi-autoregressive decode needs the first part's `out`")
        if out is None:
            out = dict(
                seq=torch.empty(B, S, dtype=torch.int64, device=dev),
                seq_logprob=torch.empty(B, S, V, dtype=torch.float32, device=dev) if want_logprob else None,
                phrase_num=torch.empty(B, dtype=torch.int32, device=dev),
                phrase_length=torch.empty(B, S, dtype=torch.int32, device=dev),
                phrase_syn=torch.empty(B, S, dtype=torch.int64, device=dev),
                bound_iters=torch.empty(1, dtype=torch.int32, device=dev), memory=None)
        flags = (hip.FLAG_RAW_LOGITS if raw_logits else 0) | (hip.FLAG_GRAPH if graph else 0) | (hip.FLAG_SAIC_LAYOUT_ONLY if layout_only else 0)
        first, last = it_range if it_range is not None else (1, 0)
        o = hip.BofiCallOpts(saic_it_begin=int(first), saic_it_end=int(last) if last < S else 0)
        if sample is not None:
            o.sample_temperature, o.sample_seed = float(sample[0]), int(sample[1]) & 0xFFFFFFFFFFFFFFFF
            flags |= hip.FLAG_SAMPLE
        hip.check(self._lib.bofi_engine_decode_saic(
            self._h, hip.ptr(att_feats), hip.dtype_code(att_feats), hip.ptr(att_len), B, R, flags,
            hip.ptr(out["seq"]), hip.ptr(out["seq_logprob"]), hip.ptr(out["phrase_num"]), hip.ptr(out["phrase_length"]),
            hip.ptr(out["phrase_syn"]), hip.ptr(out["bound_iters"]), C.byref(o), hip.stream_ptr()), "bofi_engine_decode_saic")
        return out

    def saic_put_words(self, seq: torch.Tensor) -> None:
        """Between two partial ``decode_saic`` calls (``it_range``): replace the tokens emitted so far by ``seq`` (int64 [B, S], the layout of
        ``out["seq"]``) -- the loop continues on the caller's words (bofi_engine_saic_put_words)."""
        if seq.dtype != torch.int64 or seq.dim() != 2 or seq.size(1) != self.cfg.seq_length or not seq.is_cuda or not seq.is_contiguous():
            raise hip.BofiHipError("saic_put_words: contiguous int64 [B, seq_length] on the device")
        hip.check(self._lib.bofi_engine_saic_put_words(self._h, hip.ptr(seq), int(seq.size(0)), hip.stream_ptr()), "bofi_engine_saic_put_words")

    def encode(self, att_feats: torch.Tensor, att_len: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Encoder output (float32 [B, R, d]); also leaves memory + cross K/V in the engine workspace."""
        self._check_feats(att_feats, att_len)
        B, R, _ = att_feats.shape
        mem = torch.empty(B, R, self.cfg.d_model, dtype=torch.float32, device=att_feats.device)
        hip.check(self._lib.bofi_engine_encode(self._h, hip.ptr(att_feats), hip.dtype_code(att_feats), hip.ptr(att_len), B, R,
                                               hip.ptr(mem), hip.stream_ptr()), "bofi_engine_encode")
        return mem

    def bound_step(self, ext_syn: torch.Tensor, last: torch.Tensor, R: int, att_len: Optional[torch.Tensor] = None):
        """One bounding step on the memory of the preceding ``encode``: (len_logp [B,20], syn_logp [B,10])."""
        B = ext_syn.size(0)
        if ext_syn.dtype != torch.int32 or last.dtype != torch.int32 or ext_syn.size(1) != self.cfg.bound_len:
            raise hip.BofiHipError("ext_syn must be int32 [B, S+2] and last int32 [B]")
        llp = torch.empty(B, 20, dtype=torch.float32, device=ext_syn.device)
        slp = torch.empty(B, 10, dtype=torch.float32, device=ext_syn.device)
        hip.check(self._lib.bofi_engine_bound_step(self._h, hip.ptr(ext_syn.contiguous()), hip.ptr(last.contiguous()), B, R,
                                                   hip.ptr(att_len), hip.ptr(llp), hip.ptr(slp), hip.stream_ptr()), "bofi_engine_bound_step")
        return llp, slp

    def fill_naic(self, ext_syn: torch.Tensor, last: torch.Tensor, R: int, att_len: Optional[torch.Tensor] = None, *, strict_q1: bool = True,
                  raw_logits: bool = False, refine_rounds: int = 0, refine_method: str = "feed_back", attn_topk: int = 0, attn_maps: bool = False,
                  attn_heads: bool = False, attn_layer: int = -1, ban_ids=None, no_repeat: bool = False, repeat_min_id: int = 7, block_trigrams: bool = False,
                  require_ids=None, nbest: Optional[int] = None, nbest_no_repeat: bool = False, require_phrases=None, require_any=None,
                  diverse: Optional[int] = None, diversity_lambda: float = 0.5, diverse_no_repeat: bool = False):
        """The filling pass alone on a given slot layout (``ext_syn`` int32 [B, S+2], ``last`` int32 [B]) and the memory of the
        preceding ``encode``: (seq int64 [B, S], seq_logprob float32 [B, S, V]); with ``refine_method='mask_predict'`` (as ``decode_naic``) a third
        element, refine_round int32 [B, S].  With ``attn_topk`` / ``attn_maps`` / ``attn_heads`` (as ``decode_naic``) a last element, a dict of the attention tensors
        ('attn', 'attn_heads', 'attn_top', 'attn_top_w': those asked for).  ``ban_ids`` / ``no_repeat`` / ``repeat_min_id`` / ``block_trigrams`` as ``decode_naic``: that dict (the last element)
        then carries 'constrained', int32 [B].  ``require_ids`` as ``decode_naic`` (bofi_vocab_require behind the call, on the last pass; the same refusals): that dict
        then carries 'required_pos' int32 [B, K] and 'required_moved' int32 [B]; ``require_phrases`` as ``decode_naic`` (bofi_vocab_require_units in its place, the
        same keys); ``require_any`` as ``decode_naic`` (bofi_vocab_require_any in its place: 'required_alt' int32 [B, K] beside those keys).  ``nbest`` as ``decode_naic`` (bofi_vocab_nbest behind the call, on the last pass; the
        same refusals): that dict then carries 'nbest_seq' int64 [B, N, S], 'nbest_logp' float64 [B, N] and 'nbest_count' int32 [B]; ``nbest_no_repeat`` as
        ``decode_naic`` (bofi_vocab_nbest_norepeat in its place, N <= 6).  ``diverse`` / ``diversity_lambda`` / ``diverse_no_repeat`` as ``decode_naic``
        (bofi_vocab_diverse behind the call, on the last pass; the same refusals): that dict then carries 'diverse_seq', 'diverse_logp', 'diverse_aug' and
        'diverse_count'."""
        mp = self._refine_flag(refine_method, refine_rounds, raw_logits)
        B = ext_syn.size(0)
        ban, pick_on, req, nbest, nb_min, dv = self._post_options(ban_ids, no_repeat, repeat_min_id, block_trigrams, require_ids, nbest, nbest_no_repeat, B, None, mp,
                                                                   True, require_phrases, require_any, diverse, diversity_lambda, diverse_no_repeat)
        if ext_syn.dtype != torch.int32 or last.dtype != torch.int32 or ext_syn.size(1) != self.cfg.bound_len or last.numel() != B:
            raise hip.BofiHipError("ext_syn must be int32 [B, S+2] and last int32 [B]")
        S, V, dev = self.cfg.seq_length, self.cfg.tgt_vocab, ext_syn.device
        seq = torch.empty(B, S, dtype=torch.int64, device=dev)
        lp = torch.empty(B, S, V, dtype=torch.float32, device=dev)
        flags = (hip.FLAG_STRICT_Q1 if strict_q1 else 0) | (hip.FLAG_RAW_LOGITS if raw_logits else 0) | (refine_rounds << hip.FLAG_REFINE_SHIFT) | mp | (hip.FLAG_PICK_TRIGRAMS if block_trigrams else 0)
        rnd = torch.empty(B, S, dtype=torch.int32, device=dev) if mp else None
        o = hip.BofiCallOpts(refine_round=rnd.data_ptr() if mp else None)
        attn = {}
        self._attn_opts(o, attn, B, int(R), dev, attn_topk, attn_maps, attn_heads, attn_layer)
        self._pick_opts(o, ban, no_repeat, repeat_min_id, block_trigrams)
        hip.check(self._lib.bofi_engine_fill_naic(self._h, hip.ptr(ext_syn.contiguous()), hip.ptr(last.contiguous()), B, R, hip.ptr(att_len), flags,
                                                  hip.ptr(seq), hip.ptr(lp), C.byref(o), hip.stream_ptr()), "bofi_engine_fill_naic")
        self._post_passes(attn, B, seq, lp, last.contiguous, -1, ban, pick_on, req, nbest, nb_min, no_repeat, repeat_min_id, None, dv)
        res = (seq, lp, rnd) if mp else (seq, lp)
        return res + (attn,) if attn else res


class DecodePipeline:
    """Many loader batches through the NAIC bound+fill decode at the engine's throughput: what ``tools/eval.py`` and
    ``TransformerModel.decode_many`` run instead of one synchronised ``mode='sample'`` call per batch (the reference's eval loop,
    eval_utils.py:456-460 under tools/eval.py:123).

      * ``in_flight`` engine forks on streams that provably overlap, one launch each (default 3: with the copy stream that is the runtime's four
        hardware queues -- a copy stream that shares a queue with a launch stream: 161 against 210 k images/s, profiles/r05_decode_many.txt).  Launch streams and the copy stream are found by probing for queues of their own;
      * ``batches_per_launch`` (default 10) consecutive loader batches of one shape ride ONE launch (dynamic batching: quirk Q1 stays per batch, so every
        batch's result is its own decode's -- bit for bit under the same kernel family and hint); ragged batches (region counts given) are padded to the
        next of ``region_buckets`` so that differently clipped batches share launches and captured graphs (the padding is masked by the counts);
      * features are double-buffered per fork and copied from (pinned) host memory on a copy stream that runs ahead of the launches; the small
        outputs (ids, slot layout, per-image entropy / perplexity) come back through pinned buffers behind an event, the 48.6 MB of log-probs per
        batch stay on the device unless asked for.

    ``run(batches)`` is a generator: one dict per input batch, in input order, as soon as its launch is through -- while later launches are
    already in flight."""

    def __init__(self, engine: "BofiEngine", *, in_flight: Optional[int] = None, batches_per_launch: int = 16, strict_q1: bool = True, stats: bool = True,
                 keep_logprob: bool = False, region_buckets=(36, 48, 64, 80, 100, 128), fused_vocab: bool = False,
                 refine_rounds: int = 0, refine_method: str = "feed_back", attn_topk: int = 0, keep_attn: bool = False, ban_ids=None, no_repeat: bool = False,
                 repeat_min_id: int = 7, block_trigrams: bool = False, require_ids=None, require_phrases=None, require_any=None):
        BofiEngine._refine_flag(refine_method, refine_rounds, False)
        # ban_ids / no_repeat / repeat_min_id / block_trigrams: the constrained pick of BofiEngine.decode_naic on every launch; every yielded dict then carries constrained int32 [b].  Not
        # with fused_vocab (ids-only launches keep no distribution to re-pick from) or 'mask_predict'
        self.ban_ids = tuple(sorted({int(i) for i in ban_ids})) if ban_ids is not None else ()
        self.no_repeat, self.repeat_min_id = bool(no_repeat), int(repeat_min_id)
        self.block_trigrams = bool(block_trigrams)
        self.pick_on = bool(self.ban_ids) or self.no_repeat or self.block_trigrams
        if self.pick_on and fused_vocab:
            raise hip.BofiHipError("ban_ids / no_repeat / block_trigrams: not with fused_vocab (the ids-only launches keep no distribution to re-pick from)")
        if self.pick_on and refine_method == "mask_predict":
            raise hip.BofiHipError("ban_ids / no_repeat / block_trigrams: not with refine_method='mask_predict'")
        if self.ban_ids:
            hip.ban_bits(self.ban_ids, engine.cfg.tgt_vocab)        # (checked here, on the host: a bad list raises before anything is launched)
            if self.block_trigrams and engine.cfg.tgt_vocab - len(self.ban_ids) < engine.cfg.seq_length + 1:
                raise hip.BofiHipError("ban_ids: with block_trigrams at least seq_length + 1 ids must stay")
        # require_ids: required words (BofiEngine.decode_naic(require_ids=...)) -- the default of ``run``, which states the forms; checked here so that a pipeline that cannot
        # place words refuses before anything is launched
        self.fused_vocab, self.refine_method, self.root_vocab = bool(fused_vocab), refine_method, engine.cfg.tgt_vocab
        self.require_ids = require_ids
        self._require_split(require_ids)
        # require_phrases: required multi-word units (BofiEngine.decode_naic(require_phrases=...)), in the same two forms and under the same refusals; not with require_ids
        self.require_phrases = require_phrases
        self._require_both(require_ids, require_phrases)
        self._phrase_split(require_phrases)
        # require_any: required alternatives (BofiEngine.decode_naic(require_any=...)), in the same two forms and under the same refusals; not with the other two
        self.require_any = require_any
        self._require_both(require_ids, require_phrases, require_any)
        self._any_split(require_any)
        # attn_topk = K > 0: every yielded dict carries attn_top int32 / attn_top_w float32 [b, S, K] -- each position's K heaviest regions (BofiEngine.decode_naic) -- on the
        # host, through the pinned buffers (rows x S x K x 8 bytes per launch); keep_attn: also attn [b, S, R of the launch's region bucket] on the device, as keep_logprob
        if not 0 <= int(attn_topk) <= 8:
            raise hip.BofiHipError("attn_topk must be in 0..8")
        self.attn_topk, self.keep_attn = int(attn_topk), bool(keep_attn)
        # refine_rounds / refine_method: as BofiEngine.decode_naic; with 'mask_predict' every yielded dict also carries refine_round [b, S]
        self.refine_rounds, self.refine_method = int(refine_rounds), refine_method
        if in_flight is None:                                    # 3 launch streams + the copy stream = the runtime's default of 4 hardware queues
            in_flight = 3
        if in_flight < 1 or batches_per_launch < 1:
            raise hip.BofiHipError("in_flight and batches_per_launch must be >= 1")
        if fused_vocab and keep_logprob:
            raise hip.BofiHipError("fused_vocab leaves no log-probs to keep")
        # fused_vocab: the forks own no vocabulary-wide buffers and every launch is an ids-only decode (BofiEngine.decode_naic(ids_only=True)): where the launch is
        # large enough for the row-block kernels, the generator and the vocabulary epilogue are one launch and the distribution never reaches memory
        self.fused_vocab = bool(fused_vocab)
        self.root, self.nf, self.bpl = engine, int(in_flight), int(batches_per_launch)
        self.strict_q1, self.stats, self.keep_logprob = strict_q1, stats, keep_logprob
        self.dev = engine.device
        # ragged loader batches (att_masks given: every batch is clipped to ITS longest image, AttModel.py:113-120) are padded to the next of a few region counts, so that
        # consecutive batches share launches and captured graphs; the padding rows are masked by the region counts like any short image's
        self.buckets = sorted({int(r) for r in region_buckets if int(r) <= engine.max_regions} | {int(engine.max_regions)})
        self._slots = None                                       # built for the first launch's shape

    def _build(self, rows_max: int):
        # launch streams AND the copy stream on hardware queues of their own, found by probing (two streams on one queue serialise: a copy stream that
        # shares a queue with a launch stream costs a quarter of the throughput)
        streams = pick_concurrent_streams(self.nf + 1, self.dev, candidates=24)
        self.copy_stream = streams.pop() if len(streams) == self.nf + 1 else torch.cuda.Stream(self.dev)
        while len(streams) < self.nf:                            # (fewer hardware queues than launches in flight: the extra ones share)
            streams.append(torch.cuda.Stream(self.dev))
        self._slots = []
        for k in range(self.nf):
            e = self.root.fork(max_batch=rows_max, ids_only=self.fused_vocab)
            e.set_decodes_in_flight(self.nf)
            self._slots.append(dict(eng=e, stream=streams[k], feats=[{}, {}], lens=[None, None], out=None, host=None, copied=[torch.cuda.Event(), torch.cuda.Event()],
                                    done=torch.cuda.Event()))
        self.rows_max = rows_max

    def _require_split(self, require_ids):
        """``require_ids`` of a run as (flat, per_batch): one flat id list for every image, or an iterator of per-batch tables aligned with the batches; (None, None) when
        off.  The refusals of required words are raised here."""
        if require_ids is None:
            return None, None
        import numpy as np
        if isinstance(require_ids, (torch.Tensor, np.ndarray)):
            raise hip.BofiHipError("require_ids: a pipeline takes one flat id list for every image or a sequence of per-batch tables")
        seq = require_ids if hasattr(require_ids, "__len__") else None
        if seq is not None and len(seq) == 0:
            return None, None
        if self.fused_vocab:
            raise hip.BofiHipError("require_ids: not with fused_vocab (the ids-only launches keep no distribution to place the words by)")
        if self.refine_method == "mask_predict":
            raise hip.BofiHipError("require_ids: not with refine_method='mask_predict'")
        if self.block_trigrams:
            raise hip.BofiHipError("require_ids: not with block_trigrams (a placement could create a blocked trigram)")
        if seq is not None and isinstance(seq[0], (int, np.integer)):
            flat = hip.require_table(list(seq), 1, self.root_vocab, self.ban_ids)      # (checked once, here)
            return (None, None) if flat is None else ([int(i) for i in flat[0]], None)
        return None, iter(require_ids)

    @staticmethod
    def _require_both(require_ids, require_phrases, require_any=None) -> None:
        on = lambda v: v is not None and not (hasattr(v, "__len__") and len(v) == 0)
        if on(require_ids) and on(require_phrases):
            raise hip.BofiHipError("require_ids and require_phrases: give one (single ids are units of length 1)")
        if on(require_any) and (on(require_ids) or on(require_phrases)):
            raise hip.BofiHipError("require_ids / require_phrases and require_any: give one (a word or a unit is a group of one alternative)")

    def _any_split(self, require_any):
        """``require_any`` of a run as (flat, per_batch): one flat list of groups for every image, or an iterator of per-batch tables aligned with the batches; (None,
        None) when off.  The refusals are those of required phrases, raised here."""
        if require_any is None:
            return None, None
        import numpy as np
        if isinstance(require_any, (torch.Tensor, np.ndarray)):
            raise hip.BofiHipError("require_any: a pipeline takes one flat list of groups for every image or a sequence of per-batch tables")
        seq = require_any if hasattr(require_any, "__len__") else None
        if seq is not None and len(seq) == 0:
            return None, None
        if self.fused_vocab:
            raise hip.BofiHipError("require_any: not with fused_vocab (the ids-only launches keep no distribution to place the words by)")
        if self.refine_method == "mask_predict":
            raise hip.BofiHipError("require_any: not with refine_method='mask_predict'")
        if self.block_trigrams:
            raise hip.BofiHipError("require_any: not with block_trigrams (a placement could create a blocked trigram)")
        is_id = lambda v: isinstance(v, (int, np.integer))
        if seq is not None and any(is_id(g) for g in seq):
            hip.require_any_table(list(seq), 1, self.root_vocab)     # (raises, showing the nesting)
        # one flat list of groups: an element's first non-empty entry is an alternative (a list of ids); in a per-batch table it is a group or an image (lists of lists)
        first = lambda g: next((u for u in g if is_id(u) or (u is not None and len(u))), None) if isinstance(g, (list, tuple)) else None
        if seq is not None and any(first(g) is not None and (is_id(first(g)) or is_id(first(g)[0])) for g in seq):
            flat = hip.require_any_table(list(seq), 1, self.root_vocab, self.ban_ids, self.no_repeat, self.repeat_min_id)      # (checked once, here)
            return (None, None) if flat is None else ([[[int(i) for i in u if i >= 0] for u in g] for g in flat[0].tolist()], None)
        return None, iter(require_any)

    def _phrase_split(self, require_phrases):
        """``require_phrases`` of a run as (flat, per_batch): one flat list of units for every image, or an iterator of per-batch tables aligned with the batches; (None,
        None) when off.  The refusals are those of required words, raised here."""
        if require_phrases is None:
            return None, None
        import numpy as np
        if isinstance(require_phrases, (torch.Tensor, np.ndarray)):
            raise hip.BofiHipError("require_phrases: a pipeline takes one flat list of units for every image or a sequence of per-batch tables")
        seq = require_phrases if hasattr(require_phrases, "__len__") else None
        if seq is not None and len(seq) == 0:
            return None, None
        if self.fused_vocab:
            raise hip.BofiHipError("require_phrases: not with fused_vocab (the ids-only launches keep no distribution to place the words by)")
        if self.refine_method == "mask_predict":
            raise hip.BofiHipError("require_phrases: not with refine_method='mask_predict'")
        if self.block_trigrams:
            raise hip.BofiHipError("require_phrases: not with block_trigrams (a placement could create a blocked trigram)")
        if seq is not None and any(isinstance(u, (int, np.integer)) for u in seq):
            raise hip.BofiHipError("require_phrases: a unit is a list of ids -- [[3, 4]] is one unit of two ids; for single ids give require_ids")
        if seq is not None and any(isinstance(u, (list, tuple)) and len(u) and isinstance(u[0], (int, np.integer)) for u in seq):
            flat = hip.require_unit_table(list(seq), 1, self.root_vocab, self.ban_ids, self.no_repeat, self.repeat_min_id)      # (checked once, here)
            return (None, None) if flat is None else ([[int(i) for i in u if i >= 0] for u in flat[0].tolist()], None)
        return None, iter(require_phrases)

    def _require_launch(self, group, b):
        """The [rows, K] host table of a launch from its batches' tables (each checked on the host by ``hip.require_table``), and every batch's own K (0: none); (None,
        ks) when no batch of the launch requires a word."""
        if any(len(g) > 3 and g[3] == "any" for g in group):    # alternatives: a [rows, K, A, L] table, every batch checked by ``hip.require_any_table``
            tabs = [hip.require_any_table(g[2], b, self.root_vocab, self.ban_ids, self.no_repeat, self.repeat_min_id) if g[2] is not None else None for g in group]
            ks = [0 if t is None else t.size(1) for t in tabs]
            if max(ks) == 0:
                return None, ks
            full = torch.full((len(group) * b, max(ks)) + tuple(max(t.size(d) for t in tabs if t is not None) for d in (2, 3)), -1, dtype=torch.int32)
            for i, t in enumerate(tabs):
                if t is not None:
                    full[i * b:(i + 1) * b, :t.size(1), :t.size(2), :t.size(3)] = t
            return full, ks
        if any(len(g) > 3 and g[3] for g in group):             # units: a [rows, K, L] table, every batch checked by ``hip.require_unit_table``
            tabs = [hip.require_unit_table(g[2], b, self.root_vocab, self.ban_ids, self.no_repeat, self.repeat_min_id) if g[2] is not None else None for g in group]
            ks = [0 if t is None else t.size(1) for t in tabs]
            if max(ks) == 0:
                return None, ks
            full = torch.full((len(group) * b, max(ks), max(t.size(2) for t in tabs if t is not None)), -1, dtype=torch.int32)
            for i, t in enumerate(tabs):
                if t is not None:
                    full[i * b:(i + 1) * b, :t.size(1), :t.size(2)] = t
            return full, ks
        tabs = [hip.require_table(g[2], b, self.root_vocab, self.ban_ids) if len(g) > 2 and g[2] is not None else None for g in group]
        ks = [0 if t is None else t.size(1) for t in tabs]
        K = max(ks)
        if K == 0:
            return None, ks
        full = torch.full((len(group) * b, K), -1, dtype=torch.int32)
        for i, t in enumerate(tabs):
            if t is not None:
                full[i * b:(i + 1) * b, :t.size(1)] = t
        return full, ks

    @staticmethod
    def _as_host_or_device(x):
        return torch.from_numpy(x) if not torch.is_tensor(x) else x

    def _width(self, F: int) -> int:
        """The feature width of a launch's buffer: dense items of an unaligned att_feat_size (2053) are copied into the engine's zero-padded width."""
        cfg = self.root.cfg
        return cfg.att_feat_padded if F == cfg.att_feat_size else F

    def _bucket(self, r: int) -> int:
        for b in self.buckets:
            if b >= r:
                return b
        raise hip.BofiHipError(f"{r} regions exceed the engine's max_regions={self.root.max_regions}")

    def run(self, batches, require_ids=None, require_phrases=None, require_any=None):
        """``batches``: iterable of ``att_feats`` or ``(att_feats, att_len)``: [b, R, F] tensors / arrays in the engine's compute dtype or float32, on
        the host (pinned: the copy is asynchronous) or the device; ``att_len`` int32 [b] region counts or None (every image has R regions).  An item may
        also be a ``features.RaggedBatch``: its real rows alone are copied, in the files' dtype, and ``bofi_pack_regions`` pads them to the region bucket
        in the compute dtype on the device (a batch whose images all have the bucket's count is decoded without counts, as the loader hands it over).  A
        ``features.BoxRaggedBatch`` (use_box) also brings boxes and image sizes: ``bofi_pack_regions_box`` appends the geometry columns, sorts by box area and
        writes the engine's padded width.  Dense items of an ``att_feat_size`` that is no multiple of 64 are copied into that zero-padded width.
        ``require_ids`` (default: the constructor's): required words, as ``BofiEngine.decode_naic`` places them -- one flat id list for every image, or a sequence of
        per-batch tables aligned with ``batches`` (each a [b, K] int table, a list of b id lists, one flat list for the batch, or None); a launch that carries several
        batches concatenates their tables, and every batch's result is its own ``decode_naic(require_ids=...)``: its dict carries required_pos int32 [b, K of the batch]
        and required_moved int32 [b] (no keys for a batch that requires nothing).  Not with ``fused_vocab``, 'mask_predict' or ``block_trigrams``: raised here, before
        anything is launched.
        ``require_phrases`` (default: the constructor's): required multi-word units, as ``BofiEngine.decode_naic(require_phrases=...)`` places them, in the same two
        forms -- one flat list of units (each a list of 1..4 ids) for every image, or a sequence of per-batch tables aligned with ``batches`` (each a list of b unit lists,
        one flat list of units for the batch, a [b, K, L] int table, or None) --, with the same keys (required_pos holds the units' start positions) and refusals.  Not
        together with ``require_ids``: give one.
        ``require_any`` (default: the constructor's): required alternatives, as ``BofiEngine.decode_naic(require_any=...)`` places them, in the same two forms -- one
        flat list of groups (each a list of 1..4 alternatives, each a list of 1..4 ids) for every image, or a sequence of per-batch tables aligned with ``batches`` (each
        a list of b group lists, one flat list of groups for the batch, a [b, K, A, L] int table, or None) --, with the keys required_pos (the start of each group's
        placed alternative), required_alt int32 [b, K of the batch] (its index in the group) and required_moved, and the same refusals.  Not together with the other
        two: give one."""
        if require_ids is None and require_phrases is None and require_any is None:
            require_ids, require_phrases, require_any = self.require_ids, self.require_phrases, self.require_any
        self._require_both(require_ids, require_phrases, require_any)
        flat, per_batch = self._require_split(require_ids)
        if flat is None and per_batch is None:
            flat, per_batch = self._phrase_split(require_phrases)
            if flat is None and per_batch is None:
                flat, per_batch = self._any_split(require_any)
                return self._run(batches, flat, per_batch, "any" if flat is not None or per_batch is not None else False)
            return self._run(batches, flat, per_batch, flat is not None or per_batch is not None)
        return self._run(batches, flat, per_batch)

    def _run(self, batches, req_flat, req_iter, units=False):      # units: False (words), True (units), 'any' (alternatives)
        from .features import RaggedBatch
        pending = []                                             # launches in flight: (slot, [batch sizes])
        group, gkey = [], None
        j = 0

        def flush():
            nonlocal j, group
            if not group:
                return
            k, p = j % self.nf, (j // self.nf) % 2
            if j >= self.nf:
                yield from self._finish(pending.pop(0))
            self._launch(k, p, group, gkey)
            pending.append((k, [g[0].B if isinstance(g[0], RaggedBatch) else g[0].shape[0] for g in group], self._slots[k]["req_ks"]))
            j += 1
            group = []

        for item in batches:
            req = req_flat
            if req_iter is not None:
                try:
                    req = next(req_iter)
                except StopIteration:
                    raise hip.BofiHipError("require_ids / require_phrases / require_any: fewer per-batch tables than batches") from None
            if isinstance(item, RaggedBatch):
                r = self._bucket(item.max_len)
                key = (item.B, r, item.out_F, self.root.dtype, item.equal_lengths and item.max_len == r)
                if group and (key != gkey or len(group) >= self.bpl):
                    yield from flush()
                group.append((item, None, req, units))
                gkey = key
                continue
            att, lens = item if isinstance(item, (tuple, list)) else (item, None)
            att = self._as_host_or_device(att)
            lens = None if lens is None else self._as_host_or_device(lens).to(torch.int32)
            b, r = att.shape[0], att.shape[1]
            key = (b, r if lens is None else self._bucket(r), self._width(att.shape[2]), att.dtype, lens is None)
            if group and (key != gkey or len(group) >= self.bpl):
                yield from flush()
            group.append((att, lens, req, units))
            gkey = key
        yield from flush()
        while pending:
            yield from self._finish(pending.pop(0))

    def _launch(self, k, p, group, key):
        b, R, F, dt, no_len = key
        nb, rows = len(group), len(group) * b
        if self._slots is None:
            self._build(max(rows, self.bpl * b))
        if rows > self.rows_max:
            raise hip.BofiHipError(f"a launch of {rows} images exceeds the pipeline's {self.rows_max} (first batch x batches_per_launch)")
        sl = self._slots[k]
        e, st = sl["eng"], sl["stream"]
        has_len = not no_len
        cs = self.copy_stream
        caller = torch.cuda.current_stream(self.dev)
        with torch.cuda.stream(cs):
            # (the buffers are created -- and zero-filled -- ON the copy stream: a fill enqueued on the caller's stream would race the copies below)
            buf = sl["feats"][p].get((R, F, dt))
            if buf is None:
                buf = sl["feats"][p][(R, F, dt)] = torch.zeros(self.rows_max, R, F, dtype=dt, device=self.dev)
            if has_len and sl["lens"][p] is None:
                sl["lens"][p] = torch.zeros(self.rows_max, dtype=torch.int32, device=self.dev)
            feats, lens = buf[:rows], (sl["lens"][p][:rows] if has_len else None)
            cs.wait_event(sl["done"])                            # the launch that last read this slot's buffers is through (it was finished before this one is issued)
            staged = self._stage_ragged(sl, p, group)
            for i, (att, ln, *_) in enumerate(group):
                if i in staged:                                  # a RaggedBatch: its rows and offsets to the slot's staging buffer, the padding made on the device
                    srows, soffs = staged[i][:2]
                    srows.copy_(att.rows, non_blocking=True)
                    soffs.copy_(att.offsets, non_blocking=True)
                    if len(staged[i]) == 4:                      # a BoxRaggedBatch: boxes and sizes beside them, the box launch (geometry columns, area sort, padded width)
                        sboxes, swh = staged[i][2:]
                        sboxes.copy_(att.boxes, non_blocking=True)
                        swh.copy_(att.wh, non_blocking=True)
                        hip.pack_regions_box(srows, sboxes, swh, att.wh, soffs, att.offsets, feats[i * b:(i + 1) * b], norm_att=att.norm, norm_box=att.norm_box,
                                             att_len=lens[i * b:(i + 1) * b] if has_len else None)
                        continue
                    hip.pack_regions(srows, soffs, att.offsets, feats[i * b:(i + 1) * b], norm=att.norm, att_len=lens[i * b:(i + 1) * b] if has_len else None)
                    continue
                for src in (att, ln):                            # a DEVICE batch was produced on its caller's stream: the copy waits for that stream, and the caching
                    if src is not None and src.is_cuda:          # allocator must not hand the batch's memory out again while the copy is pending
                        cs.wait_stream(caller)
                        src.record_stream(cs)
                feats[i * b:(i + 1) * b, :att.shape[1], :att.shape[2]].copy_(att, non_blocking=True)      # (a batch clipped below the bucket leaves padding rows: masked by its counts; columns past an unaligned att_feat_size stay zero)
                if has_len:
                    lens[i * b:(i + 1) * b].copy_(ln, non_blocking=True)
            sl["copied"][p].record(cs)
        sl["last"] = (feats, lens, b, nb, rows)                  # (kept for the fallback decode of _finish: this slot's buffers stay untouched until its next launch)
        req, sl["req_ks"] = self._require_launch(group, b)
        with torch.cuda.stream(st):
            st.wait_event(sl["copied"][p])
            sl["req"] = None if req is None else req.to(self.dev)      # (on the launch's stream: the post-pass that reads it follows there)
            self._decode_and_copy_out(sl)
            sl["done"].record(st)

    def _stage_ragged(self, sl, p, group):
        """Device views {item index: (rows, offsets)} -- (rows, offsets, boxes, wh) for a BoxRaggedBatch -- for the RaggedBatch items of ``group``, carved out of slot ``sl``'s staging buffers of parity ``p`` (grown,
        never shrunk; created and reused on the copy stream alone, so the stream orders every use)."""
        from .features import BoxRaggedBatch, RaggedBatch
        items = [(i, g[0]) for i, g in enumerate(group) if isinstance(g[0], RaggedBatch)]
        if not items:
            return {}
        boxed = lambda it: isinstance(it, BoxRaggedBatch)
        # (every item's bytes are a multiple of 16: F % 8 == 0 is checked by the kernel's wrapper, and a box is 16 bytes)
        need = sum(it.rows.numel() * it.rows.element_size() + (it.boxes.numel() * 4 if boxed(it) else 0) for _, it in items)
        need_off = sum(it.B + 1 + (2 * it.B if boxed(it) else 0) for _, it in items)
        stage = sl.setdefault("stage", [None, None])
        if stage[p] is None or stage[p][0].numel() < need or stage[p][1].numel() < need_off:
            old = stage[p]
            stage[p] = (torch.empty(max(need, old[0].numel() if old else 0), dtype=torch.uint8, device=self.dev),
                        torch.empty(max(need_off, old[1].numel() if old else 0), dtype=torch.int32, device=self.dev))
        raw, offs = stage[p]
        views, o, q = {}, 0, 0
        for i, it in items:
            n = it.rows.numel() * it.rows.element_size()
            views[i] = (raw[o:o + n].view(it.rows.dtype).view(it.rows.shape), offs[q:q + it.B + 1])
            o, q = o + n, q + it.B + 1
            if boxed(it):
                nb = it.boxes.numel() * 4
                views[i] += (raw[o:o + nb].view(torch.float32).view(it.boxes.shape), offs[q:q + 2 * it.B].view(it.B, 2))
                o, q = o + nb, q + 2 * it.B
        return views

    def _decode_and_copy_out(self, sl):
        e = sl["eng"]
        feats, lens, b, nb, rows = sl["last"]
        if self.fused_vocab and not e.ids_only_fused(rows):      # (a launch too small for the fused generator -- a short tail: a plain fork of this slot's, made when first needed)
            if sl.get("eng_plain") is None:
                sl["eng_plain"] = self.root.fork(max_batch=self.rows_max)
                sl["eng_plain"].set_decodes_in_flight(self.nf)
            e = sl["eng_plain"]
        sl["ran"] = e
        sl["out"] = e.decode_naic(feats, lens, strict_q1=self.strict_q1, graph=True, out=sl["out"] if sl["out"] is not None and sl["out"]["seq"].shape[0] == rows else None,
                                  q1_group=b if nb > 1 else 0, row_stats=self.stats, want_logprob=self.keep_logprob, ids_only=self.fused_vocab,
                                  refine_rounds=self.refine_rounds, refine_method=self.refine_method, attn_topk=self.attn_topk, attn_maps=self.keep_attn,
                                  ban_ids=self.ban_ids or None, no_repeat=self.no_repeat, repeat_min_id=self.repeat_min_id, block_trigrams=self.block_trigrams,
                                  **({} if sl.get("req") is None else {("require_ids", "require_phrases", "require_any")[sl["req"].dim() - 2]: sl["req"]}))
        out = sl["out"]
        small = {k2: out[k2] for k2 in ("seq", "phrase_num", "phrase_length", "phrase_syn", "bound_saturated")}
        if self.refine_method == "mask_predict":
            small["refine_round"] = out["refine_round"]
        if self.attn_topk:
            small["attn_top"], small["attn_top_w"] = out["attn_top"], out["attn_top_w"]
        if self.pick_on:
            small["constrained"] = out["constrained"]
        if sl.get("req") is not None:
            small["required_pos"], small["required_moved"] = out["required_pos"], out["required_moved"]
            if sl["req"].dim() == 4:
                small["required_alt"] = out["required_alt"]
        if self.stats:
            small["entropy"], small["perplexity"] = e.entropy_perplexity(out)
        if sl["host"] is None or sl["host"].keys() != small.keys() or any(sl["host"][k2].shape != v.shape for k2, v in small.items()):
            sl["host"] = {k2: torch.empty(v.shape, dtype=v.dtype).pin_memory() for k2, v in small.items()}
        for k2, v in small.items():
            sl["host"][k2].copy_(v, non_blocking=True)
        sl["lp"] = out["seq_logprob"].clone() if self.keep_logprob else None
        sl["attn"] = out["attn"].clone() if self.keep_attn else None

    def _finish(self, launch):
        k, sizes, req_ks = launch
        sl = self._slots[k]
        sl["done"].synchronize()
        sat = int(sl["host"]["bound_saturated"][0])
        if sat:                                                  # the fp16 loop kernel clamped something (BofiEngine.saturated): this launch again with the bf16 iterations

            def again():
                with torch.cuda.stream(sl["stream"]):
                    self._decode_and_copy_out(sl)
                    sl["done"].record(sl["stream"])
                sl["done"].synchronize()
            sl["ran"]._redo_without_loop_kernel(sat, again)
        mine = {k2: v.clone() for k2, v in sl["host"].items() if k2 != "bound_saturated"}      # (one private copy per launch: the pinned buffers are the next launch's; batches are views of it)
        o = 0
        for i, b in enumerate(sizes):
            res = {k2: v[o:o + b] for k2, v in mine.items()}
            if "required_pos" in res:                            # (a batch's own K columns; no keys for a batch of the launch that requires nothing)
                if req_ks[i]:
                    res["required_pos"] = res["required_pos"][:, :req_ks[i]]
                    if "required_alt" in res:
                        res["required_alt"] = res["required_alt"][:, :req_ks[i]]
                else:
                    del res["required_pos"], res["required_moved"]
                    res.pop("required_alt", None)
            if sl["lp"] is not None:
                res["seq_logprob"] = sl["lp"][o:o + b]
            if sl["attn"] is not None:
                res["attn"] = sl["attn"][o:o + b]
            o += b
            yield res
