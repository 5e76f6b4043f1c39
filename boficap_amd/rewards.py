"""The whole self-critical reward of the reference's ``get_scores`` (captioning/utils/rewards.py:86-131) on the device:

    scores = cider_reward_weight * CIDEr-D + bleu_reward_weight * BLEU-4

with CIDEr-D the ``CiderD`` scorer of pyciderevalcap (boficap_amd.cider) and BLEU-4 the fourth per-sentence score of pycocoevalcap's
``Bleu(4)`` (option 'closest'), both on the kernels bofi_reward_refs / bofi_reward_score of csrc/cider.hip (fp64).  A term is computed
only if its weight is above 0, as get_scores does; without the CIDEr-D term no df table is needed.

    scorer = RewardScorer(df="coco-train-idxs", cider_weight=1.0, bleu_weight=0.5)
    scores = scorer.score(data_gts, seq, seq_per_img)      # [N] float32 on seq's device, current stream: no host copy, no sync
    score_fn = scorer.bind(data_gts, seq_per_img)          # XETrainer.rl_step's device score_fn
"""
from __future__ import annotations

import torch

from . import hip
from .cider import ORDERS, DfTable, _Bound, as_device_ids, pack_references, reference_lists

COMPS = 2 + 2 * ORDERS        # per candidate: testlen, reflen, guess[4], correct[4]


class RewardScorer:
    """``cider_weight`` x CIDEr-D (df file or ``'corpus'``, sigma) + ``bleu_weight`` x BLEU-4 of every candidate.  ``on_device``: ``score``
    takes and returns device tensors."""
    on_device = True

    def __init__(self, df="corpus", cider_weight: float = 1.0, bleu_weight: float = 0.0, sigma: float = 6.0, device=None):
        self.cider_weight = float(cider_weight) if float(cider_weight) > 0 else 0.0
        self.bleu_weight = float(bleu_weight) if float(bleu_weight) > 0 else 0.0
        if self.cider_weight == 0.0 and self.bleu_weight == 0.0:
            raise ValueError("a reward needs cider_weight > 0 or bleu_weight > 0")
        self.sigma = float(sigma)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.df = DfTable(df, self.device) if self.cider_weight > 0 else None

    def bind(self, data_gts, seq_per_img: int):
        """The scorer of one batch as a ``score_fn(seq)`` for XETrainer.rl_step."""
        return _Bound(self, data_gts, seq_per_img)

    def records(self, pk):
        """The records of uploaded references ``pk`` (cider.upload) by bofi_reward_refs, enqueued on the current stream: ``(pk, tensors)`` for
        ``_launch(records=...)`` -- a caller that scores many candidate sets against the same references builds them once."""
        R, stride, dev = pk.R, pk.stride, self.device
        rec_keys = torch.empty(R, stride, dtype=torch.int64, device=dev)
        rec_w = torch.empty(R, stride, dtype=torch.float64, device=dev)
        rec_off = torch.empty(R, ORDERS + 1, dtype=torch.int32, device=dev)
        rec_meta = torch.empty(R, ORDERS + 1, dtype=torch.float64, device=dev)
        rec_cnt = torch.empty(R, stride, dtype=torch.int32, device=dev)
        rec_len = torch.empty(R, dtype=torch.int32, device=dev)
        hip.check(hip.lib().bofi_reward_refs(hip.ptr(pk.tok), hip.ptr(pk.lens), R, pk.width, hip.ptr(pk.df_keys), hip.ptr(pk.df_vals), pk.n_df, pk.L,
                                             hip.ptr(rec_keys), hip.ptr(rec_w), hip.ptr(rec_off), hip.ptr(rec_meta), hip.ptr(rec_cnt), hip.ptr(rec_len),
                                             stride, hip.stream_ptr()), "bofi_reward_refs")
        return pk, (rec_keys, rec_w, rec_off, rec_meta, rec_cnt, rec_len)

    def _launch(self, refs, seq, cand_len, seq_per_img, want64, want_comps, records=None):
        """``records``: what ``records()`` returned for these references -- no packing and no refs kernel then (``refs`` is not read)."""
        N, S = seq.shape
        pk, (rec_keys, rec_w, rec_off, rec_meta, rec_cnt, rec_len) = records if records is not None else self.records(
            pack_references(refs, N, S, seq_per_img, self.device, self.df))
        stride, dev = pk.stride, self.device
        out = torch.empty(N, dtype=torch.float32, device=dev)
        out64 = torch.empty(N, dtype=torch.float64, device=dev) if want64 else None
        comps = torch.empty(N, COMPS, dtype=torch.int32, device=dev) if want_comps else None
        hip.check(hip.lib().bofi_reward_score(hip.ptr(seq), hip.ptr(cand_len), N, S, seq_per_img, hip.ptr(pk.start), hip.ptr(pk.df_keys),
                                              hip.ptr(pk.df_vals), pk.n_df, pk.L, self.sigma, self.cider_weight, self.bleu_weight, hip.ptr(rec_keys),
                                              hip.ptr(rec_w), hip.ptr(rec_off), hip.ptr(rec_meta), hip.ptr(rec_cnt), hip.ptr(rec_len), stride,
                                              hip.ptr(out), hip.ptr(out64), hip.ptr(comps), hip.stream_ptr()), "bofi_reward_score")
        return out, out64, comps

    def score(self, data_gts, seq, seq_per_img: int, out64: bool = False, comps: bool = False):
        """get_scores: the weighted reward of row j of ``seq`` (device ids [N, S]) against ``data_gts[j // seq_per_img]`` (the image's
        reference rows, any integer arrays).  Returns float32 [N] on seq's device, enqueued on the current stream; with ``out64`` / ``comps``
        a tuple that adds the float64 scores / the int32 [N, 10] BLEU counts (testlen, reflen, guess[4], correct[4])."""
        seq = as_device_ids(seq, self.device)
        out, o64, c = self._launch(reference_lists(data_gts), seq, None, int(seq_per_img), out64, comps)
        if not (out64 or comps):
            return out
        return (out,) + ((o64,) if out64 else ()) + ((c,) if comps else ())
