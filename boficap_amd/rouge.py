"""ROUGE-L of the pycocoevalcap package (``Rouge()``, beta = 1.2), the third token-level metric of ``COCOEvalCap``, on the device kernel of
csrc/rouge.hip (bofi_rouge_score, fp64).

    scorer = Rouge()
    scores = scorer.score(data_gts, seq, seq_per_img)      # [N] float32 on seq's device, current stream: no host copy, no sync
    mean, arr = scorer.compute_score(gts, res)             # the package's own (host) contract

For a candidate c and its image's references r_i, with lcs_i the longest common subsequence of c and r_i: p = max_i lcs_i / |c|,
r = max_i lcs_i / |r_i|, score = (1 + beta^2) p r / (r + beta^2 p) if p and r are non-zero, else 0; the corpus score is the mean over the
images.  An empty candidate or reference gives its pair p = r = 0.

Tokens are ids.  ``rule='reward'``: a row's ids up to and including its first 0, or the whole row (``array_to_str``, as the reward scorers
read a row); ``rule='eval'``: the ids before the first id <= 0 (``decode_sequence``, captioning/utils/misc.py:62-74, as the evaluation reads
a decoded row).
"""
from __future__ import annotations

import numpy as np
import torch

from . import hip
from .cider import _Bound, as_device_ids, host_candidates, id_lists, pack_host, token_list, upload

BETA = 1.2
RULES = {"reward": 0, "eval": 1}


def eval_token_list(row):
    """decode_sequence (misc.py:62-74) as ids: the ids of a row before its first id <= 0."""
    row = np.asarray(row).reshape(-1)
    z = np.flatnonzero(row <= 0)
    return [int(t) for t in (row[: z[0]] if z.size else row)]


def rule_lists(data_gts, rule: str):
    """Per image, the reference rows (any integer arrays) as token lists under ``rule``."""
    one = token_list if RULES[rule] == 0 else eval_token_list
    return [[one(row) for row in np.asarray(g).reshape(len(g), -1)] for g in data_gts]


class Rouge:
    """pycocoevalcap's ``Rouge()`` on the device.  ``on_device``: ``score`` takes and returns device tensors."""
    on_device = True

    def __init__(self, rule: str = "reward", beta: float = BETA, device=None):
        if rule not in RULES:
            raise ValueError(f"token rule {rule!r}: 'reward' (array_to_str) or 'eval' (decode_sequence)")
        if not float(beta) > 0:
            raise ValueError("beta must be above 0")
        self.rule, self.beta = rule, float(beta)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())

    def bind(self, data_gts, seq_per_img: int):
        """The scorer of one batch as a ``score_fn(seq)`` for XETrainer.rl_step."""
        return _Bound(self, data_gts, seq_per_img)

    def _launch(self, pk, seq, cand_len, seq_per_img, want_lcs=False, want_best=False):
        """bofi_rouge_score on uploaded references ``pk`` (cider.upload): (float64 [N], lcs int32 [seq_per_img * R] or None, best int32 [N, 2]
        or None), enqueued on the current stream."""
        N, S = seq.shape
        out64 = torch.empty(N, dtype=torch.float64, device=self.device)
        lcs = torch.empty(seq_per_img * pk.R, dtype=torch.int32, device=self.device) if want_lcs else None
        best = torch.empty(N, 2, dtype=torch.int32, device=self.device) if want_best else None
        hip.check(hip.lib().bofi_rouge_score(hip.ptr(seq), hip.ptr(cand_len), N, S, seq_per_img, hip.ptr(pk.start), hip.ptr(pk.tok), hip.ptr(pk.lens),
                                             pk.width, RULES[self.rule], self.beta, hip.ptr(out64), hip.ptr(lcs), hip.ptr(best), hip.stream_ptr()),
                  "bofi_rouge_score")
        return out64, lcs, best

    def score(self, data_gts, seq, seq_per_img: int, out64: bool = False, lcs: bool = False, best: bool = False):
        """ROUGE-L of row j of ``seq`` (device ids [N, S]) against ``data_gts[j // seq_per_img]`` (the image's reference rows, any integer
        arrays): float32 [N] on seq's device, enqueued on the current stream; with ``out64`` / ``lcs`` / ``best`` a tuple that adds the float64
        scores / every pair's subsequence length / the references that give p and r."""
        seq = as_device_ids(seq, self.device)
        N, S = seq.shape
        pk = upload(pack_host(rule_lists(data_gts, self.rule), N, S, int(seq_per_img), None), self.device, None)
        o64, l, b = self._launch(pk, seq, None, int(seq_per_img), lcs, best)
        out = o64.to(torch.float32)
        if not (out64 or lcs or best):
            return out
        return (out,) + ((o64,) if out64 else ()) + ((l,) if lcs else ()) + ((b,) if best else ())

    def compute_score(self, gts, res):
        """The package's contract: ``gts`` = {id: [ref str, ...]}, ``res`` = {id: [hypothesis str]} with the same keys, strings of
        space-separated ids.  Returns (mean score, float64 array of the scores in ``gts``' key order)."""
        assert gts.keys() == res.keys()
        cands, refs = [], []
        for i in gts.keys():
            hypo, ref = res[i], gts[i]
            assert type(hypo) is list
            assert len(hypo) == 1
            assert type(ref) is list
            assert len(ref) > 0
            cands.append(id_lists(hypo)[0])
            refs.append(id_lists(ref))
        if not cands:
            return 0.0, np.zeros(0)
        seq, lens = host_candidates(cands, self.device)
        pk = upload(pack_host(refs, len(cands), seq.shape[1], 1, None), self.device, None)
        arr = self._launch(pk, seq, lens, 1)[0].cpu().numpy()
        return float(np.mean(arr)), arr
