"""BLEU-4 of the pycocoevalcap package (``Bleu(4)``, bleu_scorer.py with option 'closest'), the second term of the reference's
``get_scores`` (captioning/utils/rewards.py:86-131, ``bleu_scores[3]``), on the device kernels of csrc/cider.hip (boficap_amd.rewards).

    scorer = Bleu(4)
    scores = scorer.score(data_gts, seq, seq_per_img)      # per-sentence BLEU-4, [N] float32 on seq's device, current stream
    corpus, per_sentence = scorer.compute_score(gts, res)  # the package's own (host) contract

Tokens are the space-separated ids of ``array_to_str`` (the terminating 0 included).  The device counts every candidate's clipped n-gram
matches, its length and the closest reference length; ``compute_score`` turns those counts into the package's per-sentence and corpus
scores in Python floats, the package's own arithmetic.
"""
from __future__ import annotations

import math

from . import hip
from .cider import MAX_ID, ORDERS, host_candidates, id_lists
from .rewards import RewardScorer

TINY = 1e-15                  # bleu_scorer.py: so that a guess of 0 still scores 0
SMALL = 1e-9


def bleu_of_comps(testlen, reflen, guess, correct):
    """BLEU-1..4 of one sentence's (or the summed corpus') counts, as bleu_scorer.BleuScorer.compute_score computes them."""
    bleu, out = 1.0, []
    for k in range(ORDERS):
        bleu *= float(correct[k] + TINY) / (guess[k] + SMALL)
        out.append(bleu ** (1.0 / (k + 1)))
    ratio = (testlen + TINY) / (reflen + SMALL)
    if ratio < 1:
        out = [b * math.exp(1 - 1 / ratio) for b in out]
    return out


class Bleu:
    """pycocoevalcap's ``Bleu(4)`` on the device.  ``on_device``: ``score`` takes and returns device tensors."""
    on_device = True

    def __init__(self, n: int = 4, device=None):
        if n != ORDERS:
            raise ValueError(f"BLEU is built for n = {ORDERS}")
        self.scorer = RewardScorer(df=None, cider_weight=0.0, bleu_weight=1.0, device=device)
        self.device = self.scorer.device

    def bind(self, data_gts, seq_per_img: int):
        """The scorer of one batch as a ``score_fn(seq)`` for XETrainer.rl_step."""
        return self.scorer.bind(data_gts, seq_per_img)

    def score(self, data_gts, seq, seq_per_img: int, out64: bool = False, comps: bool = False):
        """Per-sentence BLEU-4 of row j of ``seq`` (device ids [N, S]) against ``data_gts[j // seq_per_img]``: float32 [N] on seq's device,
        enqueued on the current stream (RewardScorer.score's ``out64`` / ``comps`` tuple if asked)."""
        return self.scorer.score(data_gts, seq, seq_per_img, out64=out64, comps=comps)

    def compute_score(self, gts, res):
        """The package's contract: ``gts`` = {id: [ref str, ...]}, ``res`` = {id: [hypothesis str]} with the same keys, strings of
        space-separated ids.  Returns ([BLEU-1..4 of the corpus], [[per-sentence BLEU-k] for k = 1..4]) in ``gts``' key order."""
        assert gts.keys() == res.keys()
        cands, refs = [], []
        for i in gts.keys():
            hypo, ref = res[i], gts[i]
            assert type(hypo) is list
            assert len(hypo) == 1
            assert type(ref) is list
            assert len(ref) >= 1
            cands.append(id_lists(hypo)[0])
            refs.append(id_lists(ref))
        for c in cands:
            if c and not (0 <= min(c) and max(c) <= MAX_ID):
                raise hip.BofiHipError(f"a hypothesis id is outside [0, {MAX_ID}]: the BLEU scorer packs (id + 1) into 16 bits")
        rows = []
        if cands:
            seq, lens = host_candidates(cands, self.device)
            _, _, comps = self.scorer._launch(refs, seq, lens, 1, False, True)
            rows = comps.cpu().tolist()
        total = {"testlen": 0, "reflen": 0, "guess": [0] * ORDERS, "correct": [0] * ORDERS}
        per_sentence = [[] for _ in range(ORDERS)]
        for c in rows:
            testlen, reflen, guess, correct = c[0], c[1], c[2:2 + ORDERS], c[2 + ORDERS:]
            for k, b in enumerate(bleu_of_comps(testlen, reflen, guess, correct)):
                per_sentence[k].append(b)
            total["testlen"] += testlen
            total["reflen"] += reflen
            for k in range(ORDERS):
                total["guess"][k] += guess[k]
                total["correct"][k] += correct[k]
        return bleu_of_comps(total["testlen"], total["reflen"], total["guess"], total["correct"]), per_sentence
