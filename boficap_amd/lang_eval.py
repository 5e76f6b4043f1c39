"""Language scores of a validation pass on the device: the token-level metrics of coco-caption's ``COCOEvalCap`` that need no Java --
BLEU-1..4 (corpus), ROUGE-L and CIDEr -- for one decoded caption per image against the image's references, plus the means of the decode's
per-image entropy and perplexity (the reference's ``language_eval``, captioning/utils/eval_utils.py:48-123).

    ev = LanguageEval(gts, device)                          # once per run: references packed, uploaded, their records built
    stats = ev.evaluate(seq, entropy, perplexity)           # per validation: two launches and one small read-back
    stats_n = ev.evaluate_n(sampled, n)                     # n sampled captions per image: their oracle and average scores (``eval_oracle``)

``gts``: per image either integer rows (``LabelStore.gts``) or a list of id strings.  Tokens are ids under the ``'eval'`` rule (the ids
before the first id <= 0: ``decode_sequence``, misc.py:62-74) on both sides; the candidates' rule is applied on the device.  CIDEr takes its
document frequencies from the evaluated references (``CiderD(df='corpus')`` at one candidate per image: coco-caption's ``Cider``), corpus
BLEU comes from the summed counts by ``bleu.bleu_of_comps``, ROUGE-L is the mean of bofi_rouge_score.  METEOR and SPICE (Java) and the PTB
tokenizer are not built: the scores are over the ids as they stand.
"""
from __future__ import annotations

import numpy as np
import torch

from . import hip
from .bleu import bleu_of_comps
from .cider import MAX_TOKENS, ORDERS, DfTable, id_lists, pack_host, upload
from .rewards import RewardScorer
from .rouge import Rouge, eval_token_list

KEYS = ("Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L", "CIDEr")
MAX_SAMPLES = 64              # bofi_oracle_stats: one lane of a wavefront per sample


def eval_reference_lists(gts):
    """Per image, the references as token lists under the 'eval' rule: integer rows, or strings of space-separated ids."""
    out = []
    for g in gts:
        if len(g) and isinstance(g[0], str):
            out.append([eval_token_list(ids) for ids in id_lists(g)])
        else:
            out.append([eval_token_list(row) for row in np.asarray(g).reshape(len(g), -1)])
    return out


class LanguageEval:
    """The references of a validation set, packed and with their records on the device."""

    def __init__(self, gts, device=None):
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.images = len(gts)
        if self.images == 0:
            raise ValueError("a validation set needs at least one image")
        # CIDEr-D alone in the reward kernel (BLEU weight 0: its value is bofi_cider_score's), whose counts serve the corpus BLEU
        self.reward = RewardScorer(df="corpus", cider_weight=1.0, bleu_weight=0.0, device=self.device)
        self.rouge = Rouge(rule="eval", device=self.device)
        df = DfTable("corpus", self.device)
        self.pk = upload(pack_host(eval_reference_lists(gts), self.images, 1, 1, df), self.device, df)
        self.records = self.reward.records(self.pk)

    def evaluate(self, seq, entropy=None, perplexity=None):
        """``seq``: decoded ids [images, S] (device or host, any integer type).  Returns {'Bleu_1'..'Bleu_4', 'ROUGE_L', 'CIDEr'} and, when given
        ([images] tensors or arrays), the means of ``entropy`` and ``perplexity``."""
        seq = torch.as_tensor(np.asarray(seq)) if not torch.is_tensor(seq) else seq
        seq = seq.to(self.device, torch.int64).contiguous()
        if seq.dim() != 2 or seq.shape[0] != self.images:
            raise ValueError(f"{tuple(seq.shape)} ids for {self.images} images: one row per image expected")
        if seq.shape[1] > MAX_TOKENS:
            raise ValueError(f"rows of {seq.shape[1]} ids: the scorers take rows of at most {MAX_TOKENS}")
        cand_len = ((seq <= 0).cumsum(1) == 0).sum(1).to(torch.int32)              # the ids before the first id <= 0
        _, cider, comps = self.reward._launch(None, seq, cand_len, 1, True, True, records=self.records)
        rouge, _, _ = self.rouge._launch(self.pk, seq, cand_len, 1)
        back = torch.cat([cider, rouge, comps.sum(0, dtype=torch.int64).to(torch.float64)]).cpu().numpy()      # (the sums are integers: exact)
        n = self.images
        total = [int(v) for v in back[2 * n:]]
        bleu = bleu_of_comps(total[0], total[1], total[2:2 + ORDERS], total[2 + ORDERS:])
        stats = {f"Bleu_{k + 1}": float(b) for k, b in enumerate(bleu)}
        stats["ROUGE_L"] = float(np.mean(back[n:2 * n]))
        stats["CIDEr"] = float(np.mean(back[:n]))
        for name, v in (("entropy", entropy), ("perplexity", perplexity)):
            if v is not None:
                v = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
                stats[name] = float(np.mean(v.astype(np.float64)))
        return stats

    def check_n(self, rows: int, S: int, n) -> int:
        """``n`` as an int, if ``rows`` rows of ``S`` ids are ``n`` samples of each of the set's images; ValueError otherwise."""
        if isinstance(n, bool) or int(n) != n or not 1 <= int(n) <= MAX_SAMPLES:
            raise ValueError(f"n = {n!r}: the oracle scores take 1 to {MAX_SAMPLES} samples per image")
        if rows != self.images * int(n):
            raise ValueError(f"{rows} rows for {self.images} images of {int(n)} samples: row m * n + i is sample i of image m")
        if S > MAX_TOKENS:
            raise ValueError(f"rows of {S} ids: the scorers take rows of at most {MAX_TOKENS}")
        return int(n)

    def _launch_n(self, seq, n: int):
        """The three launches of ``evaluate_n`` on device ids ``seq`` [images * n, S], enqueued on the current stream, no host copy: (sent float64
        [images * n, 6], stats float64 [images, 6, 2], pick int32 [images, 6], comps int32 [images * n, 10])."""
        seq = seq.to(self.device, torch.int64).contiguous()
        cand_len = ((seq <= 0).cumsum(1) == 0).sum(1).to(torch.int32)              # the ids before the first id <= 0
        _, cider, comps = self.reward._launch(None, seq, cand_len, n, True, True, records=self.records)
        rouge, _, _ = self.rouge._launch(self.pk, seq, cand_len, n)
        sent = torch.empty(self.images * n, len(KEYS), dtype=torch.float64, device=self.device)
        stats = torch.empty(self.images, len(KEYS), 2, dtype=torch.float64, device=self.device)
        pick = torch.empty(self.images, len(KEYS), dtype=torch.int32, device=self.device)
        hip.check(hip.lib().bofi_oracle_stats(hip.ptr(comps), hip.ptr(cider), hip.ptr(rouge), self.images, n, hip.ptr(sent), hip.ptr(stats), hip.ptr(pick),
                                              hip.stream_ptr()), "bofi_oracle_stats")
        return sent, stats, pick, comps

    def evaluate_n(self, seq, n):
        """The reference's ``eval_oracle``: ``seq`` holds ids [images * n, S] (device or host), row m * n + i = sample i of image m.  Every sample is
        scored at sentence level against its image's references (Bleu_k by bleu_scorer's per-sentence formula, ROUGE_L, CIDEr with the set's
        document frequencies); per image and metric the oracle is the best of the n and avg their mean.  Returns {'oracle_<M>', ...,
        'avg_<M>', ...} for M in KEYS -- the means over the images (over those that are not NaN, where an id above 65534 made a CIDEr NaN) --
        and 'per_image': {'sentence' [images, n, 6], 'oracle' [images, 6], 'avg' [images, 6], 'pick' [images, 6]: the lowest sample index that
        attains the oracle, -1 on NaN}.  Three launches and one read-back."""
        seq = torch.as_tensor(np.asarray(seq)) if not torch.is_tensor(seq) else seq
        if seq.dim() != 2:
            raise ValueError(f"{tuple(seq.shape)} ids: rows of ids expected")
        n = self.check_n(seq.shape[0], seq.shape[1], n)
        sent, stats, pick, _ = self._launch_n(seq, n)
        m, k = self.images, len(KEYS)
        back = torch.cat([sent.reshape(-1), stats.reshape(-1), pick.reshape(-1).to(torch.float64)]).cpu().numpy()      # (indices: exact)
        sentence = back[:m * n * k].reshape(m, n, k)
        both = back[m * n * k:m * n * k + 2 * m * k].reshape(m, k, 2)
        per = {"sentence": sentence, "oracle": np.ascontiguousarray(both[:, :, 0]), "avg": np.ascontiguousarray(both[:, :, 1]),
               "pick": back[m * n * k + 2 * m * k:].astype(np.int32).reshape(m, k)}
        out = {}
        for name in ("oracle", "avg"):
            for q, key in enumerate(KEYS):
                col = per[name][:, q]
                ok = ~np.isnan(col)
                out[f"{name}_{key}"] = float(np.mean(col)) if ok.all() else float(np.mean(col[ok])) if ok.any() else float("nan")
        out["per_image"] = per
        return out
