"""Diversity of the n sampled captions of one image on the device (csrc/diversity.hip, fp64): the self-CIDEr score that the reference adds to
the 'new_self_critical' advantage (``get_self_cider_scores``, captioning/utils/rewards.py:119-139, ``Cider.my_self_cider`` of the
pyciderevalcap package) and the diversity statistics of its evaluation with ``sample_n`` > 1 (eval_utils.py:105-120: Div-1, Div-2,
mBLEU-1..4, self-CIDEr).

    sc = SelfCider(df="coco-train-idxs")                  # data/coco-train-idxs.p, as the reference resolves opt.cached_tokens
    scores = sc.score(seq, n)                             # [images] float64 on seq's device, current stream: no host copy, no sync
    M = sc.matrix(seq, n)                                 # [images, n, n]: plain CIDEr between the samples of an image
    stats = DiversityEval(df).evaluate(seq, n)            # one launch, one read-back

Rows of ``seq`` [images * n, S] are grouped per image, n consecutive rows each.  Self-CIDEr: M[i][j] = 1/4 sum over the orders k of the
cosine of the two samples' tf-idf k-gram vectors (no count clipping, no length penalty; the package's x10 and the reference's /10 cancel),
score = -log(sqrt(l_max) / sum sqrt(l)) / log n over M's eigenvalues l clipped below at 0.  Div-n = distinct n-grams of an image's samples /
their tokens, averaged over the images.  mBLEU-k = the mean over the sample positions i of the corpus BLEU-k with every image's sample i as
candidate and its other samples as references (``bleu.bleu_of_comps`` on the summed device counts).  Token rules as in boficap_amd.rouge:
``'reward'`` (array_to_str) or ``'eval'`` (decode_sequence).  ``df='corpus'`` is not built for these scores.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import hip
from .bleu import bleu_of_comps
from .cider import MAX_TOKENS, ORDERS, DfTable, resolve_df
from .rewards import COMPS
from .rouge import RULES

MAX_SAMPLES = 16             # samples per image the kernel keeps side by side
KEYS = ("Div-1", "Div-2", "mBLEU_1", "mBLEU_2", "mBLEU_3", "mBLEU_4", "self_cider")


def check_shape(N: int, S: int, n: int) -> int:
    """The number of images of N rows of S ids at n samples per image; raises for what the kernel does not take."""
    n = int(n)
    if n < 2:
        raise ValueError(f"diversity needs at least two samples per image, not {n}")
    if n > MAX_SAMPLES:
        raise ValueError(f"{n} samples per image: the diversity kernel takes at most {MAX_SAMPLES}")
    if N % n != 0:
        raise ValueError(f"{N} rows are not {n} per image")
    if not 1 <= S <= MAX_TOKENS:
        raise ValueError(f"rows of {S} ids: the scorers take rows of 1 to {MAX_TOKENS}")
    return N // n


class SelfCider:
    """``Cider.my_self_cider`` and the reference's ``get_div`` on the device.  ``on_device``: ``score`` takes and returns device tensors."""
    on_device = True

    def __init__(self, df, device=None):
        if df == "corpus":
            raise ValueError("df='corpus' is not built for the self-CIDEr score: pass a document-frequency file (cached_tokens)")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.df = DfTable(df, self.device)

    def _launch(self, seq, n, rule="reward", want_mat=False, want_comps=False):
        """bofi_diversity_score on device ids ``seq`` [images * n, S]: (score float64 [images], M float64 [images, n, n] or None, div int32
        [images, 3], comps int32 [images * n, 10] or None), enqueued on the current stream."""
        if rule not in RULES:
            raise ValueError(f"token rule {rule!r}: 'reward' (array_to_str) or 'eval' (decode_sequence)")
        if seq.dim() != 2:
            raise ValueError(f"ids of shape {tuple(seq.shape)}: [images * n, S] expected")
        N, S = seq.shape
        images = check_shape(N, S, n)
        if not seq.is_cuda:
            raise ValueError("seq is on the host: the diversity kernel takes device ids")
        seq = seq if seq.dtype == torch.int64 and seq.is_contiguous() else seq.to(torch.int64).contiguous()
        dev, lib = seq.device, hip.lib()
        nbytes = int(lib.bofi_diversity_workspace(images, int(n), S))
        work = torch.empty(max(1, nbytes // 8), dtype=torch.int64, device=dev)
        score = torch.empty(images, dtype=torch.float64, device=dev)
        mat = torch.empty(images, n, n, dtype=torch.float64, device=dev) if want_mat else None
        div = torch.empty(images, 3, dtype=torch.int32, device=dev)
        comps = torch.empty(N, COMPS, dtype=torch.int32, device=dev) if want_comps else None
        hip.check(lib.bofi_diversity_score(hip.ptr(seq), images, int(n), S, RULES[rule], hip.ptr(self.df.keys), hip.ptr(self.df.vals),
                                           int(self.df.keys.numel()), self.df.log_ref_len, hip.ptr(work), nbytes, hip.ptr(score), hip.ptr(mat),
                                           hip.ptr(div), hip.ptr(comps), hip.stream_ptr()), "bofi_diversity_score")
        return score, mat, div, comps

    def score(self, seq, n: int, rule: str = "reward"):
        """The self-CIDEr diversity of every image's ``n`` samples (rows of ``seq``, device ids [images * n, S]): float64 [images] on seq's
        device, enqueued on the current stream.  NaN for an image whose M is 0: every sample empty ('eval'), or without an n-gram of non-zero weight."""
        return self._launch(seq, n, rule)[0]

    def matrix(self, seq, n: int, rule: str = "reward"):
        """M [images, n, n] float64: plain CIDEr of every pair of an image's samples (exactly symmetric)."""
        return self._launch(seq, n, rule, want_mat=True)[1]


_SCORERS: dict = {}


def self_cider_scorer(opt, device=None):
    """The ``SelfCider`` of ``opt.cached_tokens`` (resolved as for CIDEr-D: a path, or data/<name>.p), built once per df file and device."""
    name = getattr(opt, "cached_tokens", "coco-train-idxs")
    if name == "corpus":
        raise ValueError("cached_tokens='corpus' is not built for the self-CIDEr score: it needs a document-frequency file")
    path = resolve_df(name)
    if path is None:
        raise hip.BofiHipError(f"the self-CIDEr reward needs a document-frequency file for opt.cached_tokens={name!r} (a path, or "
                               "data/<cached_tokens>.p of scripts/prepro_ngrams.py)")
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    key = (os.path.abspath(path), str(dev))
    if key not in _SCORERS:
        _SCORERS[key] = SelfCider(path, dev)
    return _SCORERS[key]


def get_self_cider_scores(data_gts, seq, opt):
    """The reference's contract (rewards.py:119-139): ``seq`` [images * n, S] with n = rows / len(data_gts); returns a float64 numpy array
    [images] (a host read-back: the training path takes ``SelfCider.score`` instead)."""
    seq = torch.as_tensor(seq)
    n = seq.shape[0] // len(data_gts)
    sc = self_cider_scorer(opt, seq.device if seq.is_cuda else None)
    return sc.score(seq.to(sc.device), n).cpu().numpy()


def stats_of_counts(div, comps, n: int):
    """Div-1, Div-2 and mBLEU-1..4 from the device counts: ``div`` integer [images, 3] (distinct unigrams, distinct bigrams, tokens),
    ``comps`` integer [images * n, 10].  Returns ({key: float}, Div-1 per image, Div-2 per image)."""
    div = np.asarray(div, dtype=np.int64)
    comps = np.asarray(comps, dtype=np.int64).reshape(-1, int(n), COMPS)
    tokens = div[:, 2].astype(np.float64)
    per = [np.where(tokens > 0, div[:, k].astype(np.float64) / np.maximum(tokens, 1.0), 0.0) for k in range(2)]
    stats = {"Div-1": float(np.mean(per[0])), "Div-2": float(np.mean(per[1]))}
    runs = []
    for i in range(int(n)):                                    # the corpus of position i: every image's sample i against its other samples
        tot = [int(v) for v in comps[:, i, :].sum(0)]
        runs.append(bleu_of_comps(tot[0], tot[1], tot[2:2 + ORDERS], tot[2 + ORDERS:]))
    for k in range(ORDERS):
        stats[f"mBLEU_{k + 1}"] = float(np.mean(np.array([r[k] for r in runs], dtype=np.float64)))
    return stats, per[0], per[1]


class DiversityEval:
    """The diversity statistics of an evaluation with ``sample_n`` > 1: ``evaluate`` is one launch and one read-back."""

    def __init__(self, df, device=None):
        self.scorer = SelfCider(df, device)
        self.device = self.scorer.device

    def evaluate(self, seq, n: int, rule: str = "eval"):
        """``seq``: sampled ids [images * n, S] (device or host, any integer type), n consecutive rows per image.  Returns {'Div-1', 'Div-2',
        'mBLEU_1'..'mBLEU_4', 'self_cider'} (means over the images; self_cider over the images whose score is not NaN) and the per-image
        arrays under 'per_image': {'Div-1', 'Div-2', 'self_cider'}."""
        seq = torch.as_tensor(np.asarray(seq)) if not torch.is_tensor(seq) else seq
        seq = seq.to(self.device, torch.int64).contiguous()
        score, _, div, comps = self.scorer._launch(seq, n, rule, want_comps=True)
        images = score.numel()
        back = torch.cat([score, div.reshape(-1).to(torch.float64), comps.reshape(-1).to(torch.float64)]).cpu().numpy()     # (the counts are integers: exact)
        sc = back[:images]
        stats, d1, d2 = stats_of_counts(back[images:4 * images].reshape(images, 3), back[4 * images:].reshape(-1, COMPS), n)
        ok = ~np.isnan(sc)
        stats["self_cider"] = float(np.mean(sc[ok])) if ok.any() else float("nan")
        stats["per_image"] = {"Div-1": d1, "Div-2": d2, "self_cider": sc}
        return stats
