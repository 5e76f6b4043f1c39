"""CIDEr-D reward of the self-critical step on the device: the ``CiderD`` scorer of the pyciderevalcap package that the reference's
``get_scores`` calls (captioning/utils/rewards.py:25-31, 86-131), on the kernels of csrc/cider.hip (fp64).

    scorer = CiderD(df="coco-train-idxs")                  # data/coco-train-idxs.p, as the reference resolves opt.cached_tokens
    scores = scorer.score(data_gts, seq, seq_per_img)      # [N] float32 on seq's device, current stream: no host copy, no sync
    mean, arr = scorer.compute_score(gts, res)             # the package's own (host) contract

The document-frequency file is the pickle of the reference's scripts/prepro_ngrams.py, read as the package reads it (``encoding='latin1'``,
``{'document_frequency': {tuple of id strings: count}, 'ref_len': images}``).  ``df='corpus'`` counts the document frequency over the call's
own references instead (every image's reference set once per candidate), with L = log(number of candidates).
"""
from __future__ import annotations

import math
import os
import pickle

import numpy as np
import torch

from . import hip

ORDERS = 4
MAX_ID = 65534               # (id + 1) must fit a 16-bit field of a key
MAX_TOKENS = 64              # longest token list of a row (the kernels' record holds its 250 n-grams)


def pack_key(ids) -> int:
    """The key of an n-gram (1 to 4 ids): (id + 1) in 16-bit fields, first id in the highest used field."""
    if not 1 <= len(ids) <= ORDERS:
        raise ValueError(f"an n-gram has 1 to {ORDERS} ids, not {len(ids)}")
    k = 0
    for i in ids:
        i = int(i)
        if not 0 <= i <= MAX_ID:
            raise hip.BofiHipError(f"id {i} is outside [0, {MAX_ID}]: the CIDEr-D scorer packs (id + 1) into 16 bits")
        k = (k << 16) | (i + 1)
    return k


def unpack_key(key: int):
    """The ids of a key (inverse of pack_key)."""
    ids = []
    while key:
        ids.append((key & 0xFFFF) - 1)
        key >>= 16
    return tuple(reversed(ids))


def token_list(row):
    """array_to_str (rewards.py:33-39) as ids: the row up to and including its first 0, or the whole row if it has none."""
    row = np.asarray(row).reshape(-1)
    z = np.flatnonzero(row == 0)
    return [int(t) for t in (row[: z[0] + 1] if z.size else row)]


def ngram_keys(tokens):
    """Every contiguous n-gram (n = 1..4) of a token list as keys, with multiplicity."""
    return [pack_key(tokens[p:p + k]) for k in range(1, ORDERS + 1) for p in range(len(tokens) - k + 1)]


def resolve_df(df):
    """The file behind ``cached_tokens``: an existing path as is, else data/<name>.p (rewards.py: CiderD(df=opt.cached_tokens)); None if
    neither exists.  'corpus' resolves to itself."""
    if df == "corpus":
        return df
    if df and os.path.isfile(df):
        return df
    p = os.path.join("data", f"{df}.p")
    return p if df and os.path.isfile(p) else None


def load_df(path):
    """The df pickle of prepro_ngrams.py as (sorted unique keys uint64, values L - log(max(1, df)) float64, L = log(ref_len))."""
    with open(path, "rb") as f:
        d = pickle.load(f, encoding="latin1")
    dfd, ref_len = d["document_frequency"], d["ref_len"]
    L = float(np.log(float(ref_len)))
    keys = np.empty(len(dfd), dtype=np.uint64)
    cnt = np.empty(len(dfd), dtype=np.float64)
    for i, (g, c) in enumerate(dfd.items()):
        try:
            ids = [int(t) for t in g]
        except ValueError:
            raise hip.BofiHipError(f"{path}: n-gram {g!r} is not made of ids -- a words pickle (coco-train-words.p); the reward compares ids "
                                   "as array_to_str emits them: use the -idxs file of prepro_ngrams.py") from None
        keys[i] = pack_key(ids)
        cnt[i] = c
    order = np.argsort(keys, kind="stable")
    keys, cnt = keys[order], cnt[order]
    if keys.size > 1 and not (keys[1:] > keys[:-1]).all():
        raise hip.BofiHipError(f"{path}: two n-grams of the table name the same ids")
    return keys, L - np.log(np.maximum(1.0, cnt)), L


class _Bound:
    """``score_fn(seq) -> [N]`` of XETrainer.rl_step for one batch's references (``on_device``: the trainer hands it the device ids)."""
    on_device = True

    def __init__(self, scorer, data_gts, seq_per_img, weight):
        self.scorer, self.data_gts, self.seq_per_img, self.weight = scorer, data_gts, seq_per_img, weight

    def __call__(self, seq):
        return self.scorer.score(self.data_gts, seq, self.seq_per_img, weight=self.weight)


class CiderD:
    """pyciderevalcap's ``CiderD(n=4, sigma=6.0, df=...)`` on the device.  ``on_device``: ``score`` takes and returns device tensors."""
    on_device = True

    def __init__(self, df="corpus", n: int = 4, sigma: float = 6.0, device=None):
        if n != ORDERS:
            raise ValueError(f"CIDEr-D is built for n = {ORDERS}")
        self.sigma = float(sigma)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.corpus = df == "corpus"
        self.df_keys = self.df_vals = None
        self.log_ref_len = 0.0
        if not self.corpus:
            path = resolve_df(df)
            if path is None:
                raise FileNotFoundError(f"no document-frequency file for cached_tokens={df!r} (neither a file nor data/{df}.p)")
            keys, vals, self.log_ref_len = load_df(path)
            self.df_keys = torch.from_numpy(keys.view(np.int64)).to(self.device)
            self.df_vals = torch.from_numpy(vals).to(self.device)

    def bind(self, data_gts, seq_per_img: int, weight: float = 1.0):
        """The scorer of one batch as a ``score_fn(seq)`` for XETrainer.rl_step."""
        return _Bound(self, data_gts, seq_per_img, weight)

    # ---- host side: the references (and the corpus df) packed into one pinned buffer, one copy
    def _launch(self, refs, seq, cand_len, seq_per_img, weight, want64):
        N, S = seq.shape
        if len(refs) * seq_per_img != N:
            raise ValueError(f"{N} candidates are not {seq_per_img} per image of {len(refs)} images")
        if S > MAX_TOKENS:
            raise hip.BofiHipError(f"candidates of {S} ids: the scorer takes rows of at most {MAX_TOKENS}")
        flat = [t for r in refs for t in r]
        if any(len(r) == 0 for r in refs):
            raise ValueError("every image needs at least one reference caption")
        width = max([len(t) for t in flat] + [1])
        if width > MAX_TOKENS:
            raise hip.BofiHipError(f"a reference of {width} tokens: the scorer takes rows of at most {MAX_TOKENS}")
        for t in flat:
            if t and not (0 <= min(t) and max(t) <= MAX_ID):
                raise hip.BofiHipError(f"a reference id is outside [0, {MAX_ID}]: the CIDEr-D scorer packs (id + 1) into 16 bits")
        R, n_img = len(flat), len(refs)
        start = np.zeros(n_img + 1, dtype=np.int32)
        start[1:] = np.cumsum([len(r) for r in refs])
        lens = np.array([len(t) for t in flat], dtype=np.int32)
        tok = np.zeros((R, width), dtype=np.int32)
        for i, t in enumerate(flat):
            tok[i, :len(t)] = t
        if self.corpus:                                   # df over this call's (candidate -> reference set) pairs
            count = {}
            for r in refs:
                for k in set(k for t in r for k in ngram_keys(t)):
                    count[k] = count.get(k, 0) + seq_per_img
            keys = np.array(sorted(count), dtype=np.uint64)
            L = math.log(float(N))
            vals = L - np.log(np.maximum(1.0, np.array([count[int(k)] for k in keys], dtype=np.float64)))
        else:
            keys, vals, L = np.zeros(0, np.uint64), np.zeros(0, np.float64), self.log_ref_len
        parts = [start, lens, tok.reshape(-1), keys.view(np.int32), vals.view(np.int32)]
        offs, o = [], 0
        for p in parts:                                   # 8-byte aligned sections of one int32 buffer
            offs.append(o)
            o += (p.size + 1) // 2 * 2
        buf = np.zeros(max(o, 2), dtype=np.int32)
        for p, a in zip(parts, offs):
            buf[a:a + p.size] = p
        dev = torch.from_numpy(buf).pin_memory().to(self.device, non_blocking=True)
        sec = [dev[a:a + p.size] for p, a in zip(parts, offs)]
        if self.corpus:
            df_keys, df_vals, n_df = sec[3].view(torch.int64), sec[4].view(torch.float64), keys.size
        else:
            df_keys, df_vals, n_df = self.df_keys, self.df_vals, int(self.df_keys.numel())
        stride = 128 if width <= 33 else 256
        rec_keys = torch.empty(R, stride, dtype=torch.int64, device=self.device)
        rec_w = torch.empty(R, stride, dtype=torch.float64, device=self.device)
        rec_off = torch.empty(R, ORDERS + 1, dtype=torch.int32, device=self.device)
        rec_meta = torch.empty(R, ORDERS + 1, dtype=torch.float64, device=self.device)
        out = torch.empty(N, dtype=torch.float32, device=self.device)
        out64 = torch.empty(N, dtype=torch.float64, device=self.device) if want64 else None
        lib, st = hip.lib(), hip.stream_ptr()
        hip.check(lib.bofi_cider_refs(hip.ptr(sec[2]), hip.ptr(sec[1]), R, width, hip.ptr(df_keys), hip.ptr(df_vals), n_df, float(L),
                                      hip.ptr(rec_keys), hip.ptr(rec_w), hip.ptr(rec_off), hip.ptr(rec_meta), stride, st), "bofi_cider_refs")
        hip.check(lib.bofi_cider_score(hip.ptr(seq), hip.ptr(cand_len), N, S, seq_per_img, hip.ptr(sec[0]), hip.ptr(df_keys), hip.ptr(df_vals),
                                       n_df, float(L), self.sigma, float(weight), hip.ptr(rec_keys), hip.ptr(rec_w), hip.ptr(rec_off), hip.ptr(rec_meta),
                                       stride, hip.ptr(out), hip.ptr(out64), st), "bofi_cider_score")
        return out, out64

    def score(self, data_gts, seq, seq_per_img: int, weight: float = 1.0, out64: bool = False):
        """get_scores' CIDEr-D term: ``weight`` x CIDEr-D of row j of ``seq`` (device ids [N, S]) against ``data_gts[j // seq_per_img]`` (the
        image's reference rows, any integer arrays).  Returns float32 [N] on seq's device, enqueued on the current stream (and the float64
        scores too with ``out64``)."""
        if seq.device != self.device:
            raise ValueError(f"seq is on {seq.device}, the scorer on {self.device}")
        seq = seq if seq.dtype == torch.int64 and seq.is_contiguous() else seq.to(torch.int64).contiguous()
        refs = [[token_list(row) for row in np.asarray(g).reshape(len(g), -1)] for g in data_gts]
        out, o64 = self._launch(refs, seq, None, int(seq_per_img), weight, out64)
        return (out, o64) if out64 else out

    def compute_score(self, gts, res):
        """The package's contract: ``res`` = [{'image_id', 'caption': [str]}], ``gts`` = {image_id: [str, ...]} with space-separated
        ids (array_to_str's strings).  Returns (mean score, float64 array of the scores)."""
        def ids(s):
            try:
                return [int(t) for t in s.split()]
            except ValueError:
                raise hip.BofiHipError(f"caption {s!r} is not made of ids: the device scorer compares ids (array_to_str's strings)") from None
        cands, refs = [], []
        for r in res:
            assert isinstance(r["caption"], list) and len(r["caption"]) == 1
            cands.append(ids(r["caption"][0]))
            refs.append([ids(s) for s in gts[r["image_id"]]])
        N = len(cands)
        if N == 0:
            return 0.0, np.zeros(0)
        S = max([len(c) for c in cands] + [1])
        seq = np.zeros((N, S), dtype=np.int64)
        for i, c in enumerate(cands):
            seq[i, :len(c)] = c
        lens = torch.tensor([len(c) for c in cands], dtype=torch.int32).to(self.device)
        _, o64 = self._launch(refs, torch.from_numpy(seq).to(self.device), lens, 1, 1.0, True)
        arr = o64.cpu().numpy()
        return float(np.mean(arr)), arr
