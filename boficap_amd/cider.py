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


class DfTable:
    """The document frequencies of ``df``: a df pickle's sorted keys and values on the device, or ``df='corpus'`` (counted per call)."""

    def __init__(self, df, device):
        self.corpus = df == "corpus"
        self.keys = self.vals = None
        self.log_ref_len = 0.0
        if not self.corpus:
            path = resolve_df(df)
            if path is None:
                raise FileNotFoundError(f"no document-frequency file for cached_tokens={df!r} (neither a file nor data/{df}.p)")
            keys, vals, self.log_ref_len = load_df(path)
            self.keys = torch.from_numpy(keys.view(np.int64)).to(device)
            self.vals = torch.from_numpy(vals).to(device)


class Packed:
    """One call's references (and its corpus df) packed for the kernels.  On the host (``pack_host``): ``parts`` = [start int32 [images + 1]
    (first reference of each image), lens int32 [R] (token counts), tok int32 [R * width], df keys, df values (as int32 words)] at
    8-byte aligned offsets ``offs`` of one int32 buffer ``buf``.  After ``upload``: the same sections as device tensors ``start``, ``lens``,
    ``tok`` and the table the kernels read, ``df_keys`` / ``df_vals`` / ``n_df`` / ``L``."""


def pack_host(refs, N: int, S: int, seq_per_img: int, df: "DfTable | None") -> Packed:
    """Check the references ``refs`` (per image, token lists) of N candidates of S ids, seq_per_img per image, and pack them (and the corpus df
    of ``df='corpus'``) into one int32 buffer.  ``df`` None: no df table (n_df 0, L 0)."""
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
    corpus = df is not None and df.corpus
    if corpus:                                            # df over this call's (candidate -> reference set) pairs
        count = {}
        for r in refs:
            for k in set(k for t in r for k in ngram_keys(t)):
                count[k] = count.get(k, 0) + seq_per_img
        keys = np.array(sorted(count), dtype=np.uint64)
        L = math.log(float(N))
        vals = L - np.log(np.maximum(1.0, np.array([count[int(k)] for k in keys], dtype=np.float64)))
    else:
        keys, vals, L = np.zeros(0, np.uint64), np.zeros(0, np.float64), df.log_ref_len if df is not None else 0.0
    parts = [start, lens, tok.reshape(-1), keys.view(np.int32), vals.view(np.int32)]
    offs, o = [], 0
    for p in parts:                                       # 8-byte aligned sections of one int32 buffer
        offs.append(o)
        o += (p.size + 1) // 2 * 2
    buf = np.zeros(max(o, 2), dtype=np.int32)
    for p, a in zip(parts, offs):
        buf[a:a + p.size] = p
    pk = Packed()
    pk.R, pk.width, pk.L, pk.corpus, pk.parts, pk.offs, pk.buf = R, width, float(L), corpus, parts, offs, buf
    pk.stride = 128 if width <= 33 else 256
    return pk


def upload(pk: Packed, device, df: "DfTable | None") -> Packed:
    """The packed buffer to ``device`` with one pinned copy on the current stream, and the device views of its sections."""
    dev = torch.from_numpy(pk.buf).pin_memory().to(device, non_blocking=True)
    sec = [dev[a:a + p.size] for p, a in zip(pk.parts, pk.offs)]
    pk.start, pk.lens, pk.tok = sec[0], sec[1], sec[2]
    if pk.corpus:
        pk.df_keys, pk.df_vals, pk.n_df = sec[3].view(torch.int64), sec[4].view(torch.float64), int(pk.parts[3].size // 2)
    elif df is not None:
        pk.df_keys, pk.df_vals, pk.n_df = df.keys, df.vals, int(df.keys.numel())
    else:
        pk.df_keys, pk.df_vals, pk.n_df = None, None, 0
    return pk


def pack_references(refs, N: int, S: int, seq_per_img: int, device, df: "DfTable | None") -> Packed:
    """pack_host, then upload."""
    return upload(pack_host(refs, N, S, seq_per_img, df), device, df)


def id_lists(captions):
    """Space-separated id strings (array_to_str's) as id lists."""
    def ids(s):
        try:
            return [int(t) for t in s.split()]
        except ValueError:
            raise hip.BofiHipError(f"caption {s!r} is not made of ids: the device scorer compares ids (array_to_str's strings)") from None
    return [ids(s) for s in captions]


def as_device_ids(seq, device):
    """seq as contiguous int64 on the scorer's device (no copy if it already is)."""
    if seq.device != device:
        raise ValueError(f"seq is on {seq.device}, the scorer on {device}")
    return seq if seq.dtype == torch.int64 and seq.is_contiguous() else seq.to(torch.int64).contiguous()


def host_candidates(cands, device):
    """Host id lists as (int64 [N, S] zero-padded, int32 [N] token counts) on the device."""
    S = max([len(c) for c in cands] + [1])
    seq = np.zeros((len(cands), S), dtype=np.int64)
    for i, c in enumerate(cands):
        seq[i, :len(c)] = c
    return torch.from_numpy(seq).to(device), torch.tensor([len(c) for c in cands], dtype=torch.int32).to(device)


def reference_lists(data_gts):
    """get_scores' data_gts (per image, reference rows as integer arrays) as token lists."""
    return [[token_list(row) for row in np.asarray(g).reshape(len(g), -1)] for g in data_gts]


class _Bound:
    """``score_fn(seq) -> [N]`` of XETrainer.rl_step for one batch's references (``on_device``: the trainer hands it the device ids)."""
    on_device = True

    def __init__(self, scorer, data_gts, seq_per_img, **kw):
        self.scorer, self.data_gts, self.seq_per_img, self.kw = scorer, data_gts, seq_per_img, kw

    def __call__(self, seq):
        return self.scorer.score(self.data_gts, seq, self.seq_per_img, **self.kw)


class CiderD:
    """pyciderevalcap's ``CiderD(n=4, sigma=6.0, df=...)`` on the device.  ``on_device``: ``score`` takes and returns device tensors."""
    on_device = True

    def __init__(self, df="corpus", n: int = 4, sigma: float = 6.0, device=None):
        if n != ORDERS:
            raise ValueError(f"CIDEr-D is built for n = {ORDERS}")
        self.sigma = float(sigma)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.df = DfTable(df, self.device)
        self.corpus = self.df.corpus

    def bind(self, data_gts, seq_per_img: int, weight: float = 1.0):
        """The scorer of one batch as a ``score_fn(seq)`` for XETrainer.rl_step."""
        return _Bound(self, data_gts, seq_per_img, weight=weight)

    def records(self, pk):
        """The records of uploaded references ``pk`` (``upload``) by bofi_cider_refs, enqueued on the current stream: ``(pk, tensors)`` for
        ``_launch(records=...)`` -- a caller that scores many candidate sets against the same references builds them once."""
        R, stride = pk.R, pk.stride
        rec_keys = torch.empty(R, stride, dtype=torch.int64, device=self.device)
        rec_w = torch.empty(R, stride, dtype=torch.float64, device=self.device)
        rec_off = torch.empty(R, ORDERS + 1, dtype=torch.int32, device=self.device)
        rec_meta = torch.empty(R, ORDERS + 1, dtype=torch.float64, device=self.device)
        hip.check(hip.lib().bofi_cider_refs(hip.ptr(pk.tok), hip.ptr(pk.lens), R, pk.width, hip.ptr(pk.df_keys), hip.ptr(pk.df_vals), pk.n_df, pk.L,
                                            hip.ptr(rec_keys), hip.ptr(rec_w), hip.ptr(rec_off), hip.ptr(rec_meta), stride, hip.stream_ptr()),
                  "bofi_cider_refs")
        return pk, (rec_keys, rec_w, rec_off, rec_meta)

    def _launch(self, refs, seq, cand_len, seq_per_img, weight, want64, records=None):
        """``records``: what ``records()`` returned for these references -- no packing and no refs kernel then (``refs`` is not read)."""
        N, S = seq.shape
        pk, (rec_keys, rec_w, rec_off, rec_meta) = records if records is not None else self.records(
            pack_references(refs, N, S, seq_per_img, self.device, self.df))
        out = torch.empty(N, dtype=torch.float32, device=self.device)
        out64 = torch.empty(N, dtype=torch.float64, device=self.device) if want64 else None
        hip.check(hip.lib().bofi_cider_score(hip.ptr(seq), hip.ptr(cand_len), N, S, seq_per_img, hip.ptr(pk.start), hip.ptr(pk.df_keys), hip.ptr(pk.df_vals),
                                             pk.n_df, pk.L, self.sigma, float(weight), hip.ptr(rec_keys), hip.ptr(rec_w), hip.ptr(rec_off), hip.ptr(rec_meta),
                                             pk.stride, hip.ptr(out), hip.ptr(out64), hip.stream_ptr()), "bofi_cider_score")
        return out, out64

    def score(self, data_gts, seq, seq_per_img: int, weight: float = 1.0, out64: bool = False):
        """get_scores' CIDEr-D term: ``weight`` x CIDEr-D of row j of ``seq`` (device ids [N, S]) against ``data_gts[j // seq_per_img]`` (the
        image's reference rows, any integer arrays).  Returns float32 [N] on seq's device, enqueued on the current stream (and the float64
        scores too with ``out64``)."""
        seq = as_device_ids(seq, self.device)
        out, o64 = self._launch(reference_lists(data_gts), seq, None, int(seq_per_img), weight, out64)
        return (out, o64) if out64 else out

    def compute_score(self, gts, res):
        """The package's contract: ``res`` = [{'image_id', 'caption': [str]}], ``gts`` = {image_id: [str, ...]} with space-separated
        ids (array_to_str's strings).  Returns (mean score, float64 array of the scores)."""
        cands, refs = [], []
        for r in res:
            assert isinstance(r["caption"], list) and len(r["caption"]) == 1
            cands.append(id_lists(r["caption"])[0])
            refs.append(id_lists(gts[r["image_id"]]))
        N = len(cands)
        if N == 0:
            return 0.0, np.zeros(0)
        seq, lens = host_candidates(cands, self.device)
        _, o64 = self._launch(refs, seq, lens, 1, 1.0, True)
        arr = o64.cpu().numpy()
        return float(np.mean(arr)), arr
