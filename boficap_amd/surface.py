"""The surface of evaluated captions on the device (csrc/surface.hip): the bad-ending trim of the reference's ``decode_sequence``
(captioning/utils/misc.py:75-82, ``remove_bad_endings`` of eval_utils.py:139-140), the ``bad_count_rate`` of its ``language_eval``
(eval_utils.py:28-37, 122) and the ``novel_sentences`` / ``vocab_size`` of its sampled captions (eval_utils.py:55-69).

    surface = CaptionSurface.from_vocab(vocab, V, device)          # once: the two word sets as bit tables over the vocabulary
    seq2, length, bad = surface.trim(seq)                          # one launch: kept ids then 0, kept lengths, bad-ending flags
    rate = surface.bad_count_rate(bad)
    train = TrainSentences.from_store(store, image_ixs)            # once: the training sentences, canonical, distinct, sorted, int32 on the device
    stats = sentence_stats(seq2, length, train, V)                 # torch.unique + one launch: {'novel_sentences', 'vocab_size'}

A caption is the ids of a row before the first id <= ``limit`` (the project's 'eval' rule: 0).  The trim removes the trailing run of
``TRIM_WORDS``; a caption made of such words alone (or an empty one) is left as it is, because the reference's loop removes nothing when it
finds no other word.  The bad-ending flag is 1 when the (trimmed) caption is not empty and its last word is one of ``COUNT_WORDS`` -- a second,
different list.  An id outside [0, V) is in neither set.

Difference from the reference: it takes its training sentences as raw token strings from dataset_coco.json; here they are the label file's id
rows, which are UNK-mapped and cut at ``seq_length``, and both sides are compared as ids.  A generated caption that contains UNK can therefore
match a training row here where the reference's strings would not.

``trim_host`` / ``lookup_host`` / ``sentence_stats_host`` restate the kernels in numpy and plain Python, for the tests and for readers.
"""
from __future__ import annotations

import numpy as np
import torch

from . import hip
from .cider import MAX_TOKENS

# captioning/utils/misc.py:17-18 (what decode_sequence strips)
TRIM_WORDS = frozenset(("with", "in", "on", "of", "a", "at", "to", "for", "an", "this", "his", "her", "that", "the"))
# captioning/utils/eval_utils.py:28-29 (what count_bad counts)
COUNT_WORDS = frozenset(("a", "an", "the", "in", "for", "at", "of", "with", "before", "after", "on", "upon", "near", "to", "is", "are", "am"))


def ids_of(vocab, words):
    """The ids (sorted) of ``vocab`` {str(id): word} whose word is in ``words``."""
    words = set(words)
    return sorted(int(k) for k, w in vocab.items() if w in words)


def bit_table(ids, V: int) -> np.ndarray:
    """uint32 [ceil(V / 32)]: bit (id % 32) of word id // 32 set for every id of ``ids``; an id outside [0, V) is an error."""
    V = int(V)
    if V < 1:
        raise ValueError(f"a vocabulary of {V} ids")
    table = np.zeros((V + 31) // 32, dtype=np.uint32)
    for i in ids:
        i = int(i)
        if not 0 <= i < V:
            raise ValueError(f"id {i} is outside the vocabulary 0 .. {V - 1}")
        table[i >> 5] |= np.uint32(1 << (i & 31))
    return table


def _rows(a) -> np.ndarray:
    """``a`` as an int64 array [rows, width]."""
    a = np.asarray(a).astype(np.int64)
    if a.ndim != 2:
        raise ValueError(f"rows of shape {a.shape}: [rows, width] expected")
    return a


def trim_host(seq, trim_ids=None, count_ids=None, limit: int = 0, pad: int = 0):
    """``bofi_caption_trim`` on the host: (kept ids then ``pad`` int64 [rows, S], kept lengths int32 [rows], bad-ending flags int32 [rows]).
    ``trim_ids`` / ``count_ids``: the ids of the two word sets (None: the empty set)."""
    seq = _rows(seq)
    trim, count = set(int(i) for i in trim_ids or ()), set(int(i) for i in count_ids or ())
    out = np.full_like(seq, int(pad))
    length, bad = np.zeros(len(seq), dtype=np.int32), np.zeros(len(seq), dtype=np.int32)
    for r, row in enumerate(seq.tolist()):
        L = next((j for j, v in enumerate(row) if v <= limit), len(row))
        keep = L                                                 # (no good word at all: nothing is removed)
        for j in range(L):                                       # decode_sequence's loop: the first good word from the end
            if row[L - 1 - j] not in trim:
                keep = L - j
                break
        out[r, :keep] = row[:keep]
        length[r] = keep
        bad[r] = 1 if keep > 0 and row[keep - 1] in count else 0
    return out, length, bad


def canonical_rows(rows, limit: int = 0) -> np.ndarray:
    """Integer rows [M, St] in canonical form: the ids before the first id <= ``limit``, then zeros."""
    rows = _rows(rows)
    return np.where(np.cumsum(rows <= limit, axis=1) > 0, 0, rows)


def lookup_host(seq, length, train, V: int):
    """``bofi_sentence_lookup`` on the host: (novel int32 [rows], seen int32 [V]).  ``seq`` [rows, S] canonical rows with their kept ``length``s,
    ``train`` [M, St] canonical training rows (any order)."""
    seq, train = _rows(seq), _rows(train)
    width = max(seq.shape[1], train.shape[1])
    extend = lambda row: tuple(row) + (0,) * (width - len(row))
    known = {extend(row) for row in train.tolist()}
    novel, seen = np.zeros(len(seq), dtype=np.int32), np.zeros(int(V), dtype=np.int32)
    for r, row in enumerate(seq.tolist()):
        n = min(max(int(length[r]), 0), len(row))
        novel[r] = 0 if extend(row[:n] + [0] * (len(row) - n)) in known else 1
        for v in row[:n]:
            if 0 <= v < V:
                seen[v] = 1
    return novel, seen


def sentence_stats_host(seq, length, train, V: int):
    """``sentence_stats`` on the host: the distinct rows among ``seq`` are looked up once each, and the count of novel ones is divided by the
    number of rows BEFORE duplicates were dropped (eval_utils.py:62-64: ``len(novels) / len(preds_n)``)."""
    seq = _rows(seq)
    if len(seq) == 0:
        raise ValueError("no sampled caption: novel_sentences is a share of them")
    both = np.unique(np.concatenate([seq, np.asarray(length, dtype=np.int64).reshape(-1, 1)], axis=1), axis=0)
    novel, seen = lookup_host(both[:, :-1], both[:, -1], train, V)
    return {"novel_sentences": float(int(novel.sum())) / len(seq), "vocab_size": int(seen.sum())}


def _device_of(device):
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def _device_ids(seq, device):
    """``seq`` as contiguous int64 [rows, S] on ``device`` (rows of 1 .. MAX_TOKENS ids)."""
    seq = torch.as_tensor(np.asarray(seq)) if not torch.is_tensor(seq) else seq
    if seq.dim() != 2:
        raise ValueError(f"ids of shape {tuple(seq.shape)}: [rows, S] expected")
    if not 1 <= seq.shape[1] <= MAX_TOKENS:
        raise ValueError(f"rows of {seq.shape[1]} ids: the surface kernels take rows of 1 to {MAX_TOKENS}")
    return seq.to(device, torch.int64).contiguous()


class CaptionSurface:
    """The two word sets of a vocabulary of ``V`` ids as bit tables on the device.  ``trim_ids`` / ``count_ids``: their ids (None or empty: the
    empty set, no table).  ``limit``: a caption is the ids before the first id <= limit."""

    def __init__(self, V: int, trim_ids=None, count_ids=None, device=None, limit: int = 0):
        self.V, self.limit, self.device = int(V), int(limit), _device_of(device)
        if self.V < 1:
            raise ValueError(f"a vocabulary of {self.V} ids")
        self.trim_ids = sorted(set(int(i) for i in trim_ids or ()))
        self.count_ids = sorted(set(int(i) for i in count_ids or ()))
        up = lambda ids: torch.from_numpy(bit_table(ids, self.V).view(np.int32)).to(self.device) if ids else None      # (the bits of uint32 words)
        self.trim_bits, self.count_bits = up(self.trim_ids), up(self.count_ids)

    @classmethod
    def from_vocab(cls, vocab, V: int, device=None, trim_words=None, count_words=None, limit: int = 0):
        """The surface of ``vocab`` {str(id): word}: ``TRIM_WORDS`` / ``COUNT_WORDS`` unless other sets are given."""
        return cls(V, ids_of(vocab, TRIM_WORDS if trim_words is None else trim_words), ids_of(vocab, COUNT_WORDS if count_words is None else count_words),
                   device, limit)

    def trim(self, seq, remove: bool = True, in_place: bool = False):
        """``seq``: ids [rows, S] (device or host, any integer type).  Returns (ids int64 [rows, S]: the kept ids then 0; kept lengths int32
        [rows]; bad-ending flags int32 [rows]) on the device -- one launch on the current stream, no host copy.  ``remove`` False: nothing is
        trimmed (the caption as it stands, in the same form, and its flag).  ``in_place``: the ids are written over ``seq`` (a contiguous int64
        tensor on the surface's device) instead of a new tensor."""
        ids = _device_ids(seq, self.device)
        if in_place and ids is not seq:
            raise ValueError("in_place needs a contiguous int64 tensor on the surface's device")
        rows, S = ids.shape
        out = ids if in_place else torch.empty_like(ids)
        length = torch.empty(rows, dtype=torch.int32, device=self.device)
        bad = torch.empty(rows, dtype=torch.int32, device=self.device)
        hip.check(hip.lib().bofi_caption_trim(hip.ptr(ids), rows, S, self.limit, hip.ptr(self.trim_bits if remove else None), hip.ptr(self.count_bits), self.V,
                                              0, hip.ptr(out), hip.ptr(length), hip.ptr(bad), hip.stream_ptr()), "bofi_caption_trim")
        return out, length, bad

    @staticmethod
    def bad_count_rate(bad) -> float:
        """The share of captions whose flag is set (eval_utils.py:122); a host read-back."""
        bad = bad.detach().cpu().numpy() if torch.is_tensor(bad) else np.asarray(bad)
        if bad.size == 0:
            raise ValueError("no caption: bad_count_rate is a share of them")
        return float(int(bad.astype(np.int64).sum())) / float(bad.size)


class TrainSentences:
    """The training sentences a generated one is looked up in: ``rows`` integer [M, St] (e.g. ``LabelStore.label[...]``) are put in canonical form on
    the host, made distinct and sorted (``np.unique(axis=0)``) and uploaded once as int32."""

    def __init__(self, rows, device=None, limit: int = 0):
        self.device = _device_of(device)
        rows = np.asarray(rows)
        if rows.ndim != 2 or not 1 <= rows.shape[1] <= MAX_TOKENS:
            raise ValueError(f"training rows of shape {rows.shape}: [M, St] with 1 <= St <= {MAX_TOKENS} expected")
        canon = canonical_rows(rows, limit)
        if canon.size and (canon.min() < -2 ** 31 or canon.max() >= 2 ** 31):
            raise ValueError("training ids must fit int32")
        self.host = np.ascontiguousarray(np.unique(canon, axis=0).astype(np.int32)) if len(canon) else canon.astype(np.int32)
        self.M, self.St = int(self.host.shape[0]), int(self.host.shape[1])
        self.rows = torch.from_numpy(self.host).to(self.device)

    @classmethod
    def from_store(cls, store, image_ixs, device=None, limit: int = 0):
        """The sentences of images ``image_ixs`` of a label source with ``gts(ix)`` (``data.LabelStore``)."""
        parts = [np.asarray(store.gts(int(ix))) for ix in image_ixs]
        if not parts:
            raise ValueError("no image: the training sentences of at least one are needed")
        return cls(np.concatenate(parts), device, limit)


def sentence_stats(seq, length, train: TrainSentences, V: int):
    """{'novel_sentences', 'vocab_size'} of sampled captions as eval_utils.py:62-69 computes them: ``seq`` int64 [rows, S] / ``length`` int32 [rows] in
    the canonical form ``CaptionSurface.trim`` returns (pad 0).  The set of generated sentences is ``torch.unique`` over the rows; one
    ``bofi_sentence_lookup`` launch over the distinct rows; one read-back of two sums."""
    ids = _device_ids(seq, train.device)
    rows, S = ids.shape
    if rows == 0:
        raise ValueError("no sampled caption: novel_sentences is a share of them")
    if length.shape != (rows,):
        raise ValueError(f"{tuple(length.shape)} lengths for {rows} rows")
    both = torch.unique(torch.cat([ids, length.to(train.device, torch.int64).reshape(rows, 1)], dim=1), dim=0)
    uniq, ulen = both[:, :S].contiguous(), both[:, S].to(torch.int32).contiguous()
    novel = torch.empty(uniq.shape[0], dtype=torch.int32, device=train.device)
    seen = torch.zeros(int(V), dtype=torch.int32, device=train.device)
    hip.check(hip.lib().bofi_sentence_lookup(hip.ptr(uniq), hip.ptr(ulen), uniq.shape[0], S, hip.ptr(train.rows if train.M else None), train.M, train.St, int(V),
                                             hip.ptr(novel), hip.ptr(seen), hip.stream_ptr()), "bofi_sentence_lookup")
    back = torch.stack([novel.sum(dtype=torch.int64), seen.sum(dtype=torch.int64)]).cpu().tolist()
    return {"novel_sentences": float(back[0]) / rows, "vocab_size": int(back[1])}
