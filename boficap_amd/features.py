"""The feature side of the reference's loader (captioning/data/dataloader.py:24-86 ``HybridLoader``, :164-178 the splits, :326-338 the region
collate, :471-476 the per-image read and ``norm_att_feat``) -> batches on the device.

    store = RegionStore("data/cocobu_att")                       # <id>.npz per image, 10..100 regions each
    index = ImageIndex("data/cocotalk.json")
    batch = RaggedBatch.from_arrays([store.get(str(i)) for i in ids])
    feats, att_len = batch.to_device(out_dtype=torch.bfloat16)   # two copies + one bofi_pack_regions launch, no synchronisation

A batch is staged RAGGED: the images' real rows back to back in pinned memory, in the dtype the files are stored in, plus int32 offsets.  The
zero padding to [B, R, F], the conversion to the compute dtype, the region counts and the optional x / ||x||_2 are one device launch
(csrc/regions.hip), so neither the padding nor a float32 copy of half-precision files crosses the host link.

``RegionStore`` reads what needs nothing beyond numpy and torch: a directory of ``<id>.npz`` / ``<id>.npy`` and a ``.pth`` dictionary.  ``.h5`` and
``.lmdb`` sources are accepted when ``h5py`` / ``lmdbdict`` import; neither module was available where this was written, so THOSE TWO BRANCHES ARE
UNTESTED.

Box features (the loader's ``use_box``, dataloader.py:477-487; ``att_feat_size`` 2053): the boxes come from a second ``RegionStore`` (``input_box_dir``,
``<id>.npy`` of [r, 4] = x1, y1, x2, y2) and the images' sizes from ``ImageIndex.sizes``; a ``BoxRaggedBatch`` stages them beside the rows, and ONE launch
(``bofi_pack_regions_box``) appends x1/w, y1/h, x2/w, y2/h, area/(w h) -- L2-normalised with ``norm_box_feat`` --, sorts every image's regions by box area,
largest first, and pads the width to the engine's ``att_feat_padded`` (2112):

    boxes = RegionStore("data/cocobu_box", ".npy")
    source = RegionSource(store, ids, box_store=boxes, sizes=index.sizes(ixs), norm_box_feat=False)      # source.ragged(i0, i1) -> BoxRaggedBatch
"""
from __future__ import annotations

import io
import json
import os
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from typing import Iterable, Optional, Sequence

import numpy as np
import torch

MAX_WORKERS = 16


class RegionStore:
    """``HybridLoader.get`` + the reshape of the loader's ``__getitem__`` (dataloader.py:472-474): ``get(key)`` -> the image's regions [r, F] in the
    file's dtype (float32 or float16; anything else is cast to float32).  ``in_memory``: every array read is kept and served from memory from then on."""

    def __init__(self, db_path: str, ext: str = ".npz", in_memory: bool = False):
        self.db_path, self.ext, self.in_memory = str(db_path), ext, bool(in_memory)
        self._cache = {} if self.in_memory else None
        self.reads = 0                                           # reads that went to the source (not served from memory)
        if self.db_path.endswith(".lmdb"):
            try:
                from lmdbdict import lmdbdict
                from lmdbdict.methods import DUMPS_FUNC, LOADS_FUNC
            except ImportError as e:
                raise ImportError("reading a .lmdb feature source needs the module lmdbdict") from e
            self.kind = "lmdb"
            self._db = lmdbdict(self.db_path, unsafe=True)
            self._db._key_dumps, self._db._value_loads = DUMPS_FUNC["ascii"], LOADS_FUNC["identity"]
        elif self.db_path.endswith(".pth"):                      # a key -> array dictionary; ext is ignored
            self.kind = "pth"
            try:                                                 # tensors load without unpickling arbitrary objects; a dictionary of numpy arrays needs the full
                self._db = torch.load(self.db_path, map_location="cpu", weights_only=True)       # unpickler: such a file must come from a source the caller
            except Exception:                                    # trusts, exactly as the reference's torch.load(db_path) assumes
                self._db = torch.load(self.db_path, map_location="cpu", weights_only=False)
        elif self.db_path.endswith("h5"):
            try:
                import h5py
            except ImportError as e:
                raise ImportError("reading a .h5 feature source needs the module h5py") from e
            self.kind = "h5"
            self._db = h5py.File(self.db_path, "r")
        else:
            self.kind = "dir"
            if ext not in (".npz", ".npy"):
                raise ValueError(f"a feature directory holds .npz or .npy files, not {ext!r}")

    def _decode(self, f):
        a = np.load(f)
        if self.ext == ".npy":
            return a
        with a:
            return a["feat"] if "feat" in a.files else a["z"]     # ('z': the key of the reference's cocotest_bu files)

    def _read(self, key: str):
        if self.kind == "dir":
            path = os.path.join(self.db_path, key + self.ext)
            if not os.path.exists(path):
                raise FileNotFoundError(f"no region features for image {key!r}: {path} does not exist")
            return self._decode(path)
        if self.kind == "pth":
            if key not in self._db:
                raise KeyError(f"no region features for image {key!r} in {self.db_path}")
            a = self._db[key]
            return a.numpy() if torch.is_tensor(a) else np.asarray(a)
        if self.kind == "h5":
            if key not in self._db:
                raise KeyError(f"no region features for image {key!r} in {self.db_path}")
            return np.asarray(self._db[key])
        try:
            raw = self._db[key]
        except KeyError:
            raise KeyError(f"no region features for image {key!r} in {self.db_path}") from None
        return self._decode(io.BytesIO(raw))

    def get(self, key) -> np.ndarray:
        key = str(key)
        if self._cache is not None and key in self._cache:
            return self._cache[key]
        a = self._read(key)
        self.reads += 1
        if a.dtype not in (np.float32, np.float16):
            a = a.astype(np.float32)
        a = np.ascontiguousarray(a.reshape(-1, a.shape[-1]) if a.ndim >= 1 and a.size else a.reshape(0, a.shape[-1] if a.ndim else 0))
        if a.shape[0] == 0:
            raise ValueError(f"image {key!r} has no region rows")
        if self._cache is not None:
            self._cache[key] = a
        return a


class ImageIndex:
    """The image list of the preprocessing's json (``images[*]['id']``) and the loader's split assignment (dataloader.py:164-178): an image without a
    split is in all three, 'restval' (any other label) goes to train unless ``train_only``.  Image i of the json is image i of the label file."""

    def __init__(self, input_json, train_only: int = 0):
        if isinstance(input_json, (str, os.PathLike)):
            with open(input_json) as f:
                input_json = json.load(f)
        self.images = input_json["images"]
        self.ids = [img["id"] for img in self.images]
        self.split_ix = {"train": [], "val": [], "test": []}
        for ix, img in enumerate(self.images):
            split = img.get("split")
            if split is None:
                for s in self.split_ix.values():
                    s.append(ix)
            elif split in self.split_ix:
                self.split_ix[split].append(ix)
            elif int(train_only) == 0:
                self.split_ix["train"].append(ix)

    def __len__(self):
        return len(self.images)

    def keys(self, ixs: Sequence[int]):
        """The store keys (``str(id)``, dataloader.py:472) of images ``ixs``."""
        return [str(self.ids[int(i)]) for i in ixs]

    def sizes(self, ixs: Sequence[int]) -> np.ndarray:
        """int32 [n, 2] = (width, height) of images ``ixs`` (dataloader.py:481: the divisors of the box features)."""
        out = np.empty((len(ixs), 2), np.int32)
        for n, i in enumerate(ixs):
            img = self.images[int(i)]
            for c, name in enumerate(("width", "height")):
                if name not in img:
                    raise KeyError(f"image {img['id']!r} of the json has no {name!r}: box features are divided by the image's width and height")
                out[n, c] = int(img[name])
        return out


def _pinned(shape, dtype):
    return torch.empty(shape, dtype=dtype, pin_memory=torch.cuda.is_available())


class RaggedBatch:
    """One batch as ``rows`` [sum len, F] (pinned host memory, the files' dtype) and ``offsets`` (host int32 [B + 1]).  ``norm``: the loader's
    ``norm_att_feat``, applied by the device launch."""

    def __init__(self, rows: torch.Tensor, offsets: torch.Tensor, norm: bool = False):
        if rows.dim() != 2 or offsets.dtype != torch.int32 or offsets.dim() != 1 or offsets.numel() < 2:
            raise ValueError("rows [n, F] and int32 offsets [B + 1] expected")
        if rows.size(1) % 8 != 0:
            raise ValueError(f"F = {rows.size(1)} is not a multiple of 8: the device launch moves 16-byte vectors (box features, F = 2053, are not supported)")
        self.rows, self.offsets, self.norm = rows, offsets, bool(norm)
        lens = offsets[1:] - offsets[:-1]
        self.B, self.F = int(offsets.numel() - 1), int(rows.size(1))
        self.max_len, self.min_len = int(lens.max()), int(lens.min())

    @classmethod
    def from_arrays(cls, arrays: Sequence[np.ndarray], norm: bool = False) -> "RaggedBatch":
        """Images' region arrays [r_i, F] (float32 / float16) -> one staged batch; images of mixed dtype are cast to float32."""
        if not arrays:
            raise ValueError("an empty batch")
        F = arrays[0].shape[1]
        if any(a.ndim != 2 or a.shape[1] != F for a in arrays):
            raise ValueError(f"every image must be [r, {F}]")
        kinds = {a.dtype for a in arrays}
        dtype = np.dtype(np.float16) if kinds == {np.dtype(np.float16)} else np.dtype(np.float32)
        offsets = _pinned((len(arrays) + 1,), torch.int32)
        off = np.zeros(len(arrays) + 1, np.int64)
        np.cumsum([a.shape[0] for a in arrays], out=off[1:])
        if off[-1] >= 2 ** 31:
            raise ValueError("a batch of 2^31 region rows or more")
        offsets.numpy()[:] = off
        rows = _pinned((int(off[-1]), F), torch.float16 if dtype == np.float16 else torch.float32)
        view = rows.numpy()
        for a, o in zip(arrays, off[:-1]):
            view[o:o + a.shape[0]] = a                           # (the one host pass over the bytes; casts a mixed batch's float16 images)
        return cls(rows, offsets, norm)

    @property
    def equal_lengths(self) -> bool:
        return self.max_len == self.min_len

    @property
    def out_F(self) -> int:
        """Columns of the device launch's output (``F``; a ``BoxRaggedBatch`` widens it)."""
        return self.F

    def lengths(self) -> np.ndarray:
        return np.diff(self.offsets.numpy())

    def to_device(self, out: Optional[torch.Tensor] = None, out_dtype: torch.dtype = torch.bfloat16, out_R: Optional[int] = None, norm: Optional[bool] = None,
                  stream: Optional["torch.cuda.Stream"] = None, device=None):
        """One asynchronous copy of ``rows``, one of ``offsets`` and one ``bofi_pack_regions`` launch on ``stream`` (default: the current one); no
        synchronisation.  Returns (feats [B, out_R, F] in ``out_dtype`` -- ``out`` itself when given --, att_len int32 [B]); ``att_len`` is None when
        every image has ``out_R`` regions, as the loader returns ``att_masks=None`` then.  ``out_R`` defaults to the longest image; ``norm`` to the batch's."""
        if out is not None:
            out_R, out_dtype, device = out.size(1), out.dtype, out.device
        out_R = self.max_len if out_R is None else int(out_R)
        dev = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        with torch.cuda.device(dev), torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(dev)):
            rows = torch.empty(self.rows.shape, dtype=self.rows.dtype, device=dev)
            rows.copy_(self.rows, non_blocking=True)
            offsets = torch.empty(self.B + 1, dtype=torch.int32, device=dev)
            offsets.copy_(self.offsets, non_blocking=True)
            if out is None:
                out = torch.empty(self.B, out_R, self.out_F, dtype=out_dtype, device=dev)
            att_len = torch.empty(self.B, dtype=torch.int32, device=dev)
            self.pack(rows, offsets, out, self.norm if norm is None else norm, att_len, dev)
        return out, (None if self.equal_lengths and self.max_len == out_R else att_len)

    def pack(self, rows, offsets, out, norm, att_len, dev):
        """The device launch on the current stream: ``rows`` / ``offsets`` are the device copies of this batch's arrays."""
        from . import hip
        hip.pack_regions(rows, offsets, self.offsets, out, norm=norm, att_len=att_len)


class BoxRaggedBatch(RaggedBatch):
    """A batch of the loader's use_box mode (dataloader.py:477-487): besides ``rows`` [sum len, F] and ``offsets`` it carries ``boxes`` (pinned float32
    [sum len, 4]: x1, y1, x2, y2 in pixels, one per row) and ``wh`` (host int32 [B, 2]: width, height).  The device launch (``bofi_pack_regions_box``)
    appends the five geometry columns -- L2-normalised when ``norm_box`` --, sorts every image's rows by box area, largest first, and pads the width to
    ``F_out`` (default: F + 5 rounded up to 64 -- the engine's ``att_feat_padded``: 2112 for 2048 + 5), so ``to_device`` returns [B, out_R, F_out]."""

    def __init__(self, rows, offsets, boxes, wh, norm: bool = False, norm_box: bool = False, F_out: Optional[int] = None):
        super().__init__(rows, offsets, norm)
        if boxes.dtype != torch.float32 or boxes.dim() != 2 or tuple(boxes.shape) != (rows.size(0), 4):
            raise ValueError(f"boxes must be float32 [{rows.size(0)}, 4], one (x1, y1, x2, y2) per region row; got {boxes.dtype} {tuple(boxes.shape)}")
        if wh.dtype != torch.int32 or tuple(wh.shape) != (self.B, 2):
            raise ValueError(f"wh must be int32 [{self.B}, 2] (width, height), one per image")
        if int(wh.min()) < 1:
            raise ValueError("every image's width and height must be >= 1")
        self.boxes, self.wh, self.norm_box = boxes, wh, bool(norm_box)
        self.F_out = -(-(self.F + 5) // 64) * 64 if F_out is None else int(F_out)
        if self.F_out % 8 != 0 or self.F_out < self.F + 5:
            raise ValueError(f"F_out = {self.F_out}: a multiple of 8 that is at least F + 5 = {self.F + 5} expected")

    @classmethod
    def from_arrays(cls, arrays, boxes, sizes, norm: bool = False, norm_box: bool = False, F_out: Optional[int] = None) -> "BoxRaggedBatch":
        """Images' region arrays [r_i, F], their boxes [r_i, 4] (cast to float32) and ``sizes`` [B, 2] = (width, height) -> one staged batch."""
        base = RaggedBatch.from_arrays(arrays, norm)
        if len(boxes) != len(arrays) or any(np.ndim(q) != 2 or q.shape != (a.shape[0], 4) for q, a in zip(boxes, arrays)):
            raise ValueError("every image needs boxes [r, 4], one (x1, y1, x2, y2) per region row")
        staged = _pinned((base.rows.size(0), 4), torch.float32)
        view, o = staged.numpy(), 0
        for q in boxes:
            view[o:o + q.shape[0]] = q
            o += q.shape[0]
        wh = _pinned((base.B, 2), torch.int32)
        wh.numpy()[:] = np.asarray(sizes, np.int32).reshape(base.B, 2)
        return cls(base.rows, base.offsets, staged, wh, norm, norm_box, F_out)

    @property
    def out_F(self) -> int:
        return self.F_out

    def pack(self, rows, offsets, out, norm, att_len, dev):
        from . import hip
        boxes = torch.empty(self.boxes.shape, dtype=torch.float32, device=dev)
        boxes.copy_(self.boxes, non_blocking=True)
        wh = torch.empty(self.B, 2, dtype=torch.int32, device=dev)
        wh.copy_(self.wh, non_blocking=True)
        hip.pack_regions_box(rows, boxes, wh, self.wh, offsets, self.offsets, out, norm_att=norm, norm_box=self.norm_box, att_len=att_len)


def att_masks_of(att_len: Optional[torch.Tensor], R: int):
    """The loader's float32 mask [B, R] (dataloader.py:333-335) of region counts on the device; None stays None."""
    if att_len is None:
        return None
    return (torch.arange(R, device=att_len.device)[None, :] < att_len[:, None]).to(torch.float32)


class RegionSource:
    """The images ``ids`` of ``store`` as ``eval_utils.eval_split`` and ``DecodePipeline`` read them: ``len()`` and ``ragged(i0, i1)``.  ``box_store`` and
    ``sizes`` (int32 [len(ids), 2], ``ImageIndex.sizes``): the loader's use_box mode -- ``ragged`` then returns ``BoxRaggedBatch``es."""

    def __init__(self, store: RegionStore, ids: Sequence, norm_att_feat: bool = False, box_store: Optional[RegionStore] = None, sizes=None, norm_box_feat: bool = False):
        self.store, self.keys, self.norm = store, [str(i) for i in ids], bool(norm_att_feat)
        self.box_store, self.norm_box = box_store, bool(norm_box_feat)
        self.sizes = _checked_sizes(box_store, sizes, len(self.keys))

    def __len__(self):
        return len(self.keys)

    def ragged(self, i0: int, i1: int) -> RaggedBatch:
        return _stage(self.store, self.keys[i0:i1], self.norm, self.box_store, None if self.sizes is None else self.sizes[i0:i1], self.norm_box)


def _checked_sizes(box_store, sizes, n):
    if box_store is None:
        return None
    if sizes is None:
        raise ValueError("box features need the images' sizes: sizes = ImageIndex.sizes(ixs)")
    sizes = np.ascontiguousarray(sizes, np.int32)
    if n is not None and sizes.shape != (n, 2):
        raise ValueError(f"sizes must be int32 [{n}, 2] (width, height), one row per image; got {sizes.shape}")
    return sizes


def _stage(store, keys, norm, box_store=None, sizes=None, norm_box=False):
    arrays = [store.get(k) for k in keys]
    if box_store is None:
        return RaggedBatch.from_arrays(arrays, norm)
    return BoxRaggedBatch.from_arrays(arrays, [box_store.get(k).astype(np.float32, copy=False) for k in keys], sizes, norm, norm_box)


class RegionFeeder:
    """A bounded prefetch: ``workers`` threads (at most 16) read the images of ``index_batches`` -- an iterable of sequences of store keys, consumed
    lazily -- and stage ``RaggedBatch``es up to ``ahead`` batches before the consumer.  Iterating yields the batches in input order.  The threads
    read files and fill host memory; they enqueue nothing on the device, and no further process is started.  They do call into the HIP runtime in one way:
    a batch's pinned memory comes from torch's caching host allocator, so the first batch of each size is a (slow) page-locking allocation made on a
    worker thread; later batches reuse the cached blocks.  ``box_store`` and ``sizes`` -- a mapping from store key to (width, height) -- : the loader's
    use_box mode, the batches are ``BoxRaggedBatch``es."""

    def __init__(self, store: RegionStore, index_batches: Iterable[Sequence], workers: int = 4, ahead: Optional[int] = None, norm_att_feat: bool = False,
                 box_store: Optional[RegionStore] = None, sizes=None, norm_box_feat: bool = False):
        self.store, self.batches, self.norm = store, index_batches, bool(norm_att_feat)
        self.box_store, self.sizes, self.norm_box = box_store, sizes, bool(norm_box_feat)
        if box_store is not None and sizes is None:
            raise ValueError("box features need the images' sizes: sizes = {store key: (width, height)}")
        self.workers = max(1, min(int(workers), MAX_WORKERS))
        self.ahead = max(1, int(ahead)) if ahead is not None else self.workers + 1

    def _stage(self, keys):
        sizes = None if self.box_store is None else np.array([self.sizes[k] for k in keys], np.int32).reshape(len(keys), 2)
        return _stage(self.store, keys, self.norm, self.box_store, sizes, self.norm_box)

    def __iter__(self):
        pool = ThreadPoolExecutor(max_workers=self.workers, thread_name_prefix="region-feeder")
        queue, source = deque(), iter(self.batches)
        try:
            while True:
                while len(queue) < self.ahead:
                    keys = next(source, None)
                    if keys is None:
                        break
                    queue.append(pool.submit(self._stage, list(keys)))
                if not queue:
                    return
                yield queue.popleft().result()
        finally:
            for f in queue:
                f.cancel()
            pool.shutdown(wait=True)
