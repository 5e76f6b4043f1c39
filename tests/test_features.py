"""The feature side of the loader on the host (boficap_amd/features.py): the per-image feature sources, the json's splits, ragged staging, the
prefetching feeder, the new entry point's declaration and the CLIs' argument errors.  No GPU."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from boficap_amd import features
from boficap_amd.features import ImageIndex, RaggedBatch, RegionFeeder, RegionSource, RegionStore

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 16


def image(rng, r, dtype=np.float32):
    return rng.standard_normal((r, F)).astype(dtype)


@pytest.fixture()
def npz_dir(tmp_path):
    rng = np.random.default_rng(0)
    arrays = {"11": image(rng, 3), "12": image(rng, 7, np.float16), "13": image(rng, 5), "14": image(rng, 4).reshape(1, 4, F), "15": image(rng, 2).astype(np.float64)}
    for k, a in arrays.items():
        np.savez(tmp_path / f"{k}.npz", **{("z" if k == "13" else "feat"): a})
    np.savez(tmp_path / "16.npz", feat=np.zeros((0, F), np.float32))
    return tmp_path, arrays


def test_store_reads_a_directory_of_npz(npz_dir):
    d, arrays = npz_dir
    store = RegionStore(str(d))
    for k in ("11", "12", "13"):                                  # key 'feat', float16 kept, key 'z'
        got = store.get(k)
        assert got.dtype == arrays[k].dtype and np.array_equal(got, arrays[k]) and got.flags.c_contiguous
    assert store.get(11).shape == (3, F)                           # (keys are str(id))
    got = store.get("14")                                          # [1, r, F] -> [r, F]
    assert got.shape == (4, F) and np.array_equal(got, arrays["14"][0])
    got = store.get("15")                                          # neither float32 nor float16: cast to float32
    assert got.dtype == np.float32 and np.array_equal(got, arrays["15"].astype(np.float32))
    with pytest.raises(FileNotFoundError, match="999"):
        store.get("999")
    with pytest.raises(ValueError, match="16"):
        store.get("16")                                            # an image without rows


def test_store_reads_npy_and_pth(tmp_path):
    rng = np.random.default_rng(1)
    a, b = image(rng, 6), image(rng, 2, np.float16)
    np.save(tmp_path / "7.npy", a)
    store = RegionStore(str(tmp_path), ".npy")
    assert np.array_equal(store.get("7"), a)
    torch.save({"7": a, "8": torch.from_numpy(b).reshape(1, 2, F)}, tmp_path / "feats.pth")
    store = RegionStore(str(tmp_path / "feats.pth"))
    assert np.array_equal(store.get("7"), a)
    got = store.get("8")
    assert got.dtype == np.float16 and np.array_equal(got, b)
    with pytest.raises(KeyError, match="31"):
        store.get("31")
    with pytest.raises(ValueError):
        RegionStore(str(tmp_path), ".txt")


def test_in_memory_store_serves_the_second_read_from_memory(npz_dir):
    d, arrays = npz_dir
    store = RegionStore(str(d), in_memory=True)
    first = store.get("11")
    os.remove(d / "11.npz")
    assert store.get("11") is first and store.reads == 1
    plain = RegionStore(str(d))
    plain.get("12"), plain.get("12")
    assert plain.reads == 2


@pytest.mark.parametrize("path, module", [("feats.h5", "h5py"), ("feats.lmdb", "lmdbdict")])
def test_h5_and_lmdb_name_their_module_when_it_is_missing(tmp_path, monkeypatch, path, module):
    monkeypatch.setitem(sys.modules, module, None)                 # (an import of it now fails, installed or not)
    with pytest.raises(ImportError, match=module):
        RegionStore(str(tmp_path / path))


def test_image_index_assigns_the_splits(tmp_path):
    images = [{"id": 100 + i, "split": s} for i, s in enumerate(["train", "val", "test", "restval", "train", "val"])] + [{"id": 900}]
    with open(tmp_path / "talk.json", "w") as f:
        json.dump({"images": images, "ix_to_word": {}}, f)
    ix = ImageIndex(str(tmp_path / "talk.json"))
    assert len(ix) == 7 and ix.ids == [100, 101, 102, 103, 104, 105, 900]
    assert ix.split_ix == {"train": [0, 3, 4, 6], "val": [1, 5, 6], "test": [2, 6]}       # restval -> train; no split: all three
    only = ImageIndex({"images": images}, train_only=1)
    assert only.split_ix == {"train": [0, 4, 6], "val": [1, 5, 6], "test": [2, 6]}
    assert ix.keys([1, 5]) == ["101", "105"]


def test_ragged_batch_rows_and_offsets():
    rng = np.random.default_rng(2)
    arrays = [image(rng, r) for r in (1, 7, 36, 2)]
    rb = RaggedBatch.from_arrays(arrays)
    assert rb.offsets.dtype == torch.int32 and rb.offsets.tolist() == [0, 1, 8, 44, 46]
    assert rb.rows.dtype == torch.float32 and tuple(rb.rows.shape) == (46, F) and np.array_equal(rb.rows.numpy(), np.concatenate(arrays))
    assert (rb.B, rb.F, rb.max_len, rb.equal_lengths, rb.norm) == (4, F, 36, False, False)
    assert rb.lengths().tolist() == [1, 7, 36, 2]
    half = [a.astype(np.float16) for a in arrays]
    assert RaggedBatch.from_arrays(half).rows.dtype == torch.float16
    mixed = RaggedBatch.from_arrays([half[0], arrays[1], half[2], arrays[3]])          # mixed: promoted to float32
    assert mixed.rows.dtype == torch.float32
    assert np.array_equal(mixed.rows.numpy(), np.concatenate([half[0].astype(np.float32), arrays[1], half[2].astype(np.float32), arrays[3]]))
    same = RaggedBatch.from_arrays([image(rng, 5), image(rng, 5)], norm=True)
    assert same.equal_lengths and same.max_len == 5 and same.norm
    with pytest.raises(ValueError):
        RaggedBatch.from_arrays([arrays[0], arrays[1][:, :8]])
    with pytest.raises(ValueError):
        RaggedBatch.from_arrays([])


@pytest.mark.parametrize("workers", [1, 4])
def test_feeder_yields_the_batches_in_order(tmp_path, workers):
    rng = np.random.default_rng(3)
    arrays = {str(i): image(rng, int(rng.integers(1, 9)), np.float16 if i % 3 == 0 else np.float32) for i in range(23)}
    for k, a in arrays.items():
        np.savez(tmp_path / f"{k}.npz", feat=a)
    store = RegionStore(str(tmp_path))
    order = [str(i) for i in rng.permutation(23)] * 2
    key_batches = [order[i:i + 4] for i in range(0, len(order), 4)]
    got = list(RegionFeeder(store, iter(key_batches), workers=workers, norm_att_feat=True))
    assert len(got) == len(key_batches)
    for rb, keys in zip(got, key_batches):
        direct = RaggedBatch.from_arrays([store.get(k) for k in keys])
        assert rb.norm and rb.rows.dtype == direct.rows.dtype and torch.equal(rb.rows, direct.rows) and torch.equal(rb.offsets, direct.offsets)
    src = RegionSource(store, list(range(23)))
    assert len(src) == 23 and torch.equal(src.ragged(4, 7).rows, RaggedBatch.from_arrays([arrays[str(i)] for i in (4, 5, 6)]).rows)


def test_feeder_workers_are_clamped_and_leave_with_the_iterator(tmp_path):
    import threading
    np.savez(tmp_path / "1.npz", feat=np.ones((2, F), np.float32))
    store = RegionStore(str(tmp_path))
    assert RegionFeeder(store, [], workers=64).workers == 16 == features.MAX_WORKERS
    assert RegionFeeder(store, [], workers=0).workers == 1
    it = iter(RegionFeeder(store, (["1"] for _ in range(1000)), workers=3))
    next(it), next(it)
    it.close()                                                     # a consumer that stops early: the threads are joined
    assert not [t for t in threading.enumerate() if t.name.startswith("region-feeder")]
    with pytest.raises(FileNotFoundError, match="404"):            # a worker's error reaches the consumer
        list(RegionFeeder(store, [["1"], ["404"]], workers=2))


def test_entry_point_is_declared_bound_and_built():
    from boficap_amd import build, hip
    assert "regions.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "regions.hip"))
    header = open(os.path.join(ROOT, "include", "boficap_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    found = re.findall(r"\bint\s+bofi_pack_regions\s*\(([^;]*)\)\s*;", code)
    assert len(found) == 1 and found[0].count(",") + 1 == len(hip.SIGNATURES["bofi_pack_regions"][1]) == 12
    assert "#define BOFI_DT_F16 2" in header and hip.DT_F16 == 2
    assert hip.ABI_VERSION == 5                                    # (5: the decode calls take their options as a record)


@pytest.mark.parametrize("tool, extra, message", [
    ("eval.py", ["--input_att_dir", "feats"], "--input_json"),
    ("eval.py", ["--input_att_dir", "feats", "--input_json", "talk.json", "--use_box", "1"], "F = 2053"),
    ("train.py", ["--input_att_dir", "feats"], "--input_json"),
    ("train.py", ["--input_att_dir", "feats", "--input_json", "talk.json"], "--input_label_h5"),
    ("train.py", ["--input_att_dir", "feats", "--input_json", "talk.json", "--input_label_h5", "labels.npz", "--self_critical_after", "2"], "--self_critical_after"),
])
def test_tools_refuse_incomplete_feature_arguments(tool, extra, message):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool)] + extra, capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "error:" in out.stderr and message in out.stderr, out.stderr[-1000:]
