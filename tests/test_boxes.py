"""Box features (the loader's ``use_box``, captioning/data/dataloader.py:477-487) off the GPU: the declarations of ``bofi_pack_regions_box``, its argument
checks, the loader side (``ImageIndex.sizes``, ``BoxRaggedBatch``), the CLI's argument errors -- and ``restated_image`` / ``restated_batch``, the numpy
restatement of the loader's lines that tests/test_gpu_boxes.py compares the kernel with bit for bit.  It is the loader's own expressions on float32 arrays
(numpy keeps float32 under a Python int divisor), pinned here against a case computed by hand."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def restated_image(att, box, w, h, norm_att=False, norm_box=False):
    """dataloader.py:475-487 for one image: ``att`` [r, F] and ``box`` [r, 4] float32, ``w`` / ``h`` Python ints -> float32 [r, F + 5], sorted by the last column,
    largest first.  The loader's order is Python's stable ``sorted(..., reverse=True)``; rows whose key is NaN (an order the loader leaves undefined) follow
    every number in source order: the project's rule."""
    att, box_feat, w, h = np.asarray(att, np.float32), np.asarray(box, np.float32), int(w), int(h)
    with np.errstate(invalid="ignore", divide="ignore"):
        if norm_att:
            att = att / np.linalg.norm(att, 2, 1, keepdims=True)
        x1, y1, x2, y2 = np.hsplit(box_feat, 4)
        box_feat = np.hstack((x1 / w, y1 / h, x2 / w, y2 / h, (x2 - x1) * (y2 - y1) / (w * h)))
        if norm_box:
            box_feat = box_feat / np.linalg.norm(box_feat, 2, 1, keepdims=True)
    assert box_feat.dtype == np.float32
    att_feat = np.hstack([att, box_feat])
    numbers = [x for x in att_feat if not np.isnan(x[-1])]
    return np.stack(sorted(numbers, key=lambda x: x[-1], reverse=True) + [x for x in att_feat if np.isnan(x[-1])])


def restated_batch(atts, boxes, sizes, out_R, F_out, norm_att=False, norm_box=False):
    """The images of a batch, zero-padded to float32 [B, out_R, F_out], and their region counts."""
    out = np.zeros((len(atts), out_R, F_out), np.float32)
    for b, (a, q, (w, h)) in enumerate(zip(atts, boxes, sizes)):
        r = restated_image(a, q, w, h, norm_att, norm_box)
        out[b, :r.shape[0], :r.shape[1]] = r
    return out, [a.shape[0] for a in atts]


def f32_bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def test_restatement_against_a_case_computed_by_hand():
    # a 4 x 2 image: boxes 0 and 2 have the same area (a tie: the earlier source row first), box 1 is the whole image, box 3 has no area
    att = np.arange(4, dtype=np.float32)[:, None] + np.zeros((4, 8), np.float32)
    box = np.array([[0, 0, 2, 1], [0, 0, 4, 2], [1, 0, 3, 1], [2, 1, 2, 2]], np.float32)
    got = restated_image(att, box, 4, 2)
    want_box = np.array([[0, 0, 1, 1, 1], [0, 0, .5, .5, .25], [.25, 0, .75, .5, .25], [.5, .5, .5, 1, 0]], np.float32)      # every value exact in float32
    assert got.dtype == np.float32 and got.shape == (4, 13)
    assert np.array_equal(got[:, 0], [1, 0, 2, 3]) and np.array_equal(f32_bits(got[:, 8:]), f32_bits(want_box))
    # norm_box: (0, 0, .5, .5, .25) has norm sqrt(.5625) = .75 exactly -> (0, 0, 2/3, 2/3, 1/3) as float32 quotients; the order follows the NORMALISED key
    normed = restated_image(att, box, 4, 2, norm_box=True)
    row0 = normed[normed[:, 0] == 0][0, 8:]
    third = np.float32(.25) / np.float32(.75)
    assert np.array_equal(f32_bits(row0), f32_bits(np.array([0, 0, np.float32(.5) / np.float32(.75), np.float32(.5) / np.float32(.75), third], np.float32)))
    key = {0: third, 1: np.float32(1) / np.sqrt(np.float32(3)), 2: np.float32(.25) / np.sqrt(np.float32(.9375)), 3: np.float32(0)}
    assert key[1] > third > key[2] > 0 and np.array_equal(normed[:, 0], [1, 0, 2, 3])
    assert np.array_equal(f32_bits(normed[:, -1]), f32_bits(np.array([key[1], key[0], key[2], key[3]], np.float32)))
    # a NaN key (an all-zero box under norm_box: 0 / 0) goes last, NaNs in source order
    box_nan = box.copy()
    box_nan[0] = 0
    box_nan[2] = 0
    last = restated_image(att, box_nan, 4, 2, norm_box=True)
    assert np.array_equal(last[:, 0], [1, 3, 0, 2]) and np.isnan(last[2:, -1]).all() and not np.isnan(last[:2]).any()
    # norm_att divides the attention columns alone
    both = restated_image(att + 1, box, 4, 2, norm_att=True)
    assert np.allclose(np.linalg.norm(both[:, :8].astype(np.float64), axis=1), 1.0, atol=1e-6) and np.array_equal(f32_bits(both[:, 8:]), f32_bits(got[:, 8:]))
    out, lens = restated_batch([att, att[:2]], [box, box[:2]], [(4, 2), (4, 2)], 6, 16)
    assert lens == [4, 2] and out.shape == (2, 6, 16) and not out[:, :, 13:].any() and not out[0, 4:].any() and not out[1, 2:].any()
    assert np.array_equal(out[1, :2, 0], [1, 0])


def _lib():
    from boficap_amd import hip
    assert os.path.exists(hip.LIB_PATH), "build the library first (python -m boficap_amd.build)"
    return hip, hip.lib()


def test_entry_point_is_declared_once_bound_and_built():
    from boficap_amd import build, hip
    assert "regions.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "regions.hip"))
    header = open(os.path.join(ROOT, "include", "boficap_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    found = re.findall(r"\bint\s+bofi_pack_regions_box\s*\(([^;]*)\)\s*;", code)
    assert len(found) == 1 and found[0].count(",") + 1 == len(hip.SIGNATURES["bofi_pack_regions_box"][1]) == 17
    assert len(re.findall(r"\bint\s+bofi_pack_regions\s*\(", code)) == 1 and len(hip.SIGNATURES["bofi_pack_regions"][1]) == 12      # the plain launch is untouched
    assert hip.ABI_VERSION == 5                                    # a symbol was added, nothing changed
    _, lib = _lib()
    assert hasattr(lib, "bofi_pack_regions_box") and callable(hip.pack_regions_box)


def test_bad_arguments_are_refused_without_a_device():
    """Every case is BOFI_ERR_ARG (1) from the argument check with a message: the device pointers are never read, nothing is launched."""
    hip, lib = _lib()
    p = C.c_void_p(0x1000)                                         # (any non-null 16-byte aligned value: validation comes first)
    off = np.array([0, 3, 9], np.int32)
    wh = np.array([[640, 480], [500, 375]], np.int32)
    hp = lambda a: a.ctypes.data_as(C.c_void_p)
    good = dict(rows=p, rows_dtype=hip.DT_F16, boxes=p, wh=p, wh_host=hp(wh), offsets=p, offsets_host=hp(off), B=2, F_att=2048, out=p, out_dtype=hip.DT_BF16, out_R=12,
                F_out=2112, norm_att=0, norm_box=1, att_len=None, stream=None)
    order = list(good)

    def refused(word, **kw):
        a = dict(good, **kw)
        rc = lib.bofi_pack_regions_box(*[a[k] for k in order])
        msg = lib.bofi_last_error().decode()
        assert rc == 1 and msg.startswith("bofi_pack_regions_box: ") and word in msg, (kw, rc, msg)

    for name in ("rows", "boxes", "wh", "offsets", "out"):
        refused("must be given", **{name: None})
    refused("B >= 1", B=0)
    refused("1 .. 1024", out_R=0)
    refused("1 .. 1024", out_R=1025)
    refused("multiple of 8", F_att=2053)
    refused("multiple of 8", F_att=0)
    refused("F_att + 5", F_out=2048)                               # no room for the box columns
    refused("F_att + 5", F_out=2052)
    refused("F_out = 2060", F_out=2060)                            # room, but no multiple of 8
    refused("rows_dtype", rows_dtype=3)
    refused("out_dtype", out_dtype=hip.DT_F16)
    refused("0 or 1", norm_box=2)
    refused("0 or 1", norm_att=-1)
    for name in ("rows", "boxes", "out"):
        refused("16-byte aligned", **{name: C.c_void_p(0x1008)})
    refused("expected 0", offsets_host=hp(np.array([1, 3, 9], np.int32)))
    refused("decrease", offsets_host=hp(np.array([0, 5, 3], np.int32)))
    refused("13 regions", offsets_host=hp(np.array([0, 3, 16], np.int32)))
    refused("640 x 0", wh_host=hp(np.array([[640, 0], [500, 375]], np.int32)))
    refused("image 1 is -5 x 375", wh_host=hp(np.array([[640, 480], [-5, 375]], np.int32)))
    refused("too large", B=2 ** 24, out_R=1024, offsets_host=None, wh_host=None)


def test_image_index_sizes(tmp_path):
    from boficap_amd.features import ImageIndex
    images = [{"id": 7, "width": 640, "height": 480}, {"id": 9, "width": 500, "height": 375, "split": "val"}, {"id": 11, "width": 333}]
    path = tmp_path / "talk.json"
    path.write_text(json.dumps({"images": images}))
    index = ImageIndex(str(path))
    got = index.sizes([1, 0])
    assert got.dtype == np.int32 and got.tolist() == [[500, 375], [640, 480]]
    with pytest.raises(KeyError, match=r"11.*height"):
        index.sizes([0, 2])


def test_box_batches_are_staged_beside_the_rows(tmp_path):
    from boficap_amd.features import BoxRaggedBatch, RaggedBatch, RegionFeeder, RegionSource, RegionStore
    rng = np.random.default_rng(0)
    lens, ids = [3, 1, 5], [40, 41, 42]
    (tmp_path / "att").mkdir()
    (tmp_path / "box").mkdir()
    atts = [rng.random((l, 64)).astype(np.float16) for l in lens]
    boxes = [rng.random((l, 4)) * 100 for l in lens]               # float64 files: cast to float32
    for i, a, q in zip(ids, atts, boxes):
        np.savez(tmp_path / "att" / f"{i}.npz", feat=a)
        np.save(tmp_path / "box" / f"{i}.npy", q)
    sizes = np.array([[640, 480], [500, 375], [320, 240]], np.int32)
    store, box_store = RegionStore(str(tmp_path / "att")), RegionStore(str(tmp_path / "box"), ".npy")
    src = RegionSource(store, ids, True, box_store=box_store, sizes=sizes, norm_box_feat=True)
    rb = src.ragged(1, 3)
    assert isinstance(rb, BoxRaggedBatch) and isinstance(rb, RaggedBatch) and rb.norm and rb.norm_box and (rb.B, rb.F, rb.F_out, rb.out_F) == (2, 64, 128, 128)
    assert rb.boxes.dtype == torch.float32 and np.array_equal(rb.boxes.numpy(), np.concatenate(boxes[1:]).astype(np.float32))
    assert rb.wh.dtype == torch.int32 and rb.wh.tolist() == sizes[1:].tolist() and rb.offsets.tolist() == [0, 1, 6]
    assert torch.equal(rb.rows, RaggedBatch.from_arrays(atts[1:]).rows)
    assert BoxRaggedBatch.from_arrays([a.astype(np.float32) for a in atts], [q.astype(np.float32) for q in boxes], sizes).F_out == 128
    assert BoxRaggedBatch.from_arrays([rng.random((2, 2048)).astype(np.float16)], [np.ones((2, 4), np.float32)], [[4, 4]]).F_out == 2112
    fed = list(RegionFeeder(store, [["41", "42"], ["40"]], workers=2, box_store=box_store, sizes={str(i): wh for i, wh in zip(ids, sizes)}, norm_box_feat=True))
    assert [type(f) for f in fed] == [BoxRaggedBatch] * 2 and torch.equal(fed[0].boxes, rb.boxes) and torch.equal(fed[0].wh, rb.wh) and fed[1].wh.tolist() == [[640, 480]]
    assert fed[0].norm_box and not fed[0].norm
    assert type(RegionSource(store, ids).ragged(0, 2)) is RaggedBatch                      # without a box store nothing changes
    with pytest.raises(ValueError, match="one .x1, y1, x2, y2. per region row"):
        BoxRaggedBatch.from_arrays(atts, [boxes[0], boxes[1], boxes[2][:4]], sizes)
    with pytest.raises(ValueError, match=">= 1"):
        BoxRaggedBatch.from_arrays(atts, boxes, [[640, 480], [0, 375], [320, 240]])
    with pytest.raises(ValueError, match="sizes"):
        RegionSource(store, ids, box_store=box_store)
    with pytest.raises(ValueError, match="F = 69"):                 # the plain batch still refuses an unaligned width
        RaggedBatch.from_arrays([np.ones((2, 69), np.float32)])


def test_config_pads_an_unaligned_feature_width():
    import dataclasses
    from boficap_amd.config import FULL, TINY
    assert FULL.att_feat_padded == FULL.att_feat_size == 2048 and TINY.att_feat_padded == 64
    assert dataclasses.replace(FULL, att_feat_size=2053).att_feat_padded == 2112 and dataclasses.replace(TINY, att_feat_size=69).att_feat_padded == 128


def run_eval(extra):
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval.py")] + extra, capture_output=True, text=True, timeout=120)


def test_eval_cli_argument_errors(tmp_path):
    out = run_eval(["--input_att_dir", "feats", "--input_json", "talk.json", "--use_box", "1"])
    assert out.returncode == 2 and "error:" in out.stderr and "F = 2053" in out.stderr and "--input_box_dir" in out.stderr, out.stderr[-1000:]
    out = run_eval(["--input_att_dir", "feats", "--input_json", "talk.json", "--input_box_dir", "boxes"])
    assert out.returncode == 2 and "--use_box 1" in out.stderr, out.stderr[-1000:]
    # a model of another width than the files make: both numbers are named, before anything touches a device (the default model is the 2048-wide one)
    (tmp_path / "att").mkdir()
    (tmp_path / "box").mkdir()
    np.savez(tmp_path / "att" / "5.npz", feat=np.ones((3, 2048), np.float16))
    np.save(tmp_path / "box" / "5.npy", np.ones((3, 4), np.float32))
    talk = tmp_path / "talk.json"
    talk.write_text(json.dumps({"images": [{"id": 5, "split": "val", "width": 640, "height": 480}]}))
    out = run_eval(["--input_att_dir", str(tmp_path / "att"), "--input_json", str(talk), "--use_box", "1", "--input_box_dir", str(tmp_path / "box")])
    assert out.returncode == 2 and "att_feat_size is 2048" in out.stderr and "2053" in out.stderr, out.stderr[-1000:]
    talk.write_text(json.dumps({"images": [{"id": 5, "split": "val", "width": 640}]}))
    out = run_eval(["--input_att_dir", str(tmp_path / "att"), "--input_json", str(talk), "--use_box", "1", "--input_box_dir", str(tmp_path / "box")])
    assert out.returncode != 0 and "height" in out.stderr, out.stderr[-1000:]
