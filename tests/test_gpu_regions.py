"""``bofi_pack_regions`` (boficap_amd/csrc/regions.hip) on the MI355X against a float64 restatement written here, and the paths that consume it:
``RaggedBatch.to_device``, ``decode_many`` over ragged items, ``eval_split`` on a region source, and the two CLIs on per-image feature files.

Tolerances.  norm = 0 is a copy or a conversion: bit-equal.  norm = 1, float32 output: relative error <= 2e-6 on every non-zero element -- derived, not
measured: the sum of F non-negative squares in float32 along a chain of at most F / 64 + 6 = 38 additions carries at most 38 * 2^-24 = 2.3e-6, the
square root halves that, and the square, the root and the division add about three more roundings.  bfloat16 output: round-to-nearest-even of the kernel's
own float32 output, bit for bit, hence within (2^-8 + 2e-6) |ref| of the restatement (half a bfloat16 ulp + the float32 bar)."""
import json
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import record_parity

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORM_BAR = 2e-6
LENS5 = [1, 7, 0, 36, 2]
# (F, lens, out_R): F = 64 leaves most lanes idle, 72 is a multiple of 8 but not of 64, 2048 is the model's; out_R = 48 is a bucket wider than the longest
# image; B = 1; 15 and 5 output rows are no multiple of the 4 rows of a workgroup, 180 and 240 are many workgroups
SHAPES = [(64, LENS5, 36), (72, LENS5, 48), (2048, LENS5, 48), (64, [5], 5), (72, [3, 5, 1], 5), (2048, [36, 36], 36)]
IN_DTYPES = [torch.float32, torch.float16, torch.bfloat16]
OUT_DTYPES = [torch.float32, torch.bfloat16]


def rows_of(F, lens, dtype, seed=0):
    """Sparse non-negative rows (as the detector's ReLU outputs are) at three scales, no row all zero, in ``dtype`` on the host."""
    rng = np.random.default_rng(1000 * F + 10 * sum(lens) + seed)
    n = sum(lens)
    x = np.maximum(rng.standard_normal((n, F)), 0.0) * np.where(rng.random((n, F)) < 0.5, 1.0, 0.0)
    x *= np.array([0.03, 1.0, 40.0])[rng.integers(0, 3, n)][:, None]
    x[:, 0] += 0.01
    return torch.from_numpy(x.astype(np.float32)).to(dtype)


def restated(rows, lens, out_R, norm):
    """float64: zero-padded [B, out_R, F] of the rows, every real row divided by its L2 norm when ``norm``."""
    x = rows.to(torch.float64).numpy()
    out, o = np.zeros((len(lens), out_R, x.shape[1])), 0
    for b, l in enumerate(lens):
        r = x[o:o + l]
        if norm:
            with np.errstate(invalid="ignore"):
                r = r / np.sqrt((r * r).sum(1, keepdims=True))
        out[b, :l] = r
        o += l
    return out


def offsets_of(lens):
    return torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32)


def pack(rows, lens, out_R, out_dtype, norm, out=None):
    """One launch: (out [B, out_R, F], att_len) on the device."""
    from boficap_amd import hip
    off = offsets_of(lens)
    if out is None:
        out = torch.full((len(lens), out_R, rows.size(1)), 777.0, dtype=out_dtype, device="cuda")
    att_len = torch.full((len(lens),), -5, dtype=torch.int32, device="cuda")
    hip.pack_regions(rows.cuda(), off.cuda(), off, out, norm=norm, att_len=att_len)
    return out, att_len


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def padding_mask(lens, out_R):
    return torch.arange(out_R)[None, :] >= torch.tensor(lens)[:, None]


@pytest.mark.parametrize("F, lens, out_R", SHAPES)
def test_copy_and_conversion_are_bit_exact(F, lens, out_R):
    from boficap_amd.data import collate_regions
    pad = padding_mask(lens, out_R)
    for din in IN_DTYPES:
        rows = rows_of(F, lens, din)
        as_f32 = torch.from_numpy(restated(rows, lens, out_R, False)).to(torch.float32)          # (float16 / bfloat16 -> float32 is exact)
        for dout in OUT_DTYPES:
            out, att_len = pack(rows, lens, out_R, dout, False)
            out = out.cpu()
            assert att_len.cpu().tolist() == lens
            want = as_f32 if dout == torch.float32 else as_f32.to(torch.bfloat16)              # torch's cast: round to nearest even
            assert torch.equal(bits(out), bits(want)), (din, dout)
            assert not bits(out)[pad].any()                       # the padding is +0.0, bit for bit
    # the tie to the reference's collate (tests/golden/tiny_collate.npz pins collate_regions to it): features and mask, on float32
    rows = rows_of(F, lens, torch.float32)
    out, att_len = pack(rows, lens, out_R, torch.float32, False)
    per_image = list(torch.split(rows, lens))
    feats, masks = collate_regions([a.numpy() for a in per_image])
    longest = max(lens)
    assert np.array_equal(out.cpu().numpy()[:, :longest].view(np.int32), feats.view(np.int32)) and not out.cpu().numpy()[:, longest:].any()
    mine = (torch.arange(longest)[None, :] < att_len.cpu()[:, None]).float().numpy()
    assert np.array_equal(mine, masks if masks is not None else np.ones_like(mine))
    assert (masks is None) == (min(lens) == longest)


@pytest.mark.parametrize("F, lens, out_R", SHAPES)
def test_norm_is_within_the_derived_bar(F, lens, out_R):
    pad, worst, worst16 = padding_mask(lens, out_R), 0.0, 0.0
    for din in IN_DTYPES:
        rows = rows_of(F, lens, din)
        ref = restated(rows, lens, out_R, True)
        out32, att_len = pack(rows, lens, out_R, torch.float32, True)
        out16, _ = pack(rows, lens, out_R, torch.bfloat16, True)
        again, _ = pack(rows, lens, out_R, torch.float32, True)
        out32, out16 = out32.cpu(), out16.cpu()
        assert att_len.cpu().tolist() == lens
        assert torch.equal(bits(out32), bits(again.cpu()))        # deterministic: two calls, equal bytes
        assert not bits(out32)[pad].any() and not bits(out16)[pad].any()
        got, nz = out32.to(torch.float64).numpy(), ref != 0
        assert np.array_equal(got == 0, ref == 0)
        err = float((np.abs(got - ref)[nz] / np.abs(ref)[nz]).max())
        worst = max(worst, err)
        assert err <= NORM_BAR, (din, err)
        assert torch.equal(bits(out16), bits(out32.to(torch.bfloat16))), din       # round-to-nearest-even of the kernel's own float32 output
        err16 = float((np.abs(out16.to(torch.float64).numpy() - ref)[nz] / np.abs(ref)[nz]).max())
        worst16 = max(worst16, err16)
        assert err16 <= 2.0 ** -8 + NORM_BAR, (din, err16)
    print(f"pack_regions norm F={F} B={len(lens)} out_R={out_R}: max rel err f32 {worst:.3e} (bar {NORM_BAR:.1e}), bf16 {worst16:.3e} (bar {2.0 ** -8 + NORM_BAR:.4e})")
    record_parity(f"pack_regions_norm_f32_F{F}_B{len(lens)}_R{out_R}", worst, NORM_BAR, "relative, non-zero elements, vs the float64 restatement; bar derived from the summation chain")
    record_parity(f"pack_regions_norm_bf16_F{F}_B{len(lens)}_R{out_R}", worst16, 2.0 ** -8 + NORM_BAR, "relative; half a bf16 ulp + the float32 bar")


def test_a_zero_row_normalises_to_nan_and_leaves_its_neighbours_alone():
    lens, F = [3, 4], 72
    rows = rows_of(F, lens, torch.float32)
    base, _ = pack(rows, lens, 4, torch.float32, True)
    rows0 = rows.clone()
    rows0[4] = 0.0                                                 # image 1, row 1
    for dout in OUT_DTYPES:
        out, _ = pack(rows0, lens, 4, dout, True)
        out = out.cpu()
        assert torch.isnan(out[1, 1]).all()                        # 0 / 0, as numpy gives it
        keep = torch.ones(2, 4, dtype=torch.bool)
        keep[1, 1] = False
        want = base.cpu() if dout == torch.float32 else base.cpu().to(torch.bfloat16)
        assert torch.equal(bits(out)[keep], bits(want)[keep])


@pytest.mark.parametrize("dout", OUT_DTYPES)
@pytest.mark.parametrize("norm", [False, True])
def test_writes_stay_inside_out_and_cover_all_of_it(dout, norm):
    F, lens, out_R = 72, LENS5, 48                                 # the image without rows and the bucket wider than the longest image
    n, pre, post = len(lens) * out_R * F, 64, 200
    big = torch.full((pre + n + post,), 12288.0, dtype=dout, device="cuda")            # (12288 is a bfloat16 value)
    view = big[pre:pre + n].view(len(lens), out_R, F)
    out, _ = pack(rows_of(F, lens, torch.float16), lens, out_R, dout, norm, out=view)
    assert out.data_ptr() == view.data_ptr()
    host = big.cpu()
    assert (host[:pre] == 12288.0).all() and (host[pre + n:] == 12288.0).all()
    assert not (host[pre:pre + n] == 12288.0).any()                # every element of the view was written
    want = restated(rows_of(F, lens, torch.float16), lens, out_R, norm)
    assert np.allclose(host[pre:pre + n].to(torch.float64).numpy().reshape(want.shape), want, rtol=2.0 ** -8 + NORM_BAR, atol=0)


def test_misuse_is_refused_before_any_launch():
    from boficap_amd import hip
    lib, p = hip.lib(), hip.ptr

    def call(rows, off_host, B, F, out, out_R, off_dev=None):
        off_dev = off_host.cuda() if off_dev is None else off_dev
        rc = lib.bofi_pack_regions(p(rows), hip.DT_F32, p(off_dev), p(off_host), B, F, p(out), hip.DT_F32, out_R, 0, None, hip.stream_ptr())
        msg = lib.bofi_last_error().decode()
        torch.cuda.synchronize()
        return rc, msg

    rows = torch.ones(64, 16, device="cuda")
    out = torch.full((2, 8, 16), 777.0, device="cuda")
    good = torch.tensor([0, 3, 9], dtype=torch.int32)
    cases = [(torch.tensor([0, 5, 3], dtype=torch.int32), 2, 16, 8, "decrease"),            # decreasing offsets
             (torch.tensor([0, 3, 12], dtype=torch.int32), 2, 16, 8, "9 regions"),          # len_b > out_R
             (good, 2, 12, 8, "multiple of 8"),                                             # F = 12
             (good, 0, 16, 8, "B >= 1")]                                                    # B = 0
    for off, B, F, out_R, word in cases:
        rc, msg = call(rows, off, B, F, out, out_R)
        assert rc == 1 and word in msg, (rc, msg)                  # BOFI_ERR_ARG, with a message
        assert (out == 777.0).all()                                # nothing was launched
    with pytest.raises(hip.BofiHipError, match="decrease"):
        hip.pack_regions(rows, cases[0][0].cuda(), cases[0][0], out)
    # a bad DEVICE array behind a good host copy: the kernel clamps len_b to out_R, so the writes stay inside out all the same
    big = torch.full((64 + 2 * 8 * 16 + 64,), 777.0, device="cuda")
    view = big[64:64 + 256].view(2, 8, 16)
    rc, _ = call(rows, good, 2, 16, view, 8, off_dev=torch.tensor([0, 20, 9], dtype=torch.int32).cuda())       # lengths 20 and -11 on the device
    assert rc == 0
    host = big.cpu()
    assert (host[:64] == 777.0).all() and (host[-64:] == 777.0).all() and (host[64:320].view(2, 8, 16)[0] == 1.0).all() and (host[64:320].view(2, 8, 16)[1] == 0.0).all()


# ------------------------------------------------------------------------------------------------------------------ end to end, tiny configuration

def same(a, b):
    """Equality of nested results in which a NaN (an image whose fill mask is empty under quirk Q1 has NaN entropy) equals a NaN: floats by their bits."""
    if torch.is_tensor(a):
        return a.dtype == b.dtype and a.shape == b.shape and (torch.equal(bits(a), bits(b)) if a.is_floating_point() else torch.equal(a, b))
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and isinstance(b, float):
        return np.float64(a).tobytes() == np.float64(b).tobytes()
    return a == b


def tiny_images(lens, seed, dtype=np.float32, F=64):
    rng = np.random.default_rng(seed)
    return [np.abs(rng.standard_normal((l, F))).astype(dtype) for l in lens]


def padded(images):
    """What the loader's collate hands over: float32 [b, longest, F] and the float32 mask."""
    from boficap_amd.data import collate_regions
    feats, masks = collate_regions([a.astype(np.float32) for a in images])
    return feats, (masks if masks is not None else np.ones(feats.shape[:2], np.float32))


def test_to_device_equals_the_host_collate_and_cast():
    from boficap_amd.data import collate_regions
    from boficap_amd.features import RaggedBatch, att_masks_of
    images = tiny_images([3, 9, 1, 6], 0, np.float16)
    feats, masks = collate_regions([a.astype(np.float32) for a in images])
    rb = RaggedBatch.from_arrays(images)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                        # two copies and one launch: no synchronisation
    try:
        got, att_len = rb.to_device(out_dtype=torch.bfloat16)
        wide, wide_len = rb.to_device(out_dtype=torch.float32, out_R=12)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.equal(bits(got.cpu()), bits(torch.from_numpy(feats).to(torch.bfloat16)))
    assert np.array_equal(att_masks_of(att_len, 9).cpu().numpy(), masks)
    assert np.array_equal(wide.cpu().numpy()[:, :9], feats) and not wide.cpu().numpy()[:, 9:].any() and wide_len.cpu().tolist() == [3, 9, 1, 6]
    same = RaggedBatch.from_arrays(tiny_images([5, 5, 5], 1))
    feats5, masks5 = collate_regions(tiny_images([5, 5, 5], 1))
    got, att_len = same.to_device(out_dtype=torch.float32)
    assert masks5 is None and att_len is None and np.array_equal(got.cpu().numpy(), feats5)      # equal counts: no mask, as the loader returns it
    got, att_len = same.to_device(out_dtype=torch.float32, out_R=8)
    assert att_len is not None and att_len.cpu().tolist() == [5, 5, 5]                         # ... but not in a wider bucket
    normed, _ = RaggedBatch.from_arrays(tiny_images([5, 5, 5], 1), norm=True).to_device(out_dtype=torch.float32)
    feats64 = feats5.astype(np.float64)
    assert np.allclose(normed.cpu().numpy(), feats64 / np.linalg.norm(feats64, 2, 2, keepdims=True), rtol=NORM_BAR, atol=0)


def test_decode_many_over_ragged_items_equals_padded_items():
    from boficap_amd.features import RaggedBatch
    from test_gpu_lang_eval import tiny_model
    model = tiny_model().eval()
    groups = [tiny_images([40, 3, 17, 36], 2), tiny_images([5, 44, 1, 20], 3)]                 # longest 40 and 44: both in the 48-region bucket
    keys = ("seq", "phrase_num", "phrase_length", "phrase_syn", "entropy", "perplexity")
    with torch.no_grad():
        want = [{k: r[k].clone() for k in keys} for r in model.decode_many([padded(g) for g in groups])]
        got = [{k: r[k].clone() for k in keys} for r in model.decode_many([RaggedBatch.from_arrays(g) for g in groups])]
        half = [{k: r[k].clone() for k in keys} for r in model.decode_many([RaggedBatch.from_arrays([a.astype(np.float16) for a in g]) for g in groups])]
        want_half = [{k: r[k].clone() for k in keys} for r in model.decode_many([padded([a.astype(np.float16) for a in g]) for g in groups])]
    assert len(got) == len(want) == 2
    for a, b in list(zip(got, want)) + list(zip(half, want_half)):
        for k in keys:
            assert same(a[k], b[k]), k


def region_dir(tmp_path, name, images, ids):
    d = tmp_path / name
    d.mkdir()
    for i, a in zip(ids, images):
        np.savez(d / f"{i}.npz", feat=a)
    return str(d)


def test_eval_split_on_a_region_source_equals_the_dense_array(tmp_path):
    from boficap_amd import eval_utils
    from boficap_amd.config import TINY
    from boficap_amd.features import RegionSource, RegionStore
    from test_gpu_lang_eval import tiny_model
    labels = eval_utils.SyntheticLabels(TINY, 8, 5, seed=3)         # 8 images of 36 regions: the dense array IS the loader's batch (equal counts, no mask)
    ids = [500 + 3 * i for i in range(8)]
    source = RegionSource(RegionStore(region_dir(tmp_path, "att", list(labels.feats), ids)), ids)
    model = tiny_model()
    for mode in ("NAIC", "SAIC"):
        kw = {"batch_size": 4, "language_eval": 1, "inference_mode": mode}
        loss_d, pred_d, stats_d = eval_utils.eval_split(model, labels.feats, labels, dict(kw))
        loss_s, pred_s, stats_s = eval_utils.eval_split(model, source, labels, dict(kw))
        assert same(loss_s, loss_d) and same(pred_s, pred_d) and same(stats_s, stats_d), mode
        assert np.isfinite(loss_s) and len(pred_s) == 8
    # images of different counts: every batch padded to its longest image on the device, masked by the counts -- the NAIC captions are those of the
    # padded (features, mask) batches through the same pipeline, the SAIC captions those of mode='sample' on the loader's batch
    lens = [12, 3, 36, 7, 20, 20, 1, 9]
    images = tiny_images(lens, 5)
    ragged = RegionSource(RegionStore(region_dir(tmp_path, "ragged", images, ids)), ids)
    kw = {"batch_size": 4, "language_eval": 1, "inference_mode": "NAIC"}
    loss_r, pred_r, stats_r = eval_utils.eval_split(model, ragged, labels, dict(kw))
    with torch.no_grad():
        want = torch.cat([r["seq"] for r in model.eval().decode_many([padded(images[:4]), padded(images[4:])])])
    assert [p["seq"] for p in pred_r] == [[int(v) for v in row.tolist() if v > 0] for row in want]
    assert np.isfinite(loss_r) and loss_r != loss_d and set(stats_r) == set(stats_d)
    _, pred_sa, _ = eval_utils.eval_split(model, ragged, labels, dict(kw, inference_mode="SAIC", verbose_loss=0))
    with torch.no_grad():
        f, m = padded(images[:4])
        seq = model.eval()(torch.zeros(4, 0, device="cuda"), torch.from_numpy(f).cuda(), torch.from_numpy(m).cuda(),
                           opt={"train_mode": "SAIC", "sample_method": "greedy", "sample_n": 1}, mode="sample")[0]
    assert [p["seq"] for p in pred_sa[:4]] == [[int(v) for v in row.tolist() if v > 0] for row in seq.cpu()]


def label_arrays(n_img, per, seed=21):
    from boficap_amd.collate import synthetic_captions
    from boficap_amd.config import TINY
    Sq = TINY.seq_length
    labels, plen, psyn = synthetic_captions(TINY, n_img * per, seed=seed)
    return {"labels": labels[:, 1:Sq + 1].astype(np.uint32), "label_start_ix": (np.arange(n_img) * per + 1).astype(np.uint32),
            "label_end_ix": ((np.arange(n_img) + 1) * per).astype(np.uint32), "label_length": (labels[:, 1:Sq + 1] > 0).sum(1).astype(np.uint32),
            "phrase_num": (plen > 0).sum(1).astype(np.uint32), "phrase_length": plen.astype(np.uint32), "phrase_label": psyn.astype(np.uint32)}


SPLITS = ["train", "val", "train", "restval", "val", "test", "train", "val", "train", "train"]
IDS = [9000 + 7 * i for i in range(len(SPLITS))]
REGIONS = [12, 36, 5, 20, 36, 9, 1, 17, 30, 8]


def dataset(tmp_path, seed=7):
    """Ten images: a json with ids and splits, the label arrays as .npz, a directory of <id>.npz (float16 and float32 files)."""
    images = [a.astype(np.float16 if i % 2 else np.float32) for i, a in enumerate(tiny_images(REGIONS, seed))]
    att = region_dir(tmp_path, f"att{seed}", images, IDS)
    talk, npz = str(tmp_path / "talk.json"), str(tmp_path / "labels.npz")
    with open(talk, "w") as f:
        json.dump({"images": [{"id": i, "split": s} for i, s in zip(IDS, SPLITS)]}, f)
    np.savez(npz, **label_arrays(len(SPLITS), 5))
    return att, talk, npz


def test_tools_eval_reads_a_feature_directory(tmp_path):
    """tools/eval.py --input_att_dir --input_json --split val in a fresh process: the json's ids in the split's order, the scores of eval_split."""
    from boficap_amd import eval_utils, weights as W
    from boficap_amd.config import TINY
    from boficap_amd.data import LabelStore
    from boficap_amd.features import ImageIndex, RegionSource, RegionStore
    from test_gpu_lang_eval import tiny_model
    att, talk, npz = dataset(tmp_path)
    pth, pkl, dump = (str(tmp_path / f) for f in ("model.pth", "infos.pkl", "out.json"))
    torch.save({k: torch.from_numpy(v) for k, v in W.make_state_dict(TINY, seed=0, gen_scale=6.0).items()}, pth)
    opt = TINY.to_opt()
    with open(pkl, "wb") as f:
        pickle.dump({"opt": opt, "vocab": opt.vocab}, f, protocol=2)
    cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tools", "eval.py"), "--model", pth, "--infos_path", pkl, "--batch_size", "2", "--dtype", "f32",
           "--input_att_dir", att, "--input_json", talk, "--split", "val", "--input_label_npz", npz, "--language_eval", "1", "--dump_json", dump, "--feeder_workers", "2"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    with open(dump) as f:
        dumped = json.load(f)
    index = ImageIndex(talk)
    val_ix = index.split_ix["val"]
    assert val_ix == [1, 4, 7] and [p["image_id"] for p in dumped["predictions"]] == [IDS[i] for i in val_ix]
    c = TINY
    store = LabelStore(dict(np.load(npz)), pad_idx=c.pad_idx, bos_idx=c.bos_idx, eos_idx=c.eos_idx, len_idx=c.len_idx)
    source = RegionSource(RegionStore(att), [IDS[i] for i in val_ix])
    loss, pred, stats = eval_utils.eval_split(tiny_model(), source, store, {"batch_size": 2, "language_eval": 1, "image_ixs": val_ix, "vocab": opt.vocab})
    assert [p["seq"] for p in dumped["predictions"]] == [p["seq"] for p in pred]
    assert same(dumped["lang_stats"], stats)
    printed = dict(re.findall(r"(\w+) (-?[0-9.]+|nan)", out.stdout.split("language scores ")[1].splitlines()[0]))
    assert printed == {k: f"{v:.6f}" for k, v in stats.items()}
    assert f"validation loss {loss:.4f} over 2 batches" in out.stdout


def train_lines(cmd):
    out = subprocess.run(["timeout", "-k", "10", "240"] + cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [re.sub(r" [0-9.]+ s/it", "", ln) for ln in out.stdout.splitlines() if ln.startswith("iter ")]
    assert lines and "nan" not in " ".join(lines).lower() and "inf" not in " ".join(lines).lower(), out.stdout[-2000:]
    return lines


def test_tools_train_reads_a_feature_directory(tmp_path):
    """tools/train.py on per-image feature files in fresh processes: finite losses that depend on the features, the same with 1 and 4 feeder threads."""
    att, talk, npz = dataset(tmp_path)
    other, _, _ = dataset(tmp_path, seed=8)
    base = [sys.executable, os.path.join(ROOT, "tools", "train.py"), "--tiny", "--input_json", talk, "--input_label_h5", npz, "--max_iters", "4", "--val_images_use", "2",
            "--save_checkpoint_every", "4", "--losses_log_every", "1", "--batch_size", "3", "--dtype", "f32"]
    one = train_lines(base + ["--input_att_dir", att, "--feeder_workers", "1"])
    four = train_lines(base + ["--input_att_dir", att, "--feeder_workers", "4"])
    moved = train_lines(base + ["--input_att_dir", other, "--feeder_workers", "4"])
    assert [ln.split()[1] for ln in one] == ["1", "2", "3", "4", "4"]            # four XE steps, the validation pass
    assert all("train_loss" in ln for ln in one[:4]) and "validation loss" in one[4]
    assert one == four                                                           # the feeder does not reorder
    assert all(a != b for a, b in zip(one[:4], moved[:4])) and one[4] != moved[4]      # the features are really read


def test_tools_train_without_the_new_options_prints_what_it_printed(tmp_path):
    """The synthetic stream of tools/train.py, untouched by the feature options: the child's losses against the loop the tool ran before them, restated here
    (synthetic captions and |N(0,1)| features of 36 regions from the per-step seed)."""
    import captioning.models as models
    from boficap_amd import weights as W
    from boficap_amd.collate import synthetic_training_batch
    from boficap_amd.config import TINY
    from boficap_amd.trainer import XETrainer
    lines = train_lines([sys.executable, os.path.join(ROOT, "tools", "train.py"), "--tiny", "--max_iters", "3", "--losses_log_every", "1", "--batch_size", "3", "--dtype", "f32"])
    opt = TINY.to_opt()
    opt.batch_size, opt.seq_per_img, opt.seed, opt.id, opt.checkpoint_path, opt.bofi_train_dtype = 3, getattr(opt, "seq_per_img", 5), 42, "bofi", "", torch.float32
    torch.manual_seed(42)
    model = models.setup(opt)
    model.cuda().train()
    trainer = XETrainer(model, opt, graph=True)
    for it in range(3):
        seed = it * 7919 + 42
        host = synthetic_training_batch(model.cfg, 3, opt.seq_per_img, seed=seed)
        batch = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
        batch["max_phrase_num"] = int(host["phrase_num"].max())
        batch["max_tokens"] = int((host["phrase_length"].sum(-1) - 1).max())
        batch["att_feats"] = torch.from_numpy(W.synthetic_att_feats(3, 36, model.cfg.att_feat_size, seed=seed)).cuda()
        batch = trainer.add_token_rows(batch, host)
        loss, parts = trainer.step(batch, -1.0, False)
        names = ("sa_len", "sa_tok", "sa_syn", "na_len", "na_tok", "na_syn")
        detail = " ".join(f"{n}={float(p):.3f}" for n, p in zip(names, parts))
        assert lines[it] == f"iter {it + 1} lr {trainer.rate():.3e} train_loss {float(loss):.4f} ({detail})", (lines[it], float(loss))
