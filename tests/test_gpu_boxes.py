"""``bofi_pack_regions_box`` (boficap_amd/csrc/regions.hip) on the MI355X against the numpy restatement of the loader's use_box lines (tests/test_boxes.py),
and the layers above it: an engine whose ``att_feat_size`` is no multiple of 64, ``decode_many`` over box batches, ``tools/eval.py --use_box 1``.

Tolerances.  The box columns are single correctly rounded float32 operations in numpy's order and the order is a comparison of those values: bit-equal, as
is everything under ``norm_att = 0`` (a copy or a conversion).  ``norm_att = 1`` runs the plain launch's code on the attention columns: its bar, NORM_BAR of
tests/test_gpu_regions.py, derived there from the summation chain.  A bfloat16 output is the round-to-nearest-even of the kernel's own float32 output.  The
engine's log-probs against the float32 oracle: 1e-3, the bar of the float32 tiny cases of tests/test_gpu_naic.py."""
import dataclasses
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import boficap_oracle as O
from conftest import record_parity
from test_boxes import restated_batch
from test_gpu_regions import NORM_BAR, bits, offsets_of, rows_of, same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 12288.0                                                 # (a bfloat16 value)
OUT_DTYPES = [torch.float32, torch.bfloat16]


def boxes_of(lens, seed):
    """Per image: float32 boxes [len, 4] with fractional pixel coordinates inside a (width, height) of its own.  The first image of 7 regions or more holds
    two identical boxes (rows 2 and 5: a tie), the first OTHER image of 3 or more a box without area (row 1)."""
    rng = np.random.default_rng(seed)
    sizes = [(int(rng.integers(200, 641)), int(rng.integers(150, 481))) for _ in lens]
    boxes = []
    for l, (w, h) in zip(lens, sizes):
        x1, y1 = rng.uniform(0, w - 2, l), rng.uniform(0, h - 2, l)
        boxes.append(np.stack([x1, y1, x1 + rng.uniform(1, w - x1), y1 + rng.uniform(1, h - y1)], 1).astype(np.float32))
    tie = next(b for b, l in enumerate(lens) if l >= 7)
    boxes[tie][5] = boxes[tie][2]
    flat = next(b for b, l in enumerate(lens) if l >= 3 and b != tie)
    boxes[flat][1, 2] = boxes[flat][1, 0]
    return boxes, sizes


def pack_box(rows, boxes, sizes, lens, out_R, F_out, out_dtype, norm_att, norm_box, out=None):
    """One launch: (out [B, out_R, F_out], att_len) on the device; a fresh ``out`` is filled with the sentinel first."""
    from boficap_amd import hip
    off, wh = offsets_of(lens), torch.tensor(sizes, dtype=torch.int32)
    if out is None:
        out = torch.full((len(lens), out_R, F_out), SENTINEL, dtype=out_dtype, device="cuda")
    att_len = torch.full((len(lens),), -5, dtype=torch.int32, device="cuda")
    hip.pack_regions_box(rows.cuda(), torch.from_numpy(np.concatenate(boxes)).cuda(), wh.cuda(), wh, off.cuda(), off, out, norm_att=norm_att, norm_box=norm_box, att_len=att_len)
    return out, att_len


# (F_att, F_out, lens, out_R): 64 -> 128 leaves most lanes idle and has one chunk of box columns + 7 of zeros, 2048 -> 2112 is the model's; 100 regions are 25
# workgroups per image and more than one pass of the 64 lanes over the keys, 64 / 65 sit on that boundary, 1 is an image of one row, out_R = 12 with 3 and 9
# rows leaves padding rows in a workgroup that also moves real ones
SHAPES = [(64, 128, [1, 7, 100, 64, 65, 36, 3], 100), (64, 128, [3, 9], 12), (2048, 2112, [100, 7], 100), (2048, 2112, [3, 9], 12)]


@pytest.mark.parametrize("F_att, F_out, lens, out_R", SHAPES)
def test_kernel_against_the_restatement(F_att, F_out, lens, out_R):
    boxes, sizes = boxes_of(lens, 7 * F_att + out_R)
    worst = 0.0
    for din in (torch.float32, torch.float16):
        rows = rows_of(F_att, lens, din)
        atts = [a.numpy() for a in torch.split(rows.float(), lens)]
        for norm_box in (False, True):
            want, want_len = restated_batch(atts, boxes, sizes, out_R, F_out, False, norm_box)
            ties = sum(int((np.diff(want[b, :l, F_att + 4]) == 0).sum()) for b, l in enumerate(lens))
            flat = sum(int((want[b, :l, F_att + 4] == 0).sum()) for b, l in enumerate(lens))
            assert ties >= 1 and flat >= 1                         # the tie and the box without area are really there
            out32, att_len = pack_box(rows, boxes, sizes, lens, out_R, F_out, torch.float32, False, norm_box)
            assert att_len.cpu().tolist() == want_len
            assert np.array_equal(out32.cpu().numpy().view(np.int32), want.view(np.int32)), (din, norm_box)      # rows, box columns, order, padding: bit for bit
            out16, _ = pack_box(rows, boxes, sizes, lens, out_R, F_out, torch.bfloat16, False, norm_box)
            assert torch.equal(bits(out16.cpu()), bits(out32.cpu().to(torch.bfloat16))), (din, norm_box)
            again, _ = pack_box(rows, boxes, sizes, lens, out_R, F_out, torch.float32, False, norm_box)
            assert torch.equal(bits(again.cpu()), bits(out32.cpu()))
            # norm_att = 1: the box columns and the order stay bit-equal, the attention columns are the plain launch's normalisation
            n32, att_len = pack_box(rows, boxes, sizes, lens, out_R, F_out, torch.float32, True, norm_box)
            n16, _ = pack_box(rows, boxes, sizes, lens, out_R, F_out, torch.bfloat16, True, norm_box)
            twice, _ = pack_box(rows, boxes, sizes, lens, out_R, F_out, torch.float32, True, norm_box)
            n32, n16 = n32.cpu(), n16.cpu()
            assert att_len.cpu().tolist() == want_len and torch.equal(bits(twice.cpu()), bits(n32))
            assert np.array_equal(n32.numpy()[:, :, F_att:].view(np.int32), want[:, :, F_att:].view(np.int32)), (din, norm_box)
            assert torch.equal(bits(n16), bits(n32.to(torch.bfloat16)))
            ref = want[:, :, :F_att].astype(np.float64)            # the sorted rows; no row is all zero, the padding rows stay 0
            norms = np.sqrt((ref * ref).sum(2, keepdims=True))
            ref = np.divide(ref, norms, out=np.zeros_like(ref), where=norms > 0)
            got, nz = n32.numpy()[:, :, :F_att].astype(np.float64), ref != 0
            assert np.array_equal(got == 0, ref == 0)
            err = float((np.abs(got - ref)[nz] / np.abs(ref)[nz]).max())
            worst = max(worst, err)
            assert err <= NORM_BAR, (din, norm_box, err)
    print(f"pack_regions_box norm_att F_att={F_att} B={len(lens)} out_R={out_R}: max rel err {worst:.3e} (bar {NORM_BAR:.1e})")
    record_parity(f"pack_regions_box_norm_att_f32_F{F_att}_B{len(lens)}_R{out_R}", worst, NORM_BAR, "relative, non-zero attention elements, vs the float64 norm of the restatement's sorted rows")


@pytest.mark.parametrize("dout", OUT_DTYPES)
def test_a_nan_key_goes_last_and_every_row_is_written(dout):
    F_att, F_out, lens, out_R = 64, 128, [5, 4], 6
    boxes, sizes = boxes_of([7, 4], 3)
    boxes[0] = boxes[0][:5].copy()
    boxes[0][2] = 0.0                                               # an all-zero box: 0 / 0 under norm_box, a NaN key
    rows = rows_of(F_att, lens, torch.float32)
    atts = [a.numpy() for a in torch.split(rows, lens)]
    want, _ = restated_batch(atts, boxes, sizes, out_R, F_out, False, True)
    assert np.isnan(want[0, 4, F_att:F_att + 5]).all() and not np.isnan(want[0, :4]).any() and np.array_equal(want[0, 4, :F_att], atts[0][2])
    out, att_len = pack_box(rows, boxes, sizes, lens, out_R, F_out, dout, False, True)
    out = out.cpu()
    assert att_len.cpu().tolist() == lens
    assert not (out == SENTINEL).any()                             # the ranks were a permutation: no destination row was left out
    wanted = torch.from_numpy(want) if dout == torch.float32 else torch.from_numpy(want).to(torch.bfloat16)
    assert torch.isnan(out[0, 4, F_att:F_att + 5]).all()
    keep = torch.ones(out.shape, dtype=torch.bool)
    keep[0, 4, F_att:F_att + 5] = False                            # (a NaN's payload is not pinned)
    assert torch.equal(bits(out)[keep], bits(wanted)[keep])


@pytest.mark.parametrize("dout", OUT_DTYPES)
@pytest.mark.parametrize("norm_att", [False, True])
def test_writes_stay_inside_out_and_cover_all_of_it(dout, norm_att):
    F_att, F_out, lens, out_R = 64, 80, [1, 7, 3, 10], 10          # F_out = 80: two chunks behind the attention columns, no multiple of 64
    boxes, sizes = boxes_of(lens, 11)
    n, pre, post = len(lens) * out_R * F_out, 64, 200
    big = torch.full((pre + n + post,), SENTINEL, dtype=dout, device="cuda")
    view = big[pre:pre + n].view(len(lens), out_R, F_out)
    out, _ = pack_box(rows_of(F_att, lens, torch.float16), boxes, sizes, lens, out_R, F_out, dout, norm_att, True, out=view)
    assert out.data_ptr() == view.data_ptr()
    host = big.cpu()
    assert (host[:pre] == SENTINEL).all() and (host[pre + n:] == SENTINEL).all()
    assert not (host[pre:pre + n] == SENTINEL).any()               # every element of the view was written
    if not norm_att:
        atts = [a.numpy() for a in torch.split(rows_of(F_att, lens, torch.float16).float(), lens)]
        want = torch.from_numpy(restated_batch(atts, boxes, sizes, out_R, F_out, False, True)[0]).to(dout)
        assert torch.equal(bits(host[pre:pre + n].view(want.shape)), bits(want))


# ------------------------------------------------------------------------------------------------------------------ the engine at att_feat_size = 69

LENS5 = [3, 9, 5, 7, 4]


@pytest.fixture(scope="module")
def tiny69():
    """TINY with 64 + 5 feature columns: its weights, five images of 3 to 9 regions packed by the kernel ([5, 9, 128] float32 + counts), the loader's mask.
    The weights are ``W.make_state_dict``'s: TINY's own -- the bound-head preset is calibrated on that draw, and random bound heads end every caption at
    once, which would leave nothing to compare -- with ``att_embed.0.weight`` widened by the five box columns of the 69-wide configuration's draw."""
    from boficap_amd import weights as W
    from boficap_amd.config import TINY
    cfg = dataclasses.replace(TINY, att_feat_size=69)
    sd, wide = dict(W.make_state_dict(TINY, seed=0, gen_scale=6.0)), W.make_state_dict(cfg, seed=0, gen_scale=6.0)["att_embed.0.weight"]
    sd["att_embed.0.weight"] = np.ascontiguousarray(np.concatenate([sd["att_embed.0.weight"], wide[:, 64:]], 1))
    sd = W.with_len_row_shared(sd, cfg)
    assert sd["att_embed.0.weight"].shape == (cfg.d_model, 69) and cfg.att_feat_padded == 128
    boxes, sizes = boxes_of(LENS5, 5)
    rng = np.random.default_rng(100)
    rows = torch.from_numpy(np.abs(rng.standard_normal((sum(LENS5), 64))).astype(np.float32))
    feats, att_len = pack_box(rows, boxes, sizes, LENS5, 9, 128, torch.float32, False, True)
    masks = (torch.arange(9)[None, :] < torch.tensor(LENS5)[:, None]).float()
    return cfg, sd, feats, att_len, masks


def engine_of(cfg, sd):
    from boficap_amd.engine import BofiEngine
    eng = BofiEngine(cfg, torch.float32, max_batch=8, max_regions=36)
    eng.load_state_dict(sd)
    return eng


KEYS = ("seq", "seq_logprob", "phrase_num", "phrase_length", "phrase_syn")


def test_engine_with_an_unaligned_feature_width_against_the_oracle(tiny69):
    cfg, sd, feats, att_len, masks = tiny69
    eng, w = engine_of(cfg, sd), O.as_torch(sd)
    dense = feats[..., :69].cpu().contiguous()
    for mode, decode, oracle in (("naic", eng.decode_naic, O.sample_naic), ("saic", eng.decode_saic, O.sample_saic)):
        oseq, olp, opn, opl, ops, _ = oracle(w, cfg, dense, masks)
        r = decode(feats, att_len)
        torch.cuda.synchronize()
        assert torch.equal(r["seq"].cpu(), oseq) and torch.equal(r["phrase_num"].cpu().long(), opn.long()), mode
        assert torch.equal(r["phrase_length"].cpu().long(), opl.long()) and torch.equal(r["phrase_syn"].cpu().long(), ops.long()), mode
        lp = r["seq_logprob"].cpu()
        assert torch.equal(torch.isnan(lp), torch.isnan(olp)), mode
        ok = ~torch.isnan(olp) & ~torch.isinf(olp)
        assert ok.any() and (mode == "saic" or int((oseq > 0).sum()) >= 20)        # there is something to compare: finite log-probs, real captions
        err =float((lp[ok] - olp[ok]).abs().max())
        print(f"engine att_feat_size 69, {mode}: max abs log-prob error {err:.3e} (bar 1e-3)")
        record_parity(f"box_engine_f32_tiny69_{mode}_logprob", err, 1e-3, "float32 engine at att_feat_size 69 (K padded to 128) vs the float32 oracle on out[..., :69]")
        assert err < 1e-3, mode
    with pytest.raises(Exception, match="128"):                    # the engine itself takes the padded width only
        eng.decode_naic(feats[..., :69].contiguous(), att_len)


def test_padded_engine_equals_an_engine_of_the_padded_width(tiny69):
    from boficap_amd.config import TINY
    cfg, sd, feats, att_len, _ = tiny69
    sd128 = dict(sd)
    sd128["att_embed.0.weight"] = np.ascontiguousarray(np.pad(np.asarray(sd["att_embed.0.weight"], np.float32), ((0, 0), (0, 128 - 69))))
    a, b = engine_of(cfg, sd), engine_of(dataclasses.replace(TINY, att_feat_size=128), sd128)
    assert same(a.encode(feats, att_len), b.encode(feats, att_len))
    for name in ("decode_naic", "decode_saic"):
        ra, rb = getattr(a, name)(feats, att_len), getattr(b, name)(feats, att_len)
        torch.cuda.synchronize()
        for k in KEYS + ("bound_iters",):
            assert same(ra[k], rb[k]), (name, k)


def model_of(cfg, sd):
    import captioning.models as models
    opt = cfg.to_opt()
    opt.bofi_compute_dtype, opt.bofi_max_batch = torch.float32, 8
    model = models.setup(opt)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return model.cuda().eval()


def test_refresh_path_and_dense_input_through_the_module(tiny69):
    cfg, sd, feats, att_len, masks = tiny69
    masks, fc = masks.cuda(), torch.zeros(5, 0, device="cuda")
    opt = {"train_mode": "NAIC", "sample_method": "greedy", "sample_n": 1}
    model = model_of(cfg, sd)
    assert model.state_dict()["att_embed.0.weight"].shape == (cfg.d_model, 69)      # the schema keeps the unpadded width
    with torch.no_grad():
        first = model(fc, feats, masks, opt=opt, mode="sample")[:5]
        dense = model(fc, feats[..., :69].contiguous(), masks, opt=opt, mode="sample")[:5]      # the reference's call convention: zero-padded with torch
        assert same(list(dense), list(first))
        eng = model.engine()
        weight = dict(model.named_parameters())["att_embed.0.weight"]
        weight.mul_(-0.75).add_(0.01)                              # in place: the engine is refreshed on the device, through its padded copy
        moved = model(fc, feats, masks, opt=opt, mode="sample")[:5]
        assert model.engine() is eng and eng._att_w_padded.shape == (cfg.d_model, 128) and not bool(eng._att_w_padded[:, 69:].any())
        fresh_sd = dict(sd)
        fresh_sd["att_embed.0.weight"] = weight.detach().cpu().numpy()
        fresh = model_of(cfg, fresh_sd)(fc, feats, masks, opt=opt, mode="sample")[:5]
    assert same(list(moved), list(fresh))
    assert not same(moved[1], first[1])                            # the weights really moved
    saic = {"train_mode": "SAIC", "sample_method": "greedy", "sample_n": 1}
    with torch.no_grad():
        assert same(list(model(fc, feats[..., :69].contiguous(), masks, opt=saic, mode="sample")[:5]), list(model(fc, feats, masks, opt=saic, mode="sample")[:5]))


# ------------------------------------------------------------------------------------------------------------------ end to end

SPLITS = ["train", "val", "train", "restval", "val", "test", "train", "val"]
IDS = [7000 + 11 * i for i in range(len(SPLITS))]
REGIONS = [12, 36, 5, 20, 36, 9, 1, 36]                           # the val images fill the 36-region bucket: the dense array is the loader's batch, no mask


def box_dataset(tmp_path):
    rng = np.random.default_rng(17)
    images = [np.abs(rng.standard_normal((l, 64))).astype(np.float16 if i % 2 else np.float32) for i, l in enumerate(REGIONS)]
    boxes, sizes = boxes_of(REGIONS, 19)
    att, box = tmp_path / "att", tmp_path / "box"
    att.mkdir()
    box.mkdir()
    for i, a, q in zip(IDS, images, boxes):
        np.savez(att / f"{i}.npz", feat=a)
        np.save(box / f"{i}.npy", q)
    talk = tmp_path / "talk.json"
    talk.write_text(json.dumps({"images": [{"id": i, "split": s, "width": w, "height": h} for i, s, (w, h) in zip(IDS, SPLITS, sizes)]}))
    return str(att), str(box), str(talk), images, boxes, sizes


def test_decode_many_over_box_batches_equals_the_dense_arrays(tmp_path, tiny69):
    from boficap_amd.features import BoxRaggedBatch, ImageIndex, RegionSource, RegionStore
    cfg, sd = tiny69[:2]
    att, box, talk, images, boxes, sizes = box_dataset(tmp_path)
    index = ImageIndex(talk)
    ixs = list(range(len(IDS)))
    assert index.sizes(ixs).tolist() == [list(s) for s in sizes]
    model = model_of(cfg, sd)
    keys = ("seq", "phrase_num", "phrase_length", "phrase_syn", "entropy", "perplexity")
    for norm_box in (False, True):
        source = RegionSource(RegionStore(att), IDS, box_store=RegionStore(box, ".npy"), sizes=index.sizes(ixs), norm_box_feat=norm_box)
        ragged = [source.ragged(0, 4), source.ragged(4, 8)]
        assert all(isinstance(r, BoxRaggedBatch) and r.F_out == 128 for r in ragged)
        dense = []
        for i0 in (0, 4):
            lens = REGIONS[i0:i0 + 4]
            arr, _ = restated_batch([a.astype(np.float32) for a in images[i0:i0 + 4]], boxes[i0:i0 + 4], sizes[i0:i0 + 4], max(lens), 69, False, norm_box)
            dense.append((arr, (np.arange(max(lens))[None, :] < np.array(lens)[:, None]).astype(np.float32)))
        with torch.no_grad():
            got = [{k: r[k].clone() for k in keys} for r in model.decode_many(ragged)]
            want = [{k: r[k].clone() for k in keys} for r in model.decode_many(dense)]
        assert len(got) == len(want) == 2
        for a, b in zip(got, want):
            for k in keys:
                assert same(a[k], b[k]), (norm_box, k)


def test_tools_eval_reads_box_features(tmp_path, tiny69):
    """tools/eval.py --use_box 1 --input_box_dir in a fresh process: the captions of eval_split on the dense [N, 36, 69] array the loader would have built."""
    from boficap_amd import eval_utils
    cfg, sd = tiny69[:2]
    att, box, talk, images, boxes, sizes = box_dataset(tmp_path)
    pth, pkl, dump = (str(tmp_path / f) for f in ("model.pth", "infos.pkl", "out.json"))
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, pth)
    opt = cfg.to_opt()
    with open(pkl, "wb") as f:
        pickle.dump({"opt": opt, "vocab": opt.vocab}, f, protocol=2)
    cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tools", "eval.py"), "--model", pth, "--infos_path", pkl, "--batch_size", "2", "--dtype", "f32",
           "--input_att_dir", att, "--input_json", talk, "--split", "val", "--use_box", "1", "--input_box_dir", box, "--norm_box_feat", "1", "--dump_json", dump,
           "--feeder_workers", "2"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    with open(dump) as f:
        dumped = json.load(f)
    val = [i for i, s in enumerate(SPLITS) if s == "val"]
    assert [p["image_id"] for p in dumped] == [IDS[i] for i in val]
    dense, _ = restated_batch([images[i].astype(np.float32) for i in val], [boxes[i] for i in val], [sizes[i] for i in val], 36, 69, False, True)
    _, pred, _ = eval_utils.eval_split(model_of(cfg, sd), dense, None, {"batch_size": 2, "vocab": opt.vocab})
    for got, want in zip(dumped, pred):
        assert sorted(got) == sorted(want) and got["seq"] == want["seq"] and got["caption"] == want["caption"]
        assert got["phrase_num"] == want["phrase_num"] and got["phrase_length"] == want["phrase_length"]
        for k in ("entropy", "perplexity"):                        # (the json keeps a float's digits; a NaN equals a NaN)
            assert got[k] == want[k] or (got[k] != got[k] and want[k] != want[k]), k
    assert len(dumped) == len(pred) == 3 and any(p["seq"] for p in dumped)
    # a model of the plain width is refused with both numbers before the device is touched
    plain = dataclasses.replace(cfg, att_feat_size=64).to_opt()
    with open(pkl, "wb") as f:
        pickle.dump({"opt": plain, "vocab": plain.vocab}, f, protocol=2)
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 2 and "att_feat_size is 64" in out.stderr and "69" in out.stderr, out.stderr[-1000:]
