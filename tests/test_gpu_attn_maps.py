"""Word-to-region attention maps on the MI355X: the stand-alone kernel against the float64 restatement (tests/test_attn_maps.py), the float32 engine against the
oracle's own softmax(scores) -- recorded by a wrapper around boficap_oracle.attention while the oracle decodes --, the bf16 engine against the oracle's filling pass
on the engine's slot layout plus the exact self-consistency of its outputs, "nothing else moves", and the interface above the engine."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import boficap_oracle as O
from conftest import record_parity
from test_attn_maps import maps_np, topk_np
from test_mask_predict import _case

pytestmark = pytest.mark.gpu

LAYOUT = ("phrase_num", "phrase_length", "phrase_syn")
SENT = -7.0
# Absolute bars on probabilities, each 2x the maximum measured on the MI355X over the cases it serves (record_parity keeps every run's figures; this round's are in
# profiles/r14_attn_maps_parity.json).
#   BAR_KERNEL: the derived bar is 1e-4 -- inputs are drawn with sum |q_i k_i| * scale <= 8, so a score's float32 accumulation error is at most about 64 * 2^-24 * 8 = 3e-5
#               and a probability's about twice that times p.  Measured: 7.0e-8 at worst (two_chunks, float32) -- the terms' signs cancel and the probabilities are small --,
#               so the bar is tightened to 2x that.
#   BAR_F32:    float32 engine against the oracle's p_attn: 1.7e-7 at worst (tiny_ragged).  The top-1 check's near-tie threshold, 1e-5, stays far above twice the bar.
#   BAR_BF16:   bf16 engine against the oracle's filling pass on the engine's layout: 1.2e-3 at worst (FULL, 100 regions, ragged; 5.8e-4 .. 8.6e-4 elsewhere).
BAR_KERNEL = 1.4e-7
BAR_F32 = 3.5e-7
BAR_BF16 = 2.5e-3


def _bits(t):
    return t.contiguous().view(torch.int32)


# ----------------------------------------------------------------------------- the oracle's maps
class _Recorder:
    """While active, boficap_oracle.attention also keeps softmax(scores) per parameter prefix (the last call's: the last pass of a refined decode) -- p_attn, an
    intermediate of the very code the goldens pin to the reference -- and calls the original."""

    def __enter__(self):
        self.maps, self.orig = {}, O.attention

        def wrapped(w, p, q_in, kv_in, mask, h):
            B, _, d = q_in.shape
            dk = d // h
            q = O.linear(q_in, w, p + ".linears.0").view(B, -1, h, dk).transpose(1, 2)
            k = O.linear(kv_in, w, p + ".linears.1").view(B, -1, h, dk).transpose(1, 2)
            scores = (torch.matmul(q, k.transpose(-2, -1)) / dk ** 0.5).masked_fill(mask.unsqueeze(1) == 0, O.NEG_INF)
            self.maps[p] = F.softmax(scores, dim=-1).clone()
            return self.orig(w, p, q_in, kv_in, mask, h)
        O.attention = wrapped
        return self

    def __exit__(self, *exc):
        O.attention = self.orig


def _oracle_fill_maps(cfg, sd, att, masks, ext_syn, last, group, layer):
    """softmax(scores) [B, h, S, Lk] of decoder layer ``layer``'s cross-attention in the oracle's filling pass on a GIVEN slot layout (quirk Q1 per ``group`` images)."""
    w = O.as_torch(sd)
    B, S = att.size(0), cfg.seq_length
    with torch.no_grad(), _Recorder() as rec:
        memory, src_mask = O.memory_of(w, cfg, att, masks)
        syn_mask = torch.zeros(B, S, S, dtype=torch.bool)
        for i in range(B):
            n = int(last[(i // group) * group + group - 1]) - 1
            syn_mask[i, :, :max(n, 0)] = True
        O.decode_na(w, cfg, memory, ext_syn[:, 1:-1], src_mask, syn_mask)
    return rec.maps[f"model.decoder.layers.{layer}.src_attn"].numpy()


def _against(got, want):
    """max |got - want| over the oracle's columns; the NaN patterns must agree and the engine's columns past the oracle's (the loader clips a batch to its longest
    image) must be exact zeros on every row that is not NaN."""
    got, want = np.asarray(got), np.asarray(want)
    Lo = want.shape[-1]
    assert np.array_equal(np.isnan(got[..., :Lo]), np.isnan(want)), "NaN pattern differs"
    tail = got[..., Lo:]
    if tail.shape[-1]:
        assert ((tail == 0) | np.isnan(tail)).all() and np.array_equal(np.isnan(tail).any(-1), np.isnan(tail).all(-1))
    d = np.abs(got[..., :Lo] - want)
    return float(np.nanmax(d)) if (~np.isnan(d)).any() else 0.0


def _self_consistent(out, att_len, K):
    """What holds exactly for the engine's own outputs: mean = head-ordered float32 sum of heads / H; the top-K is the stable descending order of mean with mean's
    floats; rows sum to 1 over r < len_b within 1e-5 and are exact zeros beyond."""
    mean, heads = out["attn"].cpu().numpy(), out["attn_heads"].cpu().numpy()
    B, H, S, R = heads.shape
    acc = heads[:, 0].copy()
    for h in range(1, H):
        acc = acc + heads[:, h]
    assert np.array_equal(mean, acc / np.float32(H), equal_nan=True)
    lens = np.full(B, R) if att_len is None else att_len.cpu().numpy()
    n_tok = out["phrase_length"].sum(1).cpu().numpy()
    idx, w = topk_np(mean, K, lens, n_tok)
    assert np.array_equal(out["attn_top"].cpu().numpy(), idx)
    assert np.array_equal(out["attn_top_w"].cpu().numpy().view(np.int32)[~np.isnan(w)], w.view(np.int32)[~np.isnan(w)])
    assert np.array_equal(np.isnan(out["attn_top_w"].cpu().numpy()), np.isnan(w))
    for b in range(B):
        rows = mean[b][~np.isnan(mean[b]).any(1)]
        assert (rows[:, lens[b]:] == 0).all() and not np.signbit(rows[:, lens[b]:]).any()
        if lens[b] > 0 and len(rows):
            assert np.abs(rows[:, :lens[b]].astype(np.float64).sum(1) - 1).max() < 1e-5


# ----------------------------------------------------------------------------- 1. the stand-alone kernel
KERNEL_CASES = {
    # B, H, Lq, Lk, K and what else the case is about
    "b3_h2": dict(B=3, H=2, Lq=20, Lk=36, K=4),
    "ragged_100": dict(B=3, H=8, Lq=20, Lk=100, K=8, klen=[1, 100, 57]),
    "lk1": dict(B=2, H=2, Lq=3, Lk=1, K=1),
    "lk64": dict(B=2, H=2, Lq=5, Lk=64, K=4, klen=[64, 63]),
    "lk65_h9": dict(B=2, H=9, Lq=5, Lk=65, K=4, klen=[65, 64]),                    # the second key of a lane; heads looped over the wavefronts
    "lk128": dict(B=2, H=2, Lq=5, Lk=128, K=4, klen=[128, 127]),
    "lq1": dict(B=2, H=2, Lq=1, Lk=36, K=1),
    "pitches": dict(B=2, H=2, Lq=20, Lk=36, K=4, ldq=3, ldk=6),                     # 3 d and 6 d: the packed q|k|v and a stacked K|V
    "unaligned": dict(B=2, H=2, Lq=7, Lk=70, K=4, ldq_plus=3, ldk_plus=1),          # pitches that rule out 16-byte loads
    "k8_short": dict(B=3, H=2, Lq=4, Lk=36, K=8, klen=[3, 5, 0]),                   # K > klen, and an image without keys
    "ties": dict(B=2, H=2, Lq=6, Lk=8, K=8, same_keys=(3, 7)),                      # (all eight keys are in every row's top-K)
    "nan_row": dict(B=2, H=2, Lq=6, Lk=36, K=4, klen=[36, 20], nan_rows=[(0, 2), (1, 4)]),
    "qlen": dict(B=3, H=2, Lq=20, Lk=36, K=4, qlen=[5, 1, 21], qlen_bias=-1),
    "chunks": dict(B=2, H=16, Lq=20, Lk=128, K=4, klen=[128, 70]),                  # many heads: the wavefronts loop twice
    "one_chunk": dict(B=520, H=2, Lq=20, Lk=36, K=3),                               # launches of 512 images or more: all of an image's rows in one workgroup
    "two_chunks": dict(B=300, H=2, Lq=20, Lk=36, K=3, klen=[36, 7] * 150),          # ... below that its rows are split over workgroups (every case above: one row each)
    "max": dict(B=2, H=8, Lq=64, Lk=128, K=8),
    "max_lds": dict(B=520, H=4, Lq=64, Lk=128, K=2),                                # 64 rows do not fit the LDS budget: chunks of 48 even in a large launch
}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_kernel_equals_the_restatement(name, dtype):
    """Every output element is written (sentinel-filled buffers), A and M are within BAR_KERNEL of the float64 restatement on the same rounded inputs, and the
    outputs are exactly consistent with each other.  Measured on the MI355X: 2e-9 .. 7.0e-8 over the cases, both dtypes."""
    from boficap_amd import hip
    c = KERNEL_CASES[name]
    B, H, Lq, Lk, K = c["B"], c["H"], c["Lq"], c["Lk"], c["K"]
    d = 64 * H
    ldq, ldk = d * c.get("ldq", 1) + c.get("ldq_plus", 0), d * c.get("ldk", 1) + c.get("ldk_plus", 0)
    rng = np.random.default_rng(sum(map(ord, name)))
    q = torch.from_numpy(rng.uniform(-1, 1, (B * Lq, ldq)).astype(np.float32))          # |q_i|, |k_i| <= 1: sum |q_i k_i| / 8 <= 8
    k = torch.from_numpy(rng.uniform(-1, 1, (B * Lk, ldk)).astype(np.float32))
    if "same_keys" in c:
        i, j = c["same_keys"]
        for b in range(B):
            k[b * Lk + j] = k[b * Lk + i]
    q, k = q.to(dtype), k.to(dtype)
    for b, t in c.get("nan_rows", []):
        q[b * Lq + t, 5 if b == 0 else slice(None)] = float("nan")                     # one element of head 0; a whole row
    klen, qlen, bias = c.get("klen"), c.get("qlen"), c.get("qlen_bias", 0)
    dq, dk_ = q.cuda(), k.cuda()
    mean = torch.full((B, Lq, Lk), SENT, device="cuda")
    heads = torch.full((B, H, Lq, Lk), SENT, device="cuda")
    top = torch.full((B, Lq, K), int(SENT), dtype=torch.int32, device="cuda")
    topw = torch.full((B, Lq, K), SENT, device="cuda")
    hip.attn_maps(dq, dk_, B, H, Lq, Lk, scale=0.125, klen=None if klen is None else torch.tensor(klen, dtype=torch.int32, device="cuda"),
                  qlen=None if qlen is None else torch.tensor(qlen, dtype=torch.int32, device="cuda"), qlen_bias=bias, mean=mean, heads=heads, K=K, top_idx=top, top_w=topw)
    torch.cuda.synchronize()
    mean, heads, top, topw = mean.cpu().numpy(), heads.cpu().numpy(), top.cpu().numpy(), topw.cpu().numpy()
    for a in (mean, heads, top, topw):
        assert not (a == SENT).any()
    A, M = maps_np(q.float().numpy(), k.float().numpy(), B, H, Lq, Lk, 0.125, klen)
    assert np.array_equal(np.isnan(heads), np.isnan(A)) and np.array_equal(np.isnan(mean), np.isnan(M))
    err = max(float(np.nanmax(np.abs(heads - A))), float(np.nanmax(np.abs(mean - M))))
    print(f"attn_maps kernel {name} {dtype}: max |A - float64| {err:.3e}")
    record_parity(f"attn_maps_kernel_{name}_{'f32' if dtype == torch.float32 else 'bf16'}", err, BAR_KERNEL, "stand-alone kernel against the float64 restatement on the same inputs")
    assert err < BAR_KERNEL
    lens = [Lk] * B if klen is None else klen
    for b in range(B):                                          # exact zeros (+0.0) past an image's keys
        z = heads[b][..., lens[b]:][~np.isnan(heads[b][..., lens[b]:])]
        assert (z == 0).all() and not np.signbit(z).any()
    acc = heads[:, 0].copy()
    for h in range(1, H):
        acc = acc + heads[:, h]
    assert np.array_equal(mean, acc / np.float32(H), equal_nan=True)
    idx, w = topk_np(mean, K, klen, None if qlen is None else [v + bias for v in qlen])
    assert np.array_equal(top, idx)
    assert np.array_equal(np.isnan(topw), np.isnan(w)) and np.array_equal(topw.view(np.int32)[~np.isnan(w)], w.view(np.int32)[~np.isnan(w)])
    if "same_keys" in c:                                        # equal weights, lower index first -- and not vacuous: both are among some row's top-K
        i, j = c["same_keys"]
        assert np.array_equal(mean[..., i].view(np.int32), mean[..., j].view(np.int32))
        both = [(list(r).index(i), list(r).index(j)) for r in top.reshape(-1, K) if i in r and j in r]
        assert both and all(pj == pi + 1 for pi, pj in both)
    if "nan_rows" in c:
        assert np.isnan(mean[0, 2]).all() and np.isnan(heads[0, 0, 2]).all() and not np.isnan(heads[0, 1, 2]).any()
        assert np.isnan(heads[1, :, 4]).all() and (top[1, 4] == -1).all() and np.isnan(topw[1, 4]).all()


# ----------------------------------------------------------------------------- 2. the float32 engine against the oracle
@pytest.fixture(scope="module")
def tiny_f32():
    from boficap_amd.engine import BofiEngine
    cfg, sd, _, _ = _case("tiny_mix")
    eng = BofiEngine(cfg, torch.float32, max_batch=64, max_regions=36)
    eng.load_state_dict(sd)
    return cfg, sd, eng


def _oracle_decode_maps(name, layer, rounds=0):
    cfg, sd, att, masks = _case(name)
    w = O.as_torch(sd)
    with torch.no_grad(), _Recorder() as rec:
        r = O.sample_naic_refine(w, cfg, att, masks, rounds=rounds) if rounds else O.sample_naic(w, cfg, att, masks)
    return rec.maps[f"model.decoder.layers.{layer}.src_attn"].numpy(), r


@pytest.mark.parametrize("name", ["tiny_mix", "tiny_ragged", "tiny_ragged_short", "tiny_single", "tiny_q1_last_empty_nan"])
def test_f32_engine_equals_the_oracle_maps(name, tiny_f32):
    """attn and attn_heads of the last decoder layer against the oracle's p_attn; the top-1 region of every emitted word whose oracle top-two gap exceeds 1e-5 is the
    oracle's arg-max (at most 5 % of the words skipped as near-ties; the oracle alone skips none at 1e-5, its smallest gap is 1.5e-5 on tiny_mix).
    Measured on the MI355X: 4.8e-8 .. 1.7e-7 over the cases."""
    cfg, sd, eng = tiny_f32
    _, sd_case, att, masks = _case(name)
    assert sd_case is sd or all(np.array_equal(sd_case[k], sd[k]) for k in sd)      # (every TINY case but the patched SAIC one shares tiny_mix's weights)
    want, ref = _oracle_decode_maps(name, cfg.N_dec - 1)
    att_len = None if masks is None else masks.sum(1).to(torch.int32).cuda()
    K = 3
    out = eng.decode_naic(att.cuda(), att_len, attn_maps=True, attn_heads=True, attn_topk=K)
    torch.cuda.synchronize()
    assert np.array_equal(out["seq"].cpu().numpy(), ref[0].numpy()) and all(np.array_equal(out[k].cpu().numpy(), v.numpy()) for k, v in zip(LAYOUT, ref[2:5]))
    err = max(_against(out["attn_heads"].cpu().numpy(), want), _against(out["attn"].cpu().numpy(), want.mean(1)))
    print(f"attn maps f32 engine {name}: max |attn - oracle| {err:.3e}")
    record_parity(f"attn_maps_f32_engine_{name}", err, BAR_F32, "float32 engine, last decoder layer's cross-attention probabilities, against the oracle's p_attn")
    assert err < BAR_F32
    _self_consistent(out, att_len, K)
    top = out["attn_top"].cpu().numpy()
    n_tok = out["phrase_length"].sum(1).cpu().numpy()
    lens = np.full(att.size(0), want.shape[-1]) if masks is None else masks.sum(1).long().numpy()
    om = want.mean(1)
    words = skipped = 0
    for b in range(att.size(0)):
        for t in range(int(n_tok[b])):
            row = om[b, t, :lens[b]]
            words += 1
            if np.isnan(row).any():
                assert (top[b, t] == -1).all()
                continue
            srt = np.sort(row)
            if len(srt) > 1 and not srt[-1] - srt[-2] > 1e-5:
                skipped += 1
                continue
            assert top[b, t, 0] == int(np.argmax(row)), (b, t)
    assert words and 20 * skipped <= words, (skipped, words)
    if name == "tiny_q1_last_empty_nan":
        assert np.isnan(out["attn"].cpu().numpy()).all() and (top == -1).all()


def test_f32_engine_other_layer_and_refined_pass(tiny_f32):
    """attn_layer=0 against the oracle's layer 0; refine_rounds=1 against the last pass of the oracle's sample_naic_refine(rounds=1)."""
    cfg, sd, eng = tiny_f32
    _, _, att, _ = _case("tiny_mix")
    want0, _ = _oracle_decode_maps("tiny_mix", 0)
    out = eng.decode_naic(att.cuda(), attn_maps=True, attn_heads=True, attn_layer=0)
    torch.cuda.synchronize()
    e0 = _against(out["attn_heads"].cpu().numpy(), want0)
    want_last, _ = _oracle_decode_maps("tiny_mix", cfg.N_dec - 1)
    assert float(np.nanmax(np.abs(want0 - want_last))) > 100 * BAR_F32          # (not vacuous: the two layers' maps differ)
    want1, ref1 = _oracle_decode_maps("tiny_mix", cfg.N_dec - 1, rounds=1)
    out1 = eng.decode_naic(att.cuda(), attn_maps=True, attn_heads=True, refine_rounds=1)
    torch.cuda.synchronize()
    assert np.array_equal(out1["seq"].cpu().numpy(), ref1[0].numpy())
    e1 = _against(out1["attn_heads"].cpu().numpy(), want1)
    assert float(np.nanmax(np.abs(want1 - want_last))) > 100 * BAR_F32          # (... and so do the two passes')
    print(f"attn maps f32 engine: layer 0 {e0:.3e}, refined pass {e1:.3e}")
    record_parity("attn_maps_f32_engine_layer0", e0, BAR_F32, "float32 engine, attn_layer=0, against the oracle's layer 0")
    record_parity("attn_maps_f32_engine_refine1", e1, BAR_F32, "float32 engine, refine_rounds=1, against the last pass of the oracle's refinement")
    assert e0 < BAR_F32 and e1 < BAR_F32


# ----------------------------------------------------------------------------- 3. the bf16 engine
@pytest.fixture(scope="module")
def full_weights(weight_cache, manifest):
    m = manifest["full_b8"]
    return weight_cache(m["config"], m["seed"], m["gen_scale"], m["digest"], m.get("patch"))


def _bf16_against_oracle(cfg, sd, eng, att, masks, tag, group=0, compare=None, **kw):
    """Decode on the bf16 engine, then the oracle's filling pass on the ENGINE's slot layout (a bf16 bounding pass may lay a caption out differently from the float32
    oracle's, and the maps are a function of the layout) and the same bf16-rounded features.  Returns (out, max error over the first ``compare`` images)."""
    att_len = None if masks is None else masks.sum(1).to(torch.int32).cuda()
    out = eng.decode_naic(att.cuda(), att_len, attn_maps=True, attn_heads=True, attn_topk=3, q1_group=group, **kw)
    torch.cuda.synchronize()
    n = compare or att.size(0)
    ext, last = O.layout_of(cfg, {k: out[k][:n] for k in LAYOUT})
    want = _oracle_fill_maps(cfg, sd, att[:n].float(), None if masks is None else masks[:n], ext, last, group or n, cfg.N_dec - 1)
    err = max(_against(out["attn_heads"][:n].cpu().numpy(), want), _against(out["attn"][:n].cpu().numpy(), want.mean(1)))
    print(f"attn maps bf16 engine {tag}: max |attn - oracle| {err:.3e}")
    _self_consistent(out, att_len, 3)
    return out, err


def test_bf16_tiny_engine():
    """Measured on the MI355X: 4.4e-4 (tiny_mix), 8.6e-4 (tiny_ragged)."""
    from boficap_amd.engine import BofiEngine
    cfg, sd, _, _ = _case("tiny_mix")
    eng = BofiEngine(cfg, torch.bfloat16, max_batch=64, max_regions=36)
    eng.load_state_dict(sd)
    for name in ("tiny_mix", "tiny_ragged"):
        _, _, att, masks = _case(name)
        _, err = _bf16_against_oracle(cfg, sd, eng, att.to(torch.bfloat16), masks, name)
        record_parity(f"attn_maps_bf16_engine_{name}", err, BAR_BF16, "bf16 engine against the oracle's filling pass on the engine's layout")
        assert err < BAR_BF16


@pytest.mark.parametrize("R", [36, 100])
def test_bf16_full_engine(R, full_weights):
    """FULL, 8 images: 36 regions, and 100 regions with ragged counts (the split attention sublayer: more than 48 keys).  Measured on the MI355X: 5.8e-4 and 1.2e-3."""
    from boficap_amd import weights as W
    from boficap_amd.engine import BofiEngine
    cfg, sd = full_weights
    eng = BofiEngine(cfg, torch.bfloat16, max_batch=8, max_regions=R)
    eng.load_state_dict(sd)
    att = torch.from_numpy(W.synthetic_att_feats(8, R, cfg.att_feat_size, seed=41 + R)).to(torch.bfloat16)
    masks = None
    if R == 100:
        masks = (torch.arange(R)[None, :] < torch.tensor([100, 10, 57, 64, 65, 99, 33, 100])[:, None]).float()
    _, err = _bf16_against_oracle(cfg, sd, eng, att, masks, f"full R={R}")
    record_parity(f"attn_maps_bf16_engine_full_r{R}", err, BAR_BF16, "bf16 engine against the oracle's filling pass on the engine's layout")
    assert err < BAR_BF16


def test_bf16_large_launch_forms(full_weights):
    """512 images as 8 batches of 64 in one launch -- large enough for the row-block family, where the query projection rides another launch -- against the oracle on
    the first batch (measured on the MI355X: 6.0e-4; the fused generator and the persistent bounding loop both ran); the same maps bit for bit from a graph replay,
    the phased form and an ids-only fork."""
    from boficap_amd import weights as W
    from boficap_amd.engine import BofiEngine
    cfg, sd = full_weights
    eng = BofiEngine(cfg, torch.bfloat16, max_batch=512, max_regions=36)
    eng.load_state_dict(sd)
    att = torch.from_numpy(W.synthetic_att_feats(64, 36, cfg.att_feat_size, seed=43)).to(torch.bfloat16).repeat(8, 1, 1)      # (the same 64 images in every batch)
    forms = f"ids_only_fused(512)={eng.ids_only_fused(512)} bound_loop_active(36)={eng.bound_loop_active(36)}"
    out, err = _bf16_against_oracle(cfg, sd, eng, att, None, "full 512 images, q1_group 64: " + forms, group=64, compare=64)
    record_parity("attn_maps_bf16_engine_full_512", err, BAR_BF16, "bf16 engine, 8 x 64 images in one launch, first batch against the oracle; " + forms)
    assert err < BAR_BF16
    keys = ("attn", "attn_heads", "attn_top", "attn_top_w", "seq") + LAYOUT
    want = {k: out[k].clone() for k in keys}
    kw = dict(attn_maps=True, attn_heads=True, attn_topk=3, q1_group=64)
    datt = att.cuda()
    g = eng.decode_naic(datt, graph=True, **kw)
    g = eng.decode_naic(datt, graph=True, out=g, **kw)
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(g[k]), _bits(want[k])) if g[k].is_floating_point() else torch.equal(g[k], want[k]) for k in keys)
    ph = eng.decode_naic(datt, phases="eb", **kw)
    ph = eng.decode_naic(datt, phases="f", out=ph, **kw)
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(ph[k]), _bits(want[k])) if ph[k].is_floating_point() else torch.equal(ph[k], want[k]) for k in keys)
    f = eng.fork(ids_only=True)
    fo = f.decode_naic(datt, ids_only=True, **kw)
    torch.cuda.synchronize()
    assert torch.equal(fo["phrase_length"], want["phrase_length"])
    assert all(torch.equal(_bits(fo[k]), _bits(want[k])) for k in ("attn", "attn_heads", "attn_top_w")) and torch.equal(fo["attn_top"], want["attn_top"])


# ----------------------------------------------------------------------------- 4. nothing else moves
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_nothing_else_moves(dtype, tiny_f32):
    from boficap_amd import hip
    from boficap_amd.engine import BofiEngine
    cfg, sd, eng = tiny_f32
    if dtype == torch.bfloat16:
        eng = BofiEngine(cfg, dtype, max_batch=64, max_regions=36)
        eng.load_state_dict(sd)
    _, _, att, _ = _case("tiny_mix")
    att = att.cuda().to(dtype)
    keys = ("seq", "seq_logprob", "row_plogp", "row_chosen") + LAYOUT
    same = lambda a, b, ks: all(torch.equal(_bits(a[k]), _bits(b[k])) if a[k].is_floating_point() else torch.equal(a[k], b[k]) for k in ks)
    off = eng.decode_naic(att, row_stats=True)
    assert not any(k.startswith("attn") for k in off)
    on = eng.decode_naic(att, row_stats=True, attn_topk=3, attn_maps=True, attn_heads=True)
    torch.cuda.synchronize()
    assert same(on, off, keys)
    _self_consistent(on, None, 3)
    # two graph replays into the same buffers
    g = eng.decode_naic(att, row_stats=True, graph=True, attn_topk=3, attn_maps=True, attn_heads=True)
    first = {k: g[k].clone() for k in ("attn", "attn_heads", "attn_top", "attn_top_w")}
    ptrs = {k: g[k].data_ptr() for k in first}
    g["attn"].fill_(SENT)
    g = eng.decode_naic(att, row_stats=True, graph=True, out=g, attn_topk=3, attn_maps=True, attn_heads=True)
    torch.cuda.synchronize()
    assert all(g[k].data_ptr() == p for k, p in ptrs.items()) and same(g, first, first) and same(g, on, tuple(first) + keys)
    # the semi-autoregressive decode refuses a call whose options carry an attention output (BOFI_ERR_STATE, before any launch); the options of the decodes above ended
    # with them: a decode without the options writes no maps, and a semi-autoregressive decode right behind an attention decode runs
    import ctypes as C
    so = eng.decode_saic(att)
    o = hip.BofiCallOpts(attn_layer=-1, attn_mean=g["attn"].data_ptr())
    rc = hip.lib().bofi_engine_decode_saic(eng._h, hip.ptr(att), hip.dtype_code(att), None, att.size(0), att.size(1), 0, hip.ptr(so["seq"]), hip.ptr(so["seq_logprob"]),
                                           hip.ptr(so["phrase_num"]), hip.ptr(so["phrase_length"]), hip.ptr(so["phrase_syn"]), hip.ptr(so["bound_iters"]), C.byref(o), hip.stream_ptr())
    assert rc == 3
    with pytest.raises(hip.BofiHipError, match="attention output"):
        hip.check(rc, "bofi_engine_decode_saic")
    again = eng.decode_naic(att, row_stats=True)
    torch.cuda.synchronize()
    assert not any(k.startswith("attn") for k in again) and same(again, off, keys)
    eng.decode_saic(att)
    # mask-predict: the last pass's maps
    mp = eng.decode_naic(att, refine_rounds=2, refine_method="mask_predict", attn_topk=3, attn_maps=True, attn_heads=True)
    torch.cuda.synchronize()
    _self_consistent(mp, None, 3)
    plain_mp = eng.decode_naic(att, refine_rounds=2, refine_method="mask_predict")
    torch.cuda.synchronize()
    assert same(mp, plain_mp, ("seq", "seq_logprob", "refine_round") + LAYOUT)
    # the filling pass alone on a given layout: the decode's own maps
    ext, last = O.layout_of(cfg, on)
    eng.encode(att)
    res = eng.fill_naic(ext.to(torch.int32).cuda(), torch.from_numpy(last).to(torch.int32).cuda(), att.size(1), attn_maps=True, attn_topk=3)
    torch.cuda.synchronize()
    assert len(res) == 3 and torch.equal(res[0], on["seq"]) and same(res[2], on, ("attn", "attn_top", "attn_top_w"))
    assert len(eng.fill_naic(ext.to(torch.int32).cuda(), torch.from_numpy(last).to(torch.int32).cuda(), att.size(1))) == 2


# ----------------------------------------------------------------------------- 5. above the engine
def test_pipeline_sample_and_eval():
    """decode_many(attn_topk=3) over five TINY batches -- three dense ones that share a launch and two ragged ones that land in two region buckets -- equals the
    per-batch decode_naic results exactly and never names a padding column; mode='sample' leaves the tensors in model.last_attn; eval_split fills 'regions'."""
    import captioning.models as models
    from boficap_amd import eval_utils, hip
    from boficap_amd.engine import BofiEngine
    cfg, sd, att, _ = _case("tiny_mix")
    att = att[[0, 3, 1, 2, 4, 5, 6, 7]]                                            # (no batch below ends on an image without phrases: quirk Q1 would make it all NaN)
    opt = cfg.to_opt()
    opt.bofi_compute_dtype, opt.bofi_max_batch, opt.bofi_max_regions = torch.float32, 16, 64
    model = models.setup(opt)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    model.cuda().eval()
    wide = torch.cat([att[:4], att[4:, :14]], 1)                                   # [4, 50, F]
    lens_d, lens_e = torch.tensor([12, 1, 25, 30], dtype=torch.int32), torch.tensor([40, 37, 45, 50], dtype=torch.int32)
    mask = lambda lens, R: (torch.arange(R)[None, :] < lens[:, None]).float()
    items = [att[:4], att[4:], att[[3, 0, 5, 6]], (att[:4, :30].contiguous(), mask(lens_d, 30)), (wide, mask(lens_e, 50))]
    ref = BofiEngine(cfg, torch.float32, max_batch=16, max_regions=64)
    ref.load_state_dict(sd)
    ref.set_decodes_in_flight(2)
    want = []
    for it in items:
        a, m = it if isinstance(it, tuple) else (it, None)
        R = 36 if a.size(1) <= 36 else 64                                          # the pipeline's region bucket: zero rows behind the batch's own
        pad = torch.zeros(a.size(0), R, a.size(2))
        pad[:, :a.size(1)] = a
        r = ref.decode_naic(pad.cuda(), None if m is None else m.sum(1).to(torch.int32).cuda(), attn_topk=3, attn_maps=True, want_logprob=False)
        torch.cuda.synchronize()
        want.append({k: r[k].cpu() for k in ("seq", "attn", "attn_top", "attn_top_w") + LAYOUT})
    got = list(model.decode_many([(i[0].pin_memory(), i[1]) if isinstance(i, tuple) else i.pin_memory() for i in items], batches_per_launch=4, in_flight=2,
                                 attn_topk=3, keep_attn=True))
    assert len(got) == 5
    for i, (g, w) in enumerate(zip(got, want)):
        for k in ("seq", "attn_top") + LAYOUT:
            assert torch.equal(g[k], w[k]), (i, k)
        assert torch.equal(_bits(g["attn_top_w"]), _bits(w["attn_top_w"])) and torch.equal(_bits(g["attn"].cpu()), _bits(w["attn"])), i
        assert g["attn"].is_cuda and not g["attn_top"].is_cuda
    assert int(got[3]["attn_top"].max(2)[0].max(1)[0].sub(lens_d).max()) < 0 and int(got[4]["attn_top"].max(2)[0].max(1)[0].sub(lens_e).max()) < 0
    assert int(got[4]["attn_top"].max()) >= 36                                     # (not vacuous: the wide batch does name columns past the first bucket)
    plain = list(model.decode_many([items[0].pin_memory()], batches_per_launch=4, in_flight=2))
    assert "attn_top" not in plain[0] and "attn" not in plain[0] and torch.equal(plain[0]["seq"], want[0]["seq"])
    # eval_split
    kw = {"batch_size": 4, "batches_per_launch": 4, "in_flight": 2, "verbose_loss": 0, "attn_topk": 2}
    _, preds, _ = eval_utils.eval_split(model, att, None, kw)
    assert len(preds) == 8 and all(len(p["regions"]) == len(p["seq"]) and all(1 <= len(wd) <= 2 for wd in p["regions"]) for p in preds)
    assert any(p["seq"] for p in preds)
    top8 = torch.cat([want[0]["attn_top"], want[1]["attn_top"]])
    assert [[wd[0][0] for wd in p["regions"]] for p in preds] == [[int(top8[b, t, 0]) for t in range(len(p["seq"]))] for b, p in enumerate(preds)]
    with pytest.raises(ValueError, match="NAIC"):
        eval_utils.eval_split(model, att, None, dict(kw, inference_mode="SAIC"))
    # mode='sample'
    fc = torch.zeros(4, 0, device="cuda")
    out = model(fc, att[:4].cuda(), None, opt={"train_mode": "NAIC", "attn_topk": 3, "attn_maps": True}, mode="sample")
    assert len(out) == 6 and set(model.last_attn) == {"attn", "attn_top", "attn_top_w"}
    assert torch.equal(out[0].cpu(), want[0]["seq"]) and torch.equal(model.last_attn["attn_top"].cpu(), want[0]["attn_top"])
    assert torch.equal(_bits(model.last_attn["attn"].cpu()), _bits(want[0]["attn"]))
    out2 = model(fc, att[:4].cuda(), None, opt={"train_mode": "NAIC", "attn_topk": 3, "sample_n": 2}, mode="sample")
    assert out2[0].size(0) == 8 and set(model.last_attn) == {"attn_top", "attn_top_w"}
    assert torch.equal(model.last_attn["attn_top"].cpu(), want[0]["attn_top"].repeat_interleave(2, dim=0))
    model(fc, att[:4].cuda(), None, opt={"train_mode": "NAIC"}, mode="sample")
    assert model.last_attn is None                               # (a plain call clears it)
    with pytest.raises(hip.BofiHipError, match="NAIC"):
        model(fc, att[:4].cuda(), None, opt={"train_mode": "SAIC", "attn_topk": 3}, mode="sample")
