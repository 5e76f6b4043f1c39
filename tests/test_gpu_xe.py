"""XE training step on the MI355X: backward kernels against torch autograd of the oracle's formulas, and the
whole forward + criterion + gradients against what the reference itself produced (tests/golden/tiny_train_xe)."""
import numpy as np
import pytest
import torch

import boficap_oracle as O
import counter_streams as cs
from conftest import load_golden

pytestmark = pytest.mark.gpu


def _dev(*ts):
    return [t.cuda() for t in ts]


def _maxdiff(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


# ------------------------------------------------------------------------------------------------ op level
@pytest.mark.parametrize("M,N,K,relu,res", [(50, 96, 64, False, False), (37, 20, 128, False, True), (130, 256, 128, True, False),
                                            (8, 61, 32, False, False)])
def test_linear_backward(M, N, K, relu, res):
    from boficap_amd import xe
    g = torch.Generator().manual_seed(M * 7 + N)
    x, w, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * 0.1, torch.randn(N, generator=g)
    r = torch.randn(M, N, generator=g) if res else None
    dy = torch.randn(M, N, generator=g)
    ref_in = [t.clone().requires_grad_() for t in (x, w, b)] + ([r.clone().requires_grad_()] if res else [])
    y_ref = torch.nn.functional.linear(ref_in[0], ref_in[1], ref_in[2])
    y_ref = torch.relu(y_ref) if relu else y_ref
    y_ref = y_ref + ref_in[3] if res else y_ref
    y_ref.backward(dy)
    dev_in = [t.clone().cuda().requires_grad_() for t in (x, w, b)] + ([r.clone().cuda().requires_grad_()] if res else [])
    y = xe.linear(dev_in[0], dev_in[1], dev_in[2], residual=dev_in[3] if res else None, relu=relu)
    y.backward(dy.cuda())
    assert _maxdiff(y, y_ref) < 2e-4
    for a, b_ in zip(dev_in, ref_in):
        assert _maxdiff(a.grad, b_.grad) < 5e-4 * max(1.0, float(b_.grad.abs().max()))


def test_layernorm_backward():
    from boficap_amd import xe
    g = torch.Generator().manual_seed(3)
    x, gain, bias, dy = torch.randn(45, 128, generator=g) * 2, torch.rand(128, generator=g) + 0.5, torch.randn(128, generator=g), torch.randn(45, 128, generator=g)
    xr, gr, br = [t.clone().requires_grad_() for t in (x, gain, bias)]
    mean, std = xr.mean(-1, keepdim=True), xr.std(-1, keepdim=True)          # TransformerModel.py:1346-1349
    (gr * (xr - mean) / (std + 1e-6) + br).backward(dy)
    xd, gd, bd = [t.clone().cuda().requires_grad_() for t in (x, gain, bias)]
    xe.layer_norm(xd, gd, bd).backward(dy.cuda())
    assert _maxdiff(xd.grad, xr.grad) < 1e-4 and _maxdiff(gd.grad, gr.grad) < 1e-3 and _maxdiff(bd.grad, br.grad) < 1e-3


@pytest.mark.parametrize("mfma", [False, True])
@pytest.mark.parametrize("B,Lq,Lk,kdiv,same", [(4, 20, 20, 1, True), (6, 21, 36, 2, False), (3, 36, 36, 1, True), (4, 7, 22, 1, False),
                                               (2, 64, 64, 1, True), (5, 1, 33, 5, False)])
def test_attention_backward(B, Lq, Lk, kdiv, same, mfma):
    """VALU float32 kernel (parity path) and the bf16 MFMA kernel with transposing LDS reads (bf16 training mode)."""
    from boficap_amd import xe
    xe._COMPUTE["dtype"] = torch.bfloat16 if mfma else torch.float32
    tol = 3e-2 if mfma else 2e-4
    H, d = 2, 128
    g = torch.Generator().manual_seed(B * 100 + Lq)
    klen = torch.randint(1, Lk + 1, (B, Lq), generator=g).int()
    if same:
        buf = torch.randn(B * Lq, 3 * d, generator=g)
        qb, kvb, offs = buf, buf, (0, d, 2 * d)
    else:
        qb, kvb, offs = torch.randn(B * Lq, d, generator=g), torch.randn(B // kdiv * Lk, 2 * d, generator=g), (0, 0, d)
    dout = torch.randn(B * Lq, d, generator=g)

    def ref(qb, kvb):
        q = qb[:, offs[0]:offs[0] + d].reshape(B, Lq, H, 64).transpose(1, 2)
        k = kvb[:, offs[1]:offs[1] + d].reshape(B // kdiv, Lk, H, 64).transpose(1, 2).repeat_interleave(kdiv, 0)
        v = kvb[:, offs[2]:offs[2] + d].reshape(B // kdiv, Lk, H, 64).transpose(1, 2).repeat_interleave(kdiv, 0)
        s = q @ k.transpose(-1, -2) / 8.0
        mask = torch.arange(Lk).view(1, 1, 1, Lk) < klen.view(B, 1, Lq, 1)
        p = torch.softmax(s.masked_fill(~mask, float("-inf")), -1)
        return (p @ v).transpose(1, 2).reshape(B * Lq, d)

    qr = qb.clone().requires_grad_()
    kr = qr if same else kvb.clone().requires_grad_()
    ref(qr, kr).backward(dout)
    qd = qb.clone().cuda().requires_grad_()
    kd = qd if same else kvb.clone().cuda().requires_grad_()
    try:
        out = xe.attention(qd, kd, offs[0], offs[1], offs[2], B, H, Lq, Lk, kdiv, klen.cuda().contiguous(), Lq, 1, 0)
        assert _maxdiff(out, ref(qb, kvb)) < 1e-4
        out.backward(dout.cuda())
    finally:
        xe._COMPUTE["dtype"] = torch.float32
    assert _maxdiff(qd.grad, qr.grad) < tol * max(1.0, float(qr.grad.abs().max()))
    if not same:
        assert _maxdiff(kd.grad, kr.grad) < tol * max(1.0, float(kr.grad.abs().max()))


def test_attention_probability_dropout_bf16():
    """dropout(p_attn) inside the bf16 attention forward and the MFMA backward: against a float64 reference that
    applies the SAME keep mask (recovered from a run with V = identity-like probes), and rate / scaling checks."""
    from boficap_amd import xe
    B, H, L, d, p, seed = 3, 2, 20, 128, 0.3, 4242
    g = torch.Generator().manual_seed(9)
    qkv = torch.randn(B * L, 3 * d, generator=g)
    klen = torch.randint(4, L + 1, (B, L), generator=g).int()
    dout = torch.randn(B * L, d, generator=g)
    bf = lambda t: t.to(torch.bfloat16).float()
    xe._COMPUTE["dtype"] = torch.bfloat16
    xe._STEP_CACHE.clear(); xe._SHADOW_ONLY.clear()
    try:
        def run(qkv_t, drop):
            x = qkv_t.clone().cuda().requires_grad_()
            xe._register_shadow(x, x.detach().to(torch.bfloat16))
            out = xe.attention(x, x, 0, d, 2 * d, B, H, L, L, 1, klen.cuda().contiguous(), L, 1, 0, drop)
            return x, out, xe._shadow(out).float().cpu()
        # recover the mask: with v = one-hot(key) per head dim the context row IS the dropped probability row
        probe = qkv.clone()
        probe[:, 2 * d:] = 0
        for b in range(B):
            for k in range(L):
                for h in range(H):
                    probe[b * L + k, 2 * d + h * 64 + k] = 1.0
        _, _, ctx_nodrop = run(probe, None)
        _, _, ctx_drop = run(probe, (p, seed, None))
        P0 = ctx_nodrop.view(B, L, H, 64)[..., :L]             # [b, q, h, k]
        Pd = ctx_drop.view(B, L, H, 64)[..., :L]
        valid = (torch.arange(L).view(1, 1, 1, L) < klen.view(B, L, 1, 1)) & (P0 > 1e-3)
        keep = Pd > 0
        rate = float(keep[valid].float().mean())
        assert abs(rate - (1 - p)) < 0.05, rate
        assert torch.allclose(Pd[valid & keep], P0[valid & keep] / (1 - p), rtol=3e-2, atol=2e-3)
        # the recovered mask is the documented one: element ((b * H + h) * Lq + q) * Lk + k of stream `seed` (tests/counter_streams.py)
        kept = torch.from_numpy(cs.keep_mask(seed, 0, p, cs.attn_ids_padded(B, H, L, L))).permute(0, 2, 1, 3)      # [b, q, h, k]
        assert int(valid.sum()) > B * H * L and torch.equal(keep[valid], kept[valid])
        mask = torch.where(keep, torch.tensor(1 / (1 - p)), torch.tensor(0.0)).permute(0, 2, 1, 3)      # [b, h, q, k]
        # full forward / backward with that mask in float64-ish torch
        xr = bf(qkv).clone().requires_grad_()
        q = xr[:, :d].reshape(B, L, H, 64).transpose(1, 2)
        k = xr[:, d:2 * d].reshape(B, L, H, 64).transpose(1, 2)
        v = xr[:, 2 * d:].reshape(B, L, H, 64).transpose(1, 2)
        s_ = q @ k.transpose(-1, -2) / 8.0
        km = torch.arange(L).view(1, 1, 1, L) < klen.view(B, 1, L, 1)
        pr = torch.softmax(s_.masked_fill(~km, float("-inf")), -1) * mask
        ref = (pr @ v).transpose(1, 2).reshape(B * L, d)
        ref.backward(dout)
        x, out, ctx = run(qkv, (p, seed, None))
        assert _maxdiff(ctx, ref) < 3e-2
        out.backward(dout.cuda())
        assert _maxdiff(x.grad, xr.grad) < 3e-2 * max(1.0, float(xr.grad.abs().max()))
    finally:
        xe._COMPUTE["dtype"] = torch.float32
        xe._STEP_CACHE.clear(); xe._SHADOW_ONLY.clear()


def test_logsoftmax_embed_dropout_backward():
    from boficap_amd import xe
    g = torch.Generator().manual_seed(11)
    x, dy = torch.randn(33, 61, generator=g) * 3, torch.randn(33, 61, generator=g)
    xr = x.clone().requires_grad_()
    torch.log_softmax(xr, -1).backward(dy)
    xd = x.clone().cuda().requires_grad_()
    y = xe.log_softmax(xd * 1.0)                               # in place on a fresh (non-leaf) tensor
    y.backward(dy.cuda())
    assert _maxdiff(y, torch.log_softmax(x, -1)) < 1e-5 and _maxdiff(xd.grad, xr.grad) < 1e-5
    # embedding: tok + syn + pe, gradients scattered back into both tables
    d, L = 128, 5
    lut_t, lut_s, pe = torch.randn(30, d, generator=g), torch.randn(10, d, generator=g), torch.randn(50, d, generator=g)
    tok, syn = torch.randint(0, 30, (3 * L,), generator=g), torch.randint(0, 10, (3 * L,), generator=g)
    de = torch.randn(3 * L, d, generator=g)
    tr, sr = lut_t.clone().requires_grad_(), lut_s.clone().requires_grad_()
    ((tr[tok] * d ** 0.5 + sr[syn] * d ** 0.5) + pe[:L].repeat(3, 1)).backward(de)
    td, sd_ = lut_t.clone().cuda().requires_grad_(), lut_s.clone().cuda().requires_grad_()
    e = xe.embed(td, sd_, pe.cuda(), tok.cuda(), syn.cuda(), L)
    e.backward(de.cuda())
    assert _maxdiff(e, (lut_t[tok] * d ** 0.5 + lut_s[syn] * d ** 0.5) + pe[:L].repeat(3, 1)) < 1e-5
    assert _maxdiff(td.grad, tr.grad) < 1e-3 and _maxdiff(sd_.grad, sr.grad) < 1e-3
    # dropout: keep rate, scaling, and the backward uses the forward's mask
    xd = torch.ones(400, 256, device="cuda", requires_grad=True)
    y = xe.DropoutFn.apply(xd, None, 0.1, 12345, None)
    keep = (y != 0).float()
    assert abs(float(keep.mean()) - 0.9) < 0.01 and torch.allclose(y[y != 0], torch.tensor(1 / 0.9, device="cuda"))
    y.backward(torch.ones_like(y))
    assert torch.equal(xd.grad != 0, y != 0)
    y2 = xe.DropoutFn.apply(xd, None, 0.1, 12346, None)
    assert not torch.equal(y2 != 0, y != 0)
    # ... and the mask is the documented one: element i of stream seed (+ the step word on the device) is kept iff
    # drop_hash(seed + step, i) >= p * 2^32 (tests/counter_streams.py), seeds above 2^63 included
    idx = np.arange(400 * 256, dtype=np.uint64)
    assert np.array_equal((y != 0).cpu().numpy().ravel(), cs.keep_mask(12345, 0, 0.1, idx))
    step = torch.tensor([5], dtype=torch.int64, device="cuda")
    y5 = xe.DropoutFn.apply(xd, None, 0.1, 12345, step)
    assert np.array_equal((y5 != 0).cpu().numpy().ravel(), cs.keep_mask(12345, 5, 0.1, idx))
    assert not np.array_equal(cs.keep_mask(12345, 5, 0.1, idx), cs.keep_mask(12345, 0, 0.1, idx))
    yb = xe.DropoutFn.apply(xd, None, 0.1, 2 ** 63 + 1, None)
    assert np.array_equal((yb != 0).cpu().numpy().ravel(), cs.keep_mask(2 ** 63 + 1, 0, 0.1, idx))
    assert not np.array_equal(cs.keep_mask(2 ** 63 + 1, 0, 0.1, idx), cs.keep_mask(1, 0, 0.1, idx))       # (a seed cut to 32 bits would show)


# ------------------------------------------------------------------------------------------------ whole step
def _model(weight_cache, manifest, case):
    import captioning.models as models
    m = manifest[case]
    cfg, sd = weight_cache(m["config"], m["seed"], m["gen_scale"], m["digest"], m.get("patch"))
    model = models.setup(cfg.to_opt())
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return cfg, model.cuda()


def test_xe_step_vs_reference(weight_cache, manifest):
    """model(..., mode='forward') -> criterion -> backward against the reference's own outputs, loss and gradients."""
    from boficap_amd import xe
    cfg, model = _model(weight_cache, manifest, "tiny_train_xe")
    model.eval()                                               # the fixture was recorded with dropout off
    g = load_golden("tiny_train_xe")
    t = lambda k: torch.from_numpy(g[k]).cuda()
    fc = torch.zeros(g["att_feats"].shape[0], 0, device="cuda")
    outs = model(fc, t("att_feats"), t("labels"), None, t("phrase_num"), t("phrase_length"), t("phrase_syn"),
                 t("extend_phrase_syn_seq"), t("extend_phrase_seq"), t("extend_phrase_seq_mask"), -1.0)
    for i, o in enumerate(outs):
        assert o.shape == g[f"out{i}"].shape
        assert _maxdiff(o, torch.from_numpy(g[f"out{i}"])) < 1e-4, f"output {i}"
    loss, parts = xe.criterion_uic(outs, t("phrase_num"), t("phrase_length"), t("phrase_syn"), t("labels"))
    assert abs(float(loss.detach()) - float(g["losses"][0])) < 1e-3
    assert np.allclose([float(p.detach()) for p in parts], g["losses"][1:], atol=1e-4)
    loss.backward()
    names = [str(n) for n in g["grad_names"]]
    params = dict(model.named_parameters())
    worst = 0.0
    for n, ref_norm in zip(names, g["grad_norms"]):
        p = params[n]
        if ref_norm < 0:                                        # the reference leaves this parameter without a gradient
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, n
            continue
        assert p.grad is not None, n
        got = float(p.grad.double().norm())
        worst = max(worst, abs(got - ref_norm) / max(ref_norm, 1e-6))
        assert abs(got - ref_norm) <= 2e-3 * max(ref_norm, 1e-3), (n, got, float(ref_norm))
        if "grad." + n in g:
            ref_g = torch.from_numpy(g["grad." + n])
            assert _maxdiff(p.grad, ref_g) <= 2e-3 * max(1e-3, float(ref_g.abs().max())), n
    print("worst relative grad-norm error", worst)


def test_xe_step_oracle_ragged_regions(weight_cache, manifest):
    """Ragged att_masks + seq_per_img 2 against autograd over the oracle on the CPU (same weights, same batch)."""
    from boficap_amd import xe
    from boficap_amd.weights import synthetic_att_feats
    from training_batch import make_training_batch
    cfg, model = _model(weight_cache, manifest, "tiny_train_xe")
    model.eval()
    n_img, spi = 4, 2
    att = torch.from_numpy(synthetic_att_feats(n_img, 36, cfg.att_feat_size, seed=77))
    masks = torch.zeros(n_img, 36)
    for i, n in enumerate((36, 20, 9, 31)):
        masks[i, :n] = 1
    b = {k: torch.from_numpy(v) for k, v in make_training_batch(cfg, n_img, spi, seed=5).items()}
    w = {k: v.detach().cpu().clone().requires_grad_(v.dtype.is_floating_point and k != "model.pos_embed.pe") for k, v in model.state_dict().items()}
    outs_ref = O.forward_uic(w, cfg, att, b["labels"], masks, b["phrase_num"], b["phrase_length"], b["phrase_syn"],
                             b["extend_phrase_syn_seq"], b["extend_phrase_seq"], b["extend_phrase_seq_mask"])
    loss_ref, _ = O.criterion_uic(outs_ref, b["phrase_num"], b["phrase_length"], b["phrase_syn"], b["labels"])
    loss_ref.backward()
    fc = torch.zeros(n_img, 0, device="cuda")
    outs = model(fc, att.cuda(), b["labels"].cuda(), masks.cuda(), b["phrase_num"], b["phrase_length"], b["phrase_syn"],
                 b["extend_phrase_syn_seq"], b["extend_phrase_seq"], b["extend_phrase_seq_mask"], -1.0)
    for i, (o, r) in enumerate(zip(outs, outs_ref)):
        assert _maxdiff(o, r) < 1e-4, f"output {i}"
    loss, _ = xe.criterion_uic(outs, b["phrase_num"], b["phrase_length"], b["phrase_syn"], b["labels"])
    assert abs(float(loss.detach()) - float(loss_ref.detach())) < 1e-3
    loss.backward()
    for n, p in model.named_parameters():
        r = w[n].grad
        if r is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, n
            continue
        assert _maxdiff(p.grad, r) <= 2e-3 * max(1e-3, float(r.abs().max())), n


def test_xe_training_mode_runs_and_glat(weight_cache, manifest):
    """Dropout on: finite loss, gradients everywhere the reference has them; glat_p = 0 reveals nothing (same as -1)."""
    from boficap_amd import xe
    cfg, model = _model(weight_cache, manifest, "tiny_train_xe")
    g = load_golden("tiny_train_xe")
    t = lambda k: torch.from_numpy(g[k]).cuda()
    fc = torch.zeros(g["att_feats"].shape[0], 0, device="cuda")
    args = (fc, t("att_feats"), t("labels"), None, t("phrase_num"), t("phrase_length"), t("phrase_syn"),
            t("extend_phrase_syn_seq"), t("extend_phrase_seq"), t("extend_phrase_seq_mask"))
    model.train()
    outs = model(*args, -1.0)
    loss, _ = xe.criterion_uic(outs, t("phrase_num"), t("phrase_length"), t("phrase_syn"), t("labels"))
    loss.backward()
    assert torch.isfinite(loss)
    assert abs(float(loss.detach()) - float(g["losses"][0])) > 1e-4                         # dropout really changed the pass
    assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)
    model.eval()
    with torch.no_grad():
        a, b = model(*args, -1.0), model(*args, 0.0)
        c = model(*args, 1.0)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert all(torch.equal(x, y) for x, y in zip(a[:5], c[:5])) and not torch.equal(a[5], c[5])


# ------------------------------------------------------------------------------------------------ optimiser / trainer
def test_adam_kernel_matches_torch_adam():
    """bofi_adam_step (clip by value + Adam, flat bucket) against clip_grad_value_ + torch.optim.Adam on the CPU."""
    from boficap_amd import hip
    n = 4096 + 8
    g0 = torch.Generator().manual_seed(5)
    p_ref = torch.randn(n, generator=g0).requires_grad_()
    opt = torch.optim.Adam([p_ref], lr=0.0, betas=(0.9, 0.98), eps=1e-9)
    p, m, v = p_ref.detach().clone().cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    shadow = torch.empty(n, dtype=torch.bfloat16, device="cuda")
    for step in range(1, 6):
        grad = torch.randn(n, generator=g0) * (0.3 if step % 2 else 0.01)
        lr = 1e-3 * step
        p_ref.grad = (grad * 0.5).clone()
        torch.nn.utils.clip_grad_value_([p_ref], 0.1)
        for grp in opt.param_groups:
            grp["lr"] = lr
        opt.step()
        hip.check(hip.lib().bofi_adam_step(hip.ptr(p), hip.ptr(grad.cuda()), hip.ptr(m), hip.ptr(v), hip.ptr(shadow), n, lr, 0.9, 0.98, 1e-9,
                                           step, 0.1, 0.5, hip.stream_ptr()))
        assert _maxdiff(p, p_ref) < 2e-6
    assert _maxdiff(shadow.float(), p) < 1e-2 * float(p.abs().max())


def test_trainer_steps_reduce_loss_and_refresh_engine(weight_cache, manifest):
    """A few XE steps on one synthetic batch: the loss falls, parameters stay views of the flat bucket, the first
    step equals clip+Adam applied to the reference-checked gradients, and decode afterwards sees the new weights."""
    from boficap_amd.collate import synthetic_training_batch
    from boficap_amd.trainer import XETrainer
    from boficap_amd.weights import synthetic_att_feats
    cfg, model = _model(weight_cache, manifest, "tiny_train_xe")
    model.eval()                                               # deterministic steps (dropout off)
    opt = cfg.to_opt()
    opt.noamopt, opt.learning_rate, opt.grad_clip_value = False, 2e-3, 0.1
    tr = XETrainer(model, opt)
    n_img, spi = 4, 5
    batch = {k: torch.from_numpy(v).cuda() for k, v in synthetic_training_batch(cfg, n_img, spi, seed=2).items()}
    batch["att_feats"] = torch.from_numpy(synthetic_att_feats(n_img, 36, cfg.att_feat_size, seed=8)).cuda()
    fc = torch.zeros(n_img, 0, device="cuda")
    with torch.no_grad():
        seq0 = model(fc, batch["att_feats"], None, opt={"train_mode": "NAIC"}, mode="sample")[0].clone()
    w0 = tr.bucket.flat.clone()
    loss0, _ = tr.forward_backward(batch)
    g = tr.bucket.grad.clone()
    tr.optimizer_step(1.0)
    # first Adam step: m / bc1 = g and sqrt(v / bc2) = |g|  ->  update = lr * g / (|g| + eps)
    gc = g.clamp(-0.1, 0.1)
    expect = w0 - 2e-3 * gc / (gc.abs() + 1e-8)
    assert _maxdiff(tr.bucket.flat, expect) < 1e-6
    losses = [float(loss0)]
    for _ in range(7):
        losses.append(float(tr.step(batch)[0]))
    assert losses[-1] < 0.8 * losses[0], losses
    assert all(p.data_ptr() == tr.bucket.flat.data_ptr() + o * 4 for p, o in zip(tr.bucket.params, tr.bucket.offsets))
    with torch.no_grad():
        seq1 = model(fc, batch["att_feats"], None, opt={"train_mode": "NAIC"}, mode="sample")[0]
    ref = O.sample_naic(O.as_torch({k: v.detach().cpu() for k, v in model.state_dict().items()}), cfg, batch["att_feats"].cpu())[0]
    assert torch.equal(seq1.cpu(), ref)                        # the engine repacked the trained weights
    assert not torch.equal(seq1, seq0) or losses[-1] < losses[0]
    sd = tr.state_dict()
    assert sd["_step"] == 8 and sorted(sd["state"]) == [i for i, (n, _) in enumerate(model.named_parameters()) if not n.startswith(tr.bucket.DEAD_PREFIXES)]
    p0 = next(model.parameters())
    assert sd["state"][0]["exp_avg"].shape == p0.shape and float(sd["state"][0]["step"]) == 8.0


def test_xe_step_bf16_operands_close_to_reference(weight_cache, manifest):
    """bf16 GEMM operands with fp32 accumulation / outputs / master weights: the same step within bf16 tolerances
    (log-probs 2e-2 as north_star states for bf16 logits; gradient norms 5 %)."""
    from boficap_amd import xe
    cfg, model = _model(weight_cache, manifest, "tiny_train_xe")
    model.eval()
    model.train_dtype = torch.bfloat16
    g = load_golden("tiny_train_xe")
    t = lambda k: torch.from_numpy(g[k]).cuda()
    fc = torch.zeros(g["att_feats"].shape[0], 0, device="cuda")
    outs = model(fc, t("att_feats"), t("labels"), None, t("phrase_num"), t("phrase_length"), t("phrase_syn"),
                 t("extend_phrase_syn_seq"), t("extend_phrase_seq"), t("extend_phrase_seq_mask"), -1.0)
    errs = [_maxdiff(o, torch.from_numpy(g[f"out{i}"])) for i, o in enumerate(outs)]
    perr = [_maxdiff(o.exp(), torch.from_numpy(g[f"out{i}"]).exp()) for i, o in enumerate(outs)]
    print("bf16 log-prob errors per output", errs, "probability errors", perr)
    # token log-probs: the TINY model's logits have std 1.37 vs 0.33 at full size, hence 6e-2 for north_star's 2e-2 (as in
    # test_bf16_within_tolerance); the calibrated bound heads have logits of +-15, so they are compared as probabilities
    worst_out = max(errs[2], errs[5])
    assert max(perr) < 2e-2
    loss, _ = xe.criterion_uic(outs, t("phrase_num"), t("phrase_length"), t("phrase_syn"), t("labels"))
    loss.backward()
    assert abs(float(loss.detach()) - float(g["losses"][0])) < 1e-2 * float(g["losses"][0])
    params = dict(model.named_parameters())
    worst = 0.0
    for n, ref_norm in zip([str(n) for n in g["grad_names"]], g["grad_norms"]):
        if ref_norm < 1e-3:
            continue
        worst = max(worst, abs(float(params[n].grad.double().norm()) - ref_norm) / ref_norm)
    print("bf16: worst log-prob error", worst_out, "worst relative grad-norm error", worst)
    assert worst_out < 6e-2 and worst < 5e-2


@pytest.mark.parametrize("masks", [False, True])
def test_bucket_accumulated_gradients_equal_autograd_gradients(weight_cache, manifest, masks):
    """With a flat bucket the kernels accumulate parameter gradients straight into the bucket (packed q|k|v views, GEMM
    epilogue accumulation, atomics); without one autograd carries them.  Both must give the same gradients."""
    from boficap_amd import xe
    from boficap_amd.collate import synthetic_training_batch
    from boficap_amd.trainer import XETrainer
    from boficap_amd.weights import synthetic_att_feats
    cfg, plain = _model(weight_cache, manifest, "tiny_train_xe")
    _, bucketed = _model(weight_cache, manifest, "tiny_train_xe")
    plain.eval(); bucketed.eval()
    n_img, spi = 3, 5
    batch = {k: torch.from_numpy(v).cuda() for k, v in synthetic_training_batch(cfg, n_img, spi, seed=4).items()}
    batch["att_feats"] = torch.from_numpy(synthetic_att_feats(n_img, 36, cfg.att_feat_size, seed=6)).cuda()
    if masks:
        m = torch.zeros(n_img, 36, device="cuda")
        for i, n in enumerate((30, 36, 12)):
            m[i, :n] = 1
        batch["att_masks"] = m
    fc = torch.zeros(n_img, 0, device="cuda")
    outs = plain(fc, batch["att_feats"], batch["labels"], batch.get("att_masks"), batch["phrase_num"], batch["phrase_length"], batch["phrase_syn"],
                 batch["extend_phrase_syn_seq"], batch["extend_phrase_seq"], batch["extend_phrase_seq_mask"], -1.0)
    loss, _ = xe.criterion_uic(outs, batch["phrase_num"], batch["phrase_length"], batch["phrase_syn"], batch["labels"])
    loss.backward()
    tr = XETrainer(bucketed)
    assert tr.bucket.span([dict(bucketed.named_parameters())[f"model.encoder.layers.0.self_attn.linears.{i}.weight"] for i in range(3)]) is not None
    loss_b, _ = tr.forward_backward(batch)
    assert abs(float(loss_b) - float(loss.detach())) < 1e-5
    ref = dict(plain.named_parameters())
    for n, p in bucketed.named_parameters():
        r = ref[n].grad
        if r is None:
            assert float(p.grad.abs().max()) == 0.0, n
        else:
            assert _maxdiff(p.grad, r) <= 1e-4 * max(1e-3, float(r.abs().max())), n
    tr.forward_backward(batch)                                 # a second pass starts from zeroed buckets
    assert _maxdiff(dict(bucketed.named_parameters())["model.generator.proj.weight"].grad, ref["model.generator.proj.weight"].grad) < 1e-4


@pytest.mark.parametrize("M,NI,NJ", [(96, 64, 64), (6400, 512, 512), (1000, 200, 72), (37, 24, 136), (2304, 2048, 512)])
def test_gemm_tn_accumulates_a_transposed_times_b(M, NI, NJ):
    """bofi_gemm_tn_acc (transposing LDS reads, split over rows, atomics into C) against A^T B in float64."""
    from boficap_amd import hip
    g = torch.Generator().manual_seed(M + NI)
    pad8 = lambda n: (n + 63) // 64 * 64
    a = torch.zeros(M, pad8(NI)); a[:, :NI] = torch.randn(M, NI, generator=g)
    b = torch.zeros(M, pad8(NJ)); b[:, :NJ] = torch.randn(M, NJ, generator=g)
    ab, bb = a.cuda().to(torch.bfloat16), b.cuda().to(torch.bfloat16)
    base = torch.randn(NI, NJ, generator=g)
    c = base.clone().cuda()
    cs = torch.full((NI,), 0.5, device="cuda")
    hip.check(hip.lib().bofi_gemm_tn_acc(hip.ptr(ab), ab.shape[1], ab.shape[1], hip.ptr(bb), bb.shape[1], bb.shape[1], hip.ptr(c), NJ, M, NI, NJ,
                                         hip.ptr(cs), hip.stream_ptr()))
    ref = base.double() + ab.float().cpu().double()[:, :NI].t() @ bb.float().cpu().double()[:, :NJ]
    assert _maxdiff(c, ref) < 2e-3 * max(1.0, float(ref.abs().max()))
    cs_ref = 0.5 + ab.float().cpu().double()[:, :NI].sum(0)               # column sums of A ride along (the bias gradient)
    assert _maxdiff(cs, cs_ref) < 1e-3 * max(1.0, float(cs_ref.abs().max()))
    with pytest.raises(hip.BofiHipError):
        hip.check(hip.lib().bofi_gemm_tn_acc(hip.ptr(ab), ab.shape[1], 7, hip.ptr(bb), bb.shape[1], bb.shape[1], hip.ptr(c), NJ, M, NI, NJ,
                                             None, hip.stream_ptr()))


@pytest.mark.parametrize("dense_too", [False, True])
def test_log_softmax_pick_against_torch(dense_too):
    """log_softmax + gather fused (bofi_nll_bwd when only the picked values carry a gradient; dense fallback otherwise)."""
    from boficap_amd import xe
    T, V = 70, 1234
    g = torch.Generator().manual_seed(8)
    logits, labels, gp = torch.randn(T, V, generator=g) * 3, torch.randint(0, V, (T,), generator=g), torch.randn(T, generator=g)
    gp[::7] = 0.0                                                       # zero-weight rows (padding rows of the row list)
    gd = torch.randn(T, V, generator=g) * 0.1
    ref_in = logits.clone().requires_grad_()
    lp = torch.log_softmax(ref_in, 1)
    loss = (lp.gather(1, labels[:, None]).squeeze(1) * gp).sum() + ((lp * gd).sum() if dense_too else 0.0)
    loss.backward()
    x = logits.clone().cuda().requires_grad_()
    y, picked = xe.log_softmax_pick(x * 1.0, labels.cuda())
    assert _maxdiff(y.detach(), lp.detach()) < 1e-5 and _maxdiff(picked.detach(), lp.detach().gather(1, labels[:, None]).squeeze(1)) < 1e-5
    ((picked * gp.cuda()).sum() + ((y * gd.cuda()).sum() if dense_too else 0.0)).backward()
    assert _maxdiff(x.grad, ref_in.grad) < 1e-5 * max(1.0, float(ref_in.grad.abs().max()))


def test_layernorm_backward_hands_the_masked_gradient_to_its_producer():
    """x = r + dropout(x0 W^T + b) in the GEMM epilogue, n = LayerNorm(x): the LayerNorm backward also writes the linear's
    dz = mask o dL/dx in bf16 (bofi_layernorm_bwd_ex), which must be the dz the mask-and-cast pass would have made --
    same weight, bias and input gradients with and without the hand-over."""
    from boficap_amd import xe
    M, d, K = 200, 512, 128
    g = torch.Generator().manual_seed(12)
    x0, w, b = torch.randn(M, K, generator=g), torch.randn(d, K, generator=g) * 0.1, torch.randn(d, generator=g)
    r, gain, beta, gout = torch.randn(M, d, generator=g), torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g), torch.randn(M, d, generator=g)
    grads = []
    for hand_over in (True, False):
        xe._COMPUTE["dtype"] = torch.bfloat16
        xe._STEP_CACHE.clear(); xe._SHADOW_ONLY.clear()
        t = [v.clone().cuda().requires_grad_() for v in (x0, w, b, r, gain, beta)]
        x = xe.linear(t[0], t[1], t[2], residual=t[3], drop=(0.3, 4711, None))
        if not hand_over:
            for k in [k for k in xe._STEP_CACHE if k[0] == "prod"]:
                del xe._STEP_CACHE[k]
        xr, n = xe.layer_norm_res(x, t[4], t[5])
        ((n * gout.cuda()).sum() + (xr * 0.5).sum()).backward()
        assert any(k[0] == "gop" for k in xe._STEP_CACHE) == hand_over
        grads.append([v.grad.clone() for v in t])
    for a, c in zip(*grads):
        assert _maxdiff(a, c) <= 1e-5 * max(1.0, float(c.abs().max()))


@pytest.mark.parametrize("p_drop", [0.0, 0.25])
def test_ffn_input_gradient_arrives_masked_from_the_second_linear(p_drop):
    """h = dropout(relu(x W1^T + b1)) in the GEMM epilogue, y = h W2^T + b2: the input-gradient GEMM of the second linear masks by
    h > 0 and scales by 1 / (1 - p) in its epilogue and hands the first linear its dz in bf16 (bofi_linear_masked) -- same
    gradients as the float32 dL/dh + mask-and-cast pass."""
    from boficap_amd import xe
    M, d, dff = 300, 128, 256
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(M, d, generator=g)
    w1, b1 = torch.randn(dff, d, generator=g) * 0.1, torch.randn(dff, generator=g) * 0.1
    w2, b2, gout = torch.randn(d, dff, generator=g) * 0.1, torch.randn(d, generator=g), torch.randn(M, d, generator=g)
    grads = []
    for hand_over in (True, False):
        xe._COMPUTE["dtype"] = torch.bfloat16
        xe._STEP_CACHE.clear(); xe._SHADOW_ONLY.clear()
        t = [v.clone().cuda().requires_grad_() for v in (x0, w1, b1, w2, b2)]
        h = xe.linear(t[0], t[1], t[2], relu=True, drop=(p_drop, 99, None) if p_drop else None, shadow=True, masked_grad=hand_over)
        y = xe.linear(h, t[3], t[4])
        (y * gout.cuda()).sum().backward()
        assert any(k[0] == "gopr" for k in xe._STEP_CACHE) == hand_over
        grads.append([v.grad.clone() for v in t])
    for a, c in zip(*grads):
        assert _maxdiff(a, c) <= 1e-5 * max(1.0, float(c.abs().max()))


@pytest.mark.parametrize("n", [3, 45])
def test_grouped_weight_gradient_gemms(n):
    """bofi_gemm_tn_grouped: n problems of mixed sizes (ragged tiles, empty row sets, two problems adding into the same
    target, with and without column sums) = the problems run one by one; 45 spans several launches."""
    from boficap_amd import hip, xe
    g = torch.Generator().manual_seed(n)
    pad = lambda v: (v + 63) // 64 * 64
    shapes = [(300, 70, 130), (0, 64, 64), (129, 20, 64), (1000, 128, 65), (64, 64, 192), (500, 200, 130), (257, 128, 256),    # the last two: 128 x 128 tiles
              (704, 300, 520), (32, 256, 256), (2560, 512, 264), (96, 1000, 256), (1024, 256, 256)]                                # large outputs, M % 32 == 0
    todo, refs, targets = [], [], {}
    for e in range(n):
        M, NI, NJ = shapes[e % len(shapes)]
        a = torch.zeros(max(M, 1), pad(NI)); a[:M, :NI] = torch.randn(M, NI, generator=g)
        b = torch.zeros(max(M, 1), pad(NJ)); b[:M, :NJ] = torch.randn(M, NJ, generator=g)
        ab, bb = a.cuda().bfloat16(), b.cuda().bfloat16()
        key = (NI, NJ, e % 2 if e >= len(shapes) else e + 100)               # later problems share targets pairwise
        if key not in targets:
            targets[key] = (torch.zeros(NI, NJ, device="cuda"), torch.zeros(NI, device="cuda"), torch.zeros(NI, NJ, dtype=torch.float64),
                            torch.zeros(NI, dtype=torch.float64))
        c, cs, rc, rcs = targets[key]
        with_cs = e % 3 != 1
        todo.append((ab, ab.shape[1], bb, bb.shape[1], c, NJ, M, NI, NJ, cs if with_cs else None))
        rc += ab[:M, :NI].float().cpu().double().t() @ bb[:M, :NJ].float().cpu().double()
        if with_cs:
            rcs += ab[:M, :NI].float().cpu().double().sum(0)
    with xe.step_state(defer=True):
        xe._DEFER["list"].extend(todo)
        assert xe.flush_weight_grads() == n and xe._DEFER["list"] == []
    for c, cs, rc, rcs in targets.values():
        assert _maxdiff(c, rc) < 2e-3 * max(1.0, float(rc.abs().max()))
        assert _maxdiff(cs, rcs) < 2e-3 * max(1.0, float(rcs.abs().max()))


@pytest.mark.parametrize("relu,res", [(False, True), (True, False)])
def test_linear_with_epilogue_dropout_bf16(relu, res):
    """Dropout made in the GEMM epilogue (forward) and in the dz cast (backward) = the separate dropout kernel's mask = the documented
    one at element m * N + n (tests/counter_streams.py)."""
    _linear_with_epilogue_dropout(70, 128, 64, relu, res)


# Which epilogue of gemm_glds.hip a shape reaches is decided by vec_ok (launch_linear_glds): N a multiple of 4 and aligned rows take the
# vectorised one (four consecutive ids per lane), anything else the one-float-per-lane one.  (70, 128, 64) above, (64, 512, 64) and
# (37, 20, 128) -- 64-row tiles of 32 / 16 columns, M <= 64 -- all have N % 4 == 0: the vectorised epilogue.  (37, 61, 128) and (70, 61, 64)
# have N % 4 != 0: the general epilogue (on the 64 x 32 and the 64 x 64 tile), and the dz cast pads their rows to 64 columns.
@pytest.mark.parametrize("relu,res", [(False, True), (True, False)])
@pytest.mark.parametrize("M,N,K", [(64, 512, 64), (37, 20, 128), (37, 61, 128), (70, 61, 64)])
def test_linear_epilogue_dropout_mask_on_both_epilogues(M, N, K, relu, res):
    _linear_with_epilogue_dropout(M, N, K, relu, res)


def _linear_with_epilogue_dropout(M, N, K, relu, res):
    from boficap_amd import xe
    p, seed = 0.25, 987654321
    g = torch.Generator().manual_seed(1)
    x, w, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * 0.2, torch.randn(N, generator=g)
    r = torch.randn(M, N, generator=g) if res else None
    dy = torch.randn(M, N, generator=g)
    mask = xe.DropoutFn.apply(torch.ones(M, N, device="cuda"), None, p, seed, None).cpu()        # keep / (1 - p)
    assert 0.6 < float((mask > 0).float().mean()) < 0.9
    bf = lambda t: t.to(torch.bfloat16).float()
    xr, wr, br = bf(x).requires_grad_(), bf(w).requires_grad_(), b.clone().requires_grad_()
    z = torch.nn.functional.linear(xr, wr, br)
    z = torch.relu(z) if relu else z
    y_ref = z * mask + (r if res else 0)
    y_ref.backward(dy)
    xe._COMPUTE["dtype"] = torch.bfloat16
    xe._STEP_CACHE.clear()
    try:
        xd, wd, bd = x.clone().cuda().requires_grad_(), w.clone().cuda().requires_grad_(), b.clone().cuda().requires_grad_()
        y = xe.linear(xd, wd, bd, residual=r.cuda() if res else None, relu=relu, drop=(p, seed, None))
        y.backward(dy.cuda())
    finally:
        xe._COMPUTE["dtype"] = torch.float32
        xe._STEP_CACHE.clear()
    assert _maxdiff(y, y_ref) < 2e-3
    assert torch.equal((y.cpu() - (r if res else 0)) == 0, (mask == 0) | (z.detach() * mask == 0))
    kept = torch.from_numpy(cs.keep_mask(seed, 0, p, cs.linear_ids(M, N)))
    assert torch.equal(mask > 0, kept)
    assert torch.equal((y.detach().cpu() - (r if res else 0)) != 0, kept & (z.detach() != 0))            # the GEMM's own output, not through the dropout kernel
    rel = lambda a, ref: _maxdiff(a, ref) / float(ref.abs().max())               # dz is rounded to bf16 for the two products
    assert rel(xd.grad, xr.grad) < 1e-2 and rel(wd.grad, wr.grad) < 1e-2 and rel(bd.grad, br.grad) < 1e-2   # the bias gradient sums the bf16 dz


def test_tools_train_entry_point_writes_reference_checkpoints(tmp_path):
    """python tools/train.py (XE phase, synthetic batches): runs, logs a finite loss, writes the reference's checkpoint files --
    model.pth (state_dict schema), optimizer.pth (torch Adam layout + _step), infos / histories pickles; a second run resumes
    from them and switches to the self-critical step."""
    from boficap_amd.config import TINY
    from boficap_amd.weights import schema
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ck = str(tmp_path / "ck")
    cmd = [sys.executable, os.path.join(root, "tools", "train.py"), "--tiny", "--max_iters", "3", "--batch_size", "2", "--seq_per_img", "3",
           "--losses_log_every", "1", "--checkpoint_path", ck, "--glancing_token", "1"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "iter 3" in out.stdout and "nan" not in out.stdout.lower()
    sd = torch.load(os.path.join(ck, "model.pth"))
    assert list(sd.keys()) == list(schema(TINY).keys())
    osd = torch.load(os.path.join(ck, "optimizer.pth"), weights_only=False)
    assert osd["_step"] == 3
    # the reference's optimizer.pth layout: torch's own Adam loads it (captioning/utils/misc.py:199-204 hands it the dict minus '_step')
    import captioning.models as models
    ref_model = models.setup(TINY.to_opt())
    adam = torch.optim.Adam(ref_model.parameters(), lr=0, betas=(0.9, 0.98), eps=1e-9)
    adam.load_state_dict({k: v for k, v in osd.items() if k != "_step"})
    assert len(adam.state) == len(list(ref_model.parameters())) - 12      # the 12 parameters the model never reads carry no state
    from boficap_amd.checkpoint import load_infos
    infos, hist = load_infos(ck, "bofi")
    assert infos["iter"] == 3 and infos["opt"].caption_model == "transformer" and sorted(hist["loss_history"]) == [1, 2, 3]
    # the directory tools/train.py itself wrote goes through the reference's resume lines (tools/train.py:55-69,117-128 restated in
    # tests/test_formats.py): 'loader_state_dict' is indexed and the four model options are read without defaults there
    from test_formats import _reference_resume_lines
    it, ep, loader_state, best, hist2 = _reference_resume_lines(ck, "bofi", infos["opt"])
    assert (it, loader_state) == (3, None) and sorted(hist2["loss_history"]) == [1, 2, 3]
    out = subprocess.run(cmd + ["--start_from", ck, "--dtype", "f32", "--self_critical_after", "5", "--train_sample_n", "2"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "iter 5" in out.stdout and "iter 6" in out.stdout and "struc_loss" in out.stdout
    assert load_infos(ck, "bofi")[0]["iter"] == 6


def test_trainer_graph_replay_matches_eager_steps(weight_cache, manifest):
    """The captured step (hipGraph of zero-grad + forward + criterion + backward) against eager steps: same losses and
    weights with dropout off; with dropout on, replays draw fresh masks (the step word lives on the device)."""
    from boficap_amd.collate import synthetic_training_batch
    from boficap_amd.trainer import XETrainer
    from boficap_amd.weights import synthetic_att_feats
    cfg, eager_model = _model(weight_cache, manifest, "tiny_train_xe")
    _, graph_model = _model(weight_cache, manifest, "tiny_train_xe")
    eager_model.eval(); graph_model.eval()
    opt = cfg.to_opt()
    opt.noamopt, opt.learning_rate = False, 1e-3
    te, tg = XETrainer(eager_model, opt), XETrainer(graph_model, opt, graph=True)
    n_img, spi = 3, 4
    batches = []
    for seed in (1, 2, 3, 4):
        hb = synthetic_training_batch(cfg, n_img, spi, seed=seed)
        b = {k: torch.from_numpy(v).cuda() for k, v in hb.items()}
        b["att_feats"] = torch.from_numpy(synthetic_att_feats(n_img, 36, cfg.att_feat_size, seed=seed)).cuda()
        b["max_phrase_num"] = int(hb["phrase_num"].max())
        batches.append(b)
    for b in batches + batches:
        le, _ = te.step(b)
        lg, _ = tg.step(b)
        assert abs(float(le) - float(lg)) < 2e-4 * max(1.0, abs(float(le)))
    # Adam turns gradients that differ in the last bits (atomic accumulation order) into +-lr steps where |g| ~ eps
    assert len(tg._graphs) >= 1 and float((tg.bucket.flat - te.bucket.flat).abs().mean()) < 2e-5 and _maxdiff(tg.bucket.flat, te.bucket.flat) < 8e-3
    graph_model.train()
    l1 = float(tg.step(batches[0])[0]); l2 = float(tg.step(batches[0])[0]); l3 = float(tg.step(batches[0])[0])
    assert all(map(lambda v: v == v, (l1, l2, l3))) and len({round(l1, 5), round(l2, 5), round(l3, 5)}) == 3


def test_dynamic_padding_leaves_loss_and_gradients_unchanged(weight_cache, manifest):
    """With the longest caption's length as a host hint the decoder passes and the vocabulary projection skip the positions
    past it: same loss, same gradients (those positions are neither attended nor counted by the criterion)."""
    from boficap_amd.collate import max_tokens, synthetic_training_batch
    from boficap_amd.trainer import XETrainer
    from boficap_amd.weights import synthetic_att_feats
    cfg, full = _model(weight_cache, manifest, "tiny_train_xe")
    _, short = _model(weight_cache, manifest, "tiny_train_xe")
    full.eval(); short.eval()
    n_img, spi = 3, 3
    hb = synthetic_training_batch(cfg, n_img, spi, seed=12)
    mt = max_tokens(hb)
    assert mt < cfg.seq_length
    batch = {k: torch.from_numpy(v).cuda() for k, v in hb.items()}
    batch["att_feats"] = torch.from_numpy(synthetic_att_feats(n_img, 36, cfg.att_feat_size, seed=3)).cuda()
    batch["max_phrase_num"] = int(hb["phrase_num"].max())
    ta, tb = XETrainer(full), XETrainer(short)
    la, _ = ta.forward_backward(batch)
    lb, _ = tb.forward_backward(dict(batch, max_tokens=mt))
    assert abs(float(la) - float(lb)) < 1e-5 * max(1.0, abs(float(la)))
    assert _maxdiff(tb.bucket.grad, ta.bucket.grad) <= 1e-4 * max(1e-3, float(ta.bucket.grad.abs().max()))
    fc = torch.zeros(n_img, 0, device="cuda")
    from boficap_amd import xe
    outs = short(fc, batch["att_feats"], batch["labels"], None, batch["phrase_num"], batch["phrase_length"], batch["phrase_syn"],
                 batch["extend_phrase_syn_seq"], batch["extend_phrase_seq"], batch["extend_phrase_seq_mask"], -1.0, plan=xe.StepPlan(max_tokens=mt))
    assert outs[2].shape[1] == mt and outs[5].shape[1] == mt and outs[0].shape[1] == cfg.seq_length + 1


def test_failed_step_leaves_nothing_for_the_next_forward(weight_cache, manifest):
    """What a trainer knows about one batch reaches that batch's forward only: after a paired step, and a step that fails on the host
    before its forward has read anything, a plain model(...) call is the dense forward, and no per-step state is left armed."""
    from boficap_amd import hip, xe
    from boficap_amd.collate import max_tokens, synthetic_training_batch
    from boficap_amd.trainer import XETrainer
    from boficap_amd.weights import synthetic_att_feats
    cfg, model = _model(weight_cache, manifest, "tiny_train_xe")
    model.eval()
    model.train_dtype = torch.bfloat16                             # (the trainer's weight operands are armed in this mode)
    n_img, spi = 3, 3
    hb = synthetic_training_batch(cfg, n_img, spi, seed=12)
    assert max_tokens(hb) < cfg.seq_length
    batch = {k: torch.from_numpy(v).cuda() for k, v in hb.items()}
    batch["att_feats"] = torch.from_numpy(synthetic_att_feats(n_img, 36, cfg.att_feat_size, seed=3)).cuda()
    batch["max_phrase_num"] = int(hb["phrase_num"].max())
    tr = XETrainer(model)
    bb = tr.add_token_rows(batch, hb)
    assert "pair_src" in bb and "prep_tok2" in bb
    loss, _ = tr.forward_backward(bb)
    assert torch.isfinite(loss)
    flat = bb["labels"].reshape(n_img * spi, -1)
    with pytest.raises(hip.BofiHipError, match="captions for"):
        tr.forward_backward(dict(bb, labels=torch.cat([flat, flat[:1]])))     # one caption too many: N % B, checked on the host
    fc = torch.zeros(n_img, 0, device="cuda")
    outs = model(fc, batch["att_feats"], batch["labels"], None, batch["phrase_num"], batch["phrase_length"], batch["phrase_syn"],
                 batch["extend_phrase_syn_seq"], batch["extend_phrase_seq"], batch["extend_phrase_seq_mask"], -1.0)
    N, S = n_img * spi, cfg.seq_length
    assert outs[2].shape[:2] == (N, S) and outs[5].shape[:2] == (N, S)
    assert all(outs[i].shape[:2] == (N, S + 1) for i in (0, 1, 3, 4))
    assert xe._WEIGHTS["provider"] is None and xe._DEFER["list"] is None and xe._DEFER["side"] is None


def test_compact_vocabulary_rows_leave_loss_and_gradients_unchanged(weight_cache, manifest):
    """Projecting only the real tokens' rows onto the vocabulary (token_rows hint + criterion_uic_compact) gives the same
    loss and gradients as the dense [N, S, V] tensors with the criterion's mask; also through the captured graph."""
    from boficap_amd.collate import synthetic_training_batch
    from boficap_amd.trainer import XETrainer
    from boficap_amd.weights import synthetic_att_feats
    cfg, dense = _model(weight_cache, manifest, "tiny_train_xe")
    _, compact = _model(weight_cache, manifest, "tiny_train_xe")
    _, graphed = _model(weight_cache, manifest, "tiny_train_xe")
    for m in (dense, compact, graphed):
        m.eval()
    n_img, spi = 4, 3
    hb = synthetic_training_batch(cfg, n_img, spi, seed=21)
    batch = {k: torch.from_numpy(v).cuda() for k, v in hb.items()}
    batch["att_feats"] = torch.from_numpy(synthetic_att_feats(n_img, 36, cfg.att_feat_size, seed=4)).cuda()
    batch["max_phrase_num"] = int(hb["phrase_num"].max())
    ta, tb, tc = XETrainer(dense), XETrainer(compact), XETrainer(graphed, graph=True)
    la, pa = ta.forward_backward(batch)
    bb = tb.add_token_rows(batch, hb)
    assert bb["token_rows"].numel() % 256 == 0 and float(bb["token_weight"].sum()) == float((hb["phrase_length"].sum(-1) - 1).sum())
    lb, pb = tb.forward_backward(bb)
    assert abs(float(la) - float(lb)) < 1e-5 * max(1.0, abs(float(la)))
    assert all(abs(float(x) - float(y)) < 1e-5 * max(1.0, abs(float(x))) for x, y in zip(pa, pb))
    assert _maxdiff(tb.bucket.grad, ta.bucket.grad) <= 1e-4 * max(1e-3, float(ta.bucket.grad.abs().max()))
    lc, _ = tc.forward_backward(tc.add_token_rows(batch, hb))
    lc2, _ = tc.forward_backward(tc.add_token_rows(batch, hb))      # replay
    assert abs(float(lc2) - float(la)) < 1e-5 * max(1.0, abs(float(la)))
    assert _maxdiff(tc.bucket.grad, ta.bucket.grad) <= 1e-4 * max(1e-3, float(ta.bucket.grad.abs().max()))


@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_decoder_over_unpadded_rows_matches_padded(weight_cache, manifest, dtype, paired):
    """The decoder over the captions' real positions only (row lists from add_token_rows) against the padded [N, Sd] batch:
    same loss and gradients, with ragged region masks, in both GEMM dtypes; the glancing pass runs on the same rows.
    ``paired``: additionally the SA and the NA branch share one bound pass and one decoder pass (xe._forward_paired)."""
    from boficap_amd.collate import synthetic_training_batch
    from boficap_amd.trainer import XETrainer
    from boficap_amd.weights import synthetic_att_feats
    cfg, padded = _model(weight_cache, manifest, "tiny_train_xe")
    _, ragged = _model(weight_cache, manifest, "tiny_train_xe")
    for m in (padded, ragged):
        m.eval()
        m.train_dtype = dtype
    n_img, spi = 5, 3
    hb = synthetic_training_batch(cfg, n_img, spi, seed=33)
    batch = {k: torch.from_numpy(v).cuda() for k, v in hb.items()}
    batch["att_feats"] = torch.from_numpy(synthetic_att_feats(n_img, 36, cfg.att_feat_size, seed=6)).cuda()
    masks = torch.ones(n_img, 36)
    for b, n in enumerate((36, 20, 31, 7, 36)):
        masks[b, n:] = 0
    batch["att_masks"] = masks.cuda()
    batch["max_phrase_num"] = int(hb["phrase_num"].max())
    ta, tb = XETrainer(padded, unpadded=False), XETrainer(ragged, paired=paired)
    ba, bb = ta.add_token_rows(batch, hb), tb.add_token_rows(batch, hb)
    assert "row_cap" not in ba and bb["row_cap"].numel() == bb["token_rows"].numel() and ("pair_src" in bb) == paired
    if paired:
        T = int(bb["token_weight"].sum())
        assert float(bb["pair_w_sa"].sum()) == T == float(bb["pair_w_na"].sum()) and int(bb["pair_count"].sum()) == 2 * T
    la, pa = ta.forward_backward(ba)
    lb, pb = tb.forward_backward(bb)
    tol = 1e-5 if dtype == torch.float32 else 2e-2
    assert abs(float(la) - float(lb)) < tol * max(1.0, abs(float(la)))
    assert all(abs(float(x) - float(y)) < tol * max(1.0, abs(float(x))) for x, y in zip(pa, pb))
    gtol = 1e-4 if dtype == torch.float32 else 6e-2
    assert _maxdiff(tb.bucket.grad, ta.bucket.grad) <= gtol * max(1e-3, float(ta.bucket.grad.abs().max()))
    lg, _ = tb.forward_backward(bb, glat_p=0.5)                   # glancing pass over the same rows
    assert torch.isfinite(lg) and torch.isfinite(tb.bucket.grad).all()


@pytest.mark.parametrize("graph", [False, True])
def test_forward_branches_on_streams_leave_the_step_unchanged(weight_cache, manifest, graph):
    """SA bound / SA fill / NA bound / NA fill on four HIP streams (forward and, through autograd, backward) in eager steps, and the
    captured step of the same trainer (its branches on the capture stream): same loss and gradients as the one-stream step, dropout on."""
    from boficap_amd.collate import synthetic_training_batch
    from boficap_amd.trainer import XETrainer
    from boficap_amd.weights import synthetic_att_feats
    cfg, a = _model(weight_cache, manifest, "tiny_train_xe")
    _, b = _model(weight_cache, manifest, "tiny_train_xe")
    for m in (a, b):
        m.train()
        m.train_dtype = torch.bfloat16
        m.opt.seed = 5
    ta, tb = XETrainer(a, graph=graph, paired=False), XETrainer(b, graph=graph, streams=True, paired=False)
    assert tb._side is not None and ta._side is None
    for step in range(4):
        hb = synthetic_training_batch(cfg, 4, 3, seed=70 + step // 2)      # two signatures' worth of replays in graph mode
        batch = {k: torch.from_numpy(v).cuda() for k, v in hb.items()}
        batch["att_feats"] = torch.from_numpy(synthetic_att_feats(4, 36, cfg.att_feat_size, seed=19 + step)).cuda()
        batch["max_phrase_num"] = int(hb["phrase_num"].max())
        la, pa = ta.forward_backward(ta.add_token_rows(batch, hb))
        lb, pb = tb.forward_backward(tb.add_token_rows(batch, hb))
        torch.cuda.synchronize()
        assert abs(float(la) - float(lb)) < 1e-5 * max(1.0, abs(float(la))), step
        assert all(abs(float(x) - float(y)) < 1e-5 * max(1.0, abs(float(x))) for x, y in zip(pa, pb))
        # bf16 operands: a last-bit difference from the order of the float atomics can flip a rounding of dz
        assert _maxdiff(tb.bucket.grad, ta.bucket.grad) <= 4e-4 * max(1e-3, float(ta.bucket.grad.abs().max())), step
        assert float((tb.bucket.grad - ta.bucket.grad).abs().mean()) <= 2e-6 * max(1e-3, float(ta.bucket.grad.abs().max())), step
    lg, _ = tb.forward_backward(tb.add_token_rows(batch, hb), glat_p=0.5)
    assert torch.isfinite(lg) and torch.isfinite(tb.bucket.grad).all()


@pytest.mark.parametrize("graph", [False, True])
def test_weight_gradients_beside_the_backward_leave_the_step_unchanged(weight_cache, manifest, graph):
    """XETrainer.dw_every: the grouped weight-gradient launches started during the backward on a side stream (a few problems at a
    time) against the two launches after the backward: same loss, same gradients up to the order of the float atomics, dropout on,
    eager and as the captured step graph, which keeps them on the capture stream (two signatures, replays included)."""
    from boficap_amd.collate import synthetic_training_batch
    from boficap_amd.trainer import XETrainer
    from boficap_amd.weights import synthetic_att_feats
    cfg, a = _model(weight_cache, manifest, "tiny_train_xe")
    _, b = _model(weight_cache, manifest, "tiny_train_xe")
    for m in (a, b):
        m.train()
        m.train_dtype = torch.bfloat16
        m.opt.seed = 5
    ta, tb = XETrainer(a, graph=graph), XETrainer(b, graph=graph)
    ta.dw_every, tb.dw_every = 0, 3
    for step in range(4):
        hb = synthetic_training_batch(cfg, 4, 3, seed=70 + step // 2)
        batch = {k: torch.from_numpy(v).cuda() for k, v in hb.items()}
        batch["att_feats"] = torch.from_numpy(synthetic_att_feats(4, 36, cfg.att_feat_size, seed=19 + step)).cuda()
        batch["max_phrase_num"] = int(hb["phrase_num"].max())
        batch["max_tokens"] = int((hb["phrase_length"].sum(-1) - 1).max())
        la, pa = ta.forward_backward(ta.add_token_rows(batch, hb))
        lb, pb = tb.forward_backward(tb.add_token_rows(batch, hb))
        torch.cuda.synchronize()
        assert tb._dw_stream is not None and ta._dw_stream is None
        assert abs(float(la) - float(lb)) < 1e-5 * max(1.0, abs(float(la))), step
        assert _maxdiff(tb.bucket.grad, ta.bucket.grad) <= 4e-4 * max(1e-3, float(ta.bucket.grad.abs().max())), step
        assert float((tb.bucket.grad - ta.bucket.grad).abs().mean()) <= 2e-6 * max(1e-3, float(ta.bucket.grad.abs().max())), step


def test_bucket_weight_operands_match_per_use_casts(weight_cache, manifest):
    """WeightOperands (bf16 copy of the bucket kept by the optimiser kernel, all transposed weights from one launch) against
    the per-use casts / transposes: same loss and gradients step after step, the copy follows the optimiser and notices
    weights changed behind its back."""
    from boficap_amd.collate import synthetic_training_batch
    from boficap_amd.trainer import XETrainer
    from boficap_amd.weights import synthetic_att_feats
    cfg, a = _model(weight_cache, manifest, "tiny_train_xe")
    _, b = _model(weight_cache, manifest, "tiny_train_xe")
    for m in (a, b):
        m.eval()
        m.train_dtype = torch.bfloat16
    ta, tb = XETrainer(a, prepared_weights=False), XETrainer(b)
    assert ta.ops is None and tb.ops is not None
    for step in range(3):
        hb = synthetic_training_batch(cfg, 4, 3, seed=50 + step)
        batch = {k: torch.from_numpy(v).cuda() for k, v in hb.items()}
        batch["att_feats"] = torch.from_numpy(synthetic_att_feats(4, 36, cfg.att_feat_size, seed=9 + step)).cuda()
        batch["max_phrase_num"] = int(hb["phrase_num"].max())
        la, _ = ta.forward_backward(ta.add_token_rows(batch, hb))
        lb, _ = tb.forward_backward(tb.add_token_rows(batch, hb))
        assert abs(float(la) - float(lb)) < 1e-5 * max(1.0, abs(float(la)))
        assert _maxdiff(tb.bucket.grad, ta.bucket.grad) <= 1e-4 * max(1e-3, float(ta.bucket.grad.abs().max()))
        if step == 1:
            assert len(tb.ops._tables) == 1 and len(tb.ops._views) > 10        # learnt in step 0, batched from step 1 on
            for (o, N, K), view in list(tb.ops._views.items())[:8]:
                w = tb.bucket.flat[o:o + N * K].view(N, K)
                assert torch.equal(view[:, :N], w.bfloat16().t()) and float(view[:, N:].abs().sum()) == 0.0
        ta.optimizer_step()
        tb.optimizer_step()
        # (the two trainers' gradients differ by float-atomics ordering; Adam's g / sqrt(v) turns that into visible weight noise)
        assert float((tb.bucket.flat - ta.bucket.flat).abs().mean()) < 2e-5
        assert torch.equal(tb.ops.shadow, tb.bucket.flat.bfloat16())
    with torch.no_grad():
        b.model.generator.proj.weight.mul_(0.5)                   # somebody else edits a weight
    tb.ops.refresh_if_stale()
    assert torch.equal(tb.ops.shadow, tb.bucket.flat.bfloat16())


@pytest.mark.parametrize("mfma", [False, True])
@pytest.mark.parametrize("kdiv,self_attn", [(1, True), (2, False), (3, False), (6, False), (1, False)])
def test_attention_on_unpadded_rows(kdiv, self_attn, mfma):
    """q_start / q_count (variable rows per caption, padding rows at the end of the list) through the forward and both
    backward kernels: self-attention over each caption's own rows, cross-attention to the image's dense keys.  kdiv 3 and 6:
    an image's captions have 55 / 82 rows, which the MFMA backward walks in 32-row chunks shared by two wavefronts."""
    from boficap_amd import xe
    H, d, B, Lmax, R = 2, 128, 6, 20, 36
    g = torch.Generator().manual_seed(31 + kdiv)
    counts = torch.tensor([5, 20, 1, 0, 13, 8] if kdiv < 3 else [16, 20, 19, 7, 0, 20], dtype=torch.int32)
    if kdiv == 1 and not self_attn:                             # one item per key owner with more rows than a chunk (image-level lists)
        if not mfma:
            pytest.skip("the float32 VALU backward takes caption-sized items")
        counts, Lmax = torch.tensor([40, 20, 1, 0, 50, 8], dtype=torch.int32), 64
    starts = torch.cumsum(torch.cat([torch.zeros(1, dtype=torch.int32), counts[:-1]]), 0).to(torch.int32)
    T = int(counts.sum())
    Tp = T + 9                                                  # rows outside every segment
    klen = torch.zeros(Tp, dtype=torch.int32)
    for b in range(B):
        n, s0 = int(counts[b]), int(starts[b])
        lim = n if self_attn else R
        klen[s0:s0 + n] = torch.randint(1, lim + 1, (n,), generator=g).int() if n else klen[s0:s0 + n]
    if self_attn:
        buf = torch.randn(Tp, 3 * d, generator=g)
        qb, kvb, offs = buf, buf, (0, d, 2 * d)
    else:
        qb, kvb, offs = torch.randn(Tp, d, generator=g), torch.randn(B // kdiv * R, 2 * d, generator=g), (0, 0, d)
    dout = torch.randn(Tp, d, generator=g)
    dout[T:] = 0

    def ref(qb, kvb):
        out = torch.zeros(Tp, d)
        for b in range(B):
            n, s0 = int(counts[b]), int(starts[b])
            if n == 0:
                continue
            q = qb[s0:s0 + n, offs[0]:offs[0] + d].reshape(n, H, 64).transpose(0, 1)
            src = kvb[s0:s0 + n] if self_attn else kvb[(b // kdiv) * R:(b // kdiv + 1) * R]
            k = src[:, offs[1]:offs[1] + d].reshape(-1, H, 64).transpose(0, 1)
            v = src[:, offs[2]:offs[2] + d].reshape(-1, H, 64).transpose(0, 1)
            s = q @ k.transpose(-1, -2) / 8.0
            mask = torch.arange(k.shape[1]).view(1, 1, -1) < klen[s0:s0 + n].view(1, n, 1)
            out[s0:s0 + n] = (torch.softmax(s.masked_fill(~mask, float("-inf")), -1) @ v).transpose(0, 1).reshape(n, d)
        return out

    qr = qb.clone().requires_grad_()
    kr = qr if self_attn else kvb.clone().requires_grad_()
    ref(qr, kr).backward(dout)
    xe._COMPUTE["dtype"] = torch.bfloat16 if mfma else torch.float32
    tol = 3e-2 if mfma else 2e-4
    qd = qb.clone().cuda().requires_grad_()
    kd = qd if self_attn else kvb.clone().cuda().requires_grad_()
    seg = (starts.cuda(), counts.cuda(), self_attn)
    out = xe.attention(qd, kd, offs[0], offs[1], offs[2], B, H, Lmax, Lmax if self_attn else R, kdiv, klen.cuda(), 0, 1, 0, None, seg)
    assert _maxdiff(out.detach(), ref(qb, kvb)) < 1e-4 and float(out.detach()[T:].abs().max()) == 0.0
    out.backward(dout.cuda())
    assert _maxdiff(qd.grad, qr.grad) < tol * max(1.0, float(qr.grad.abs().max()))
    if not self_attn:
        assert _maxdiff(kd.grad, kr.grad) < tol * max(1.0, float(kr.grad.abs().max()))
    if mfma:
        # dropout(p_attn) on unpadded rows: the context is linear in V, so <dO, out> == <dV, V> exactly when the backward
        # regenerates the forward's keep mask (chunks of the backward cut across the captions the forward walks)
        qd = qb.clone().cuda().requires_grad_()
        kd = qd if self_attn else kvb.clone().cuda().requires_grad_()
        xe._register_shadow(qd, qd.detach().to(torch.bfloat16))
        if not self_attn:
            xe._register_shadow(kd, kd.detach().to(torch.bfloat16))
        out = xe.attention(qd, kd, offs[0], offs[1], offs[2], B, H, Lmax, Lmax if self_attn else R, kdiv, klen.cuda(), 0, 1, 0,
                           (0.3, 777, None), seg)
        ob = xe._shadow(out).float()
        nodrop = ref(qb.bfloat16().float(), kvb.bfloat16().float()).cuda()
        assert float((ob - nodrop).abs().max()) > 0.05                      # the mask did something
        out.backward(dout.cuda())
        vgrad = kd.grad[:, offs[2]:offs[2] + d]
        vval = kd.detach().bfloat16().float()[:, offs[2]:offs[2] + d]
        lhs, rhs = float((dout.cuda() * ob).sum()), float((vgrad * vval).sum())
        assert abs(lhs - rhs) < 2e-2 * max(1.0, abs(lhs)), (lhs, rhs)


@pytest.mark.parametrize("kdiv", [1, 2])
def test_attention_dropout_mask_on_unpadded_rows(kdiv):
    """dropout(p_attn) over unpadded rows (cross-attention to the image's dense keys): the keep mask, recovered with V = one-hot(key) per head
    so that the context row IS the dropped probability row, equals the documented one at element (global query row * H + h) * Lk + k."""
    from boficap_amd import xe
    H, d, B, Lmax, R, p, seed = 2, 128, 6, 20, 36, 0.3, 777
    g = torch.Generator().manual_seed(41 + kdiv)
    counts = torch.tensor([5, 20, 1, 0, 13, 8], dtype=torch.int32)
    starts = torch.cumsum(torch.cat([torch.zeros(1, dtype=torch.int32), counts[:-1]]), 0).to(torch.int32)
    T = int(counts.sum())
    Tp = T + 9
    klen = torch.zeros(Tp, dtype=torch.int32)
    klen[:T] = torch.randint(1, R + 1, (T,), generator=g).int()
    qb, kvb = torch.randn(Tp, d, generator=g), torch.randn(B // kdiv * R, 2 * d, generator=g)
    kvb[:, d:] = 0
    for i in range(B // kdiv):
        for k in range(R):
            for h in range(H):
                kvb[i * R + k, d + h * 64 + k] = 1.0
    seg = (starts.cuda(), counts.cuda(), False)
    xe._COMPUTE["dtype"] = torch.bfloat16
    xe._STEP_CACHE.clear(); xe._SHADOW_ONLY.clear()
    try:
        def run(drop):
            qd, kd = qb.clone().cuda().requires_grad_(), kvb.clone().cuda().requires_grad_()
            xe._register_shadow(qd, qd.detach().to(torch.bfloat16))
            xe._register_shadow(kd, kd.detach().to(torch.bfloat16))
            out = xe.attention(qd, kd, 0, 0, d, B, H, Lmax, R, kdiv, klen.cuda(), 0, 1, 0, drop, seg)
            return xe._shadow(out).float().cpu()
        P0 = run(None).view(Tp, H, 64)[:T, :, :R]                # [global row, h, k]
        Pd = run((p, seed, None)).view(Tp, H, 64)[:T, :, :R]
    finally:
        xe._COMPUTE["dtype"] = torch.float32
        xe._STEP_CACHE.clear(); xe._SHADOW_ONLY.clear()
    valid = (torch.arange(R).view(1, 1, R) < klen[:T].view(T, 1, 1)) & (P0 > 1e-3)
    keep = Pd > 0
    assert int(valid.sum()) > 4 * T * H
    assert torch.allclose(Pd[valid & keep], P0[valid & keep] / (1 - p), rtol=3e-2, atol=2e-3)
    kept = torch.from_numpy(cs.keep_mask(seed, 0, p, cs.attn_ids_unpadded(np.arange(T), H, R)))
    assert torch.equal(keep[valid], kept[valid])


def test_scheduled_sampling_step_vs_reference(weight_cache, manifest):
    """model(..., mode='forward') with model.ss_prob > 0 (tools/train.py:159-162 -> TransformerModel.py:1760-1766, ss_SAIC
    :1988-2121) against the REAL reference's outputs, loss and gradients for the same random() draws: the HIP path takes the
    loop's decisions without the tape and differentiates one batched pass over its final inputs (xe.forward_uic_ss)."""
    from boficap_amd import xe
    cfg, model = _model(weight_cache, manifest, "tiny_ss")
    model.eval()
    g = load_golden("tiny_ss")
    t = lambda k: torch.from_numpy(g[k]).cuda()
    fc = torch.zeros(g["att_feats"].shape[0], 0, device="cuda")
    it = iter(g["draws"])
    model.ss_prob = float(g["ss_prob"])
    model._ss_draw = lambda: float(next(it))
    outs = model(fc, t("att_feats"), t("labels"), None, t("phrase_num"), t("phrase_length"), t("phrase_syn"),
                 t("extend_phrase_syn_seq"), t("extend_phrase_seq"), t("extend_phrase_seq_mask"), -1.0)
    assert next(it, None) is None                               # the reference's number of draws, in its order
    assert (xe.HINTS.pop("ss_trace")["emitted"] == g["emitted_seq"]).all()
    for i, o in enumerate(outs):
        assert o.shape == g[f"out{i}"].shape
        assert _maxdiff(o, torch.from_numpy(g[f"out{i}"])) < 1e-4, f"output {i}"
    loss, parts = xe.criterion_uic(outs, t("phrase_num"), t("phrase_length"), t("phrase_syn"), t("labels"))
    assert abs(float(loss.detach()) - float(g["losses"][0])) < 1e-3
    loss.backward()
    params = dict(model.named_parameters())
    for n, ref_norm in zip([str(x) for x in g["grad_names"]], g["grad_norms"]):
        p = params[n]
        if ref_norm < 0:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, n
            continue
        assert p.grad is not None, n
        assert abs(float(p.grad.double().norm()) - ref_norm) <= 2e-3 * max(ref_norm, 1e-3), (n, float(p.grad.double().norm()), float(ref_norm))
        if "grad." + n in g:
            ref_g = torch.from_numpy(g["grad." + n])
            assert _maxdiff(p.grad, ref_g) <= 2e-3 * max(1e-3, float(ref_g.abs().max())), n


def test_scheduled_sampling_trainer_step(weight_cache, manifest):
    """XETrainer.step with ss_prob > 0 and dropout on, bf16 operands, graph=True requested: the step falls back to eager launches
    (the loop decides on the host), the dense criterion, finite loss, weights move."""
    from boficap_amd.collate import synthetic_training_batch
    from boficap_amd.trainer import XETrainer
    from boficap_amd.weights import synthetic_att_feats
    cfg, model = _model(weight_cache, manifest, "tiny_ss")
    model.train()
    model.train_dtype = torch.bfloat16
    model.ss_prob = 0.25
    tr = XETrainer(model, graph=True)
    hb = synthetic_training_batch(cfg, 3, 2, seed=3)
    batch = {k: torch.from_numpy(v).cuda() for k, v in hb.items()}
    batch["att_feats"] = torch.from_numpy(synthetic_att_feats(3, 36, cfg.att_feat_size, seed=4)).cuda()
    batch["max_phrase_num"] = int(hb["phrase_num"].max())
    before = tr.bucket.flat.clone()
    for _ in range(2):
        loss, parts = tr.step(tr.add_token_rows(batch, hb))
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and len(tr._graphs) == 0
    assert float((tr.bucket.flat - before).abs().max()) > 0


def test_tools_eval_entry_point(tmp_path):
    """python tools/eval.py (the reference's tools/eval.py:24-44,123 for this path): greedy NAIC decode of features with seeded
    weights, per-image entropy / perplexity (eval_utils.py:463-464), predictions json, and -- with a label file in the schema of
    scripts/prepro_labels_stanford.py:393-399 -- the validation loss of eval_split (eval_utils.py:440-453)."""
    import json
    import os
    import subprocess
    import sys
    from boficap_amd.config import FULL as cfg
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rng = np.random.default_rng(0)
    S, N = cfg.seq_length, 8
    ncap = np.full(N, 5)
    M = int(ncap.sum())
    labels, pnum = np.zeros((M, S), np.uint32), np.zeros(M, np.uint32)
    plen, plab = np.zeros((M, S), np.uint32), np.zeros((M, S), np.uint32)
    for m in range(M):
        lens = rng.integers(1, 4, int(rng.integers(2, 6)))
        pnum[m] = len(lens)
        plen[m, :len(lens)] = lens
        plab[m, :len(lens)] = rng.integers(4, 7, len(lens))
        labels[m, :lens.sum()] = rng.integers(7, cfg.tgt_vocab, lens.sum())
    end = np.cumsum(ncap).astype(np.uint32)
    lab_path, out_path = str(tmp_path / "labels.npz"), str(tmp_path / "pred.json")
    np.savez(lab_path, labels=labels, label_start_ix=(end - ncap + 1).astype(np.uint32), label_end_ix=end,
             label_length=(labels > 0).sum(1).astype(np.uint32), phrase_num=pnum, phrase_length=plen, phrase_label=plab)
    cmd = [sys.executable, os.path.join(root, "tools", "eval.py"), "--synthetic", str(N), "--batch_size", "8", "--dtype", "bf16",
           "--input_label_npz", lab_path, "--dump_json", out_path]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert f"decoded {N} images" in out.stdout
    loss = float(out.stdout.split("validation loss")[1].split()[0])
    assert np.isfinite(loss) and loss > 0
    pred = json.load(open(out_path))
    assert len(pred) == N and all(np.isfinite(p["entropy"]) and np.isfinite(p["perplexity"]) for p in pred if p["seq"])


def _grad_norm_check(model, names, ref_norms, tol=2e-3):
    params = dict(model.named_parameters())
    for n, ref_norm in zip(names, ref_norms):
        p = params[n]
        if ref_norm < 0:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, n
            continue
        got = float(p.grad.double().norm())
        assert abs(got - ref_norm) <= tol * max(float(ref_norm), 1e-3), (n, got, float(ref_norm))


def test_criterion_self_dis_and_drop_worst_vs_reference(weight_cache, manifest):
    """LanguageModelCriterion_UIC beyond the default (losses.py:336-339, 357-361, 366-368): self_dis=True against the reference's own
    loss, parts and gradient norms (tests/golden/tiny_criterion_variants); reduction 'none' + drop_worst (tools/train.py:216-220)
    against the oracle's statement of :358 -- the reference's own 'none' branch raises (recorded in the fixture)."""
    from boficap_amd import xe
    from boficap_amd.loss_wrapper import LossWrapper
    cfg, model = _model(weight_cache, manifest, "tiny_criterion_variants")
    model.eval()
    g = load_golden("tiny_criterion_variants")
    assert str(g["none_reference_raises"]) == "UnboundLocalError"
    t = lambda k: torch.from_numpy(g[k]).cuda()
    fc = torch.zeros(g["att_feats"].shape[0], 0, device="cuda")
    names = [str(n) for n in g["grad_names"]]
    args = (t("labels"), None, t("phrase_num"), t("phrase_length"), t("phrase_syn"), t("extend_phrase_syn_seq"), t("extend_phrase_seq"), t("extend_phrase_seq_mask"))

    model.zero_grad()
    outs = model(fc, t("att_feats"), *args, -1.0)
    loss, parts = xe.criterion_uic(outs, t("phrase_num"), t("phrase_length"), t("phrase_syn"), t("labels"), self_dis=True)
    assert abs(float(loss.detach()) - float(g["self_dis_losses"][0])) < 1e-3
    assert np.allclose([float(p.detach()) for p in parts], g["self_dis_losses"][1:], atol=1e-4)
    loss.backward()
    _grad_norm_check(model, names, g["self_dis_grad_norms"])

    model.zero_grad()
    outs = model(fc, t("att_feats"), *args, -1.0)
    per, none_parts = xe.criterion_uic(outs, t("phrase_num"), t("phrase_length"), t("phrase_syn"), t("labels"), reduction="none")
    assert none_parts is None and np.allclose(per.detach().cpu().numpy(), g["none_per_caption"], atol=1e-3)
    keep = int(per.shape[0] * (1 - float(g["drop_worst_rate"])))
    dw = torch.topk(per, k=keep, largest=False)[0].mean()
    assert abs(float(dw.detach()) - float(g["drop_worst_loss"])) < 1e-3
    dw.backward()
    _grad_norm_check(model, names, g["drop_worst_grad_norms"])

    # the wrapper's drop_worst_flag hands the per-caption vector to the caller (loss_wrapper.py:39, tools/train.py:216-220)
    opt = cfg.to_opt(structure_loss_type="new_self_critical", train_sample_n=5, structure_loss_weight=1, self_dis=True)
    lw = LossWrapper(model, opt)
    wargs = (fc, t("att_feats"), t("labels"), None, None, None, torch.arange(fc.shape[0]), False, False)
    tail = (None, t("phrase_num"), t("phrase_length"), t("phrase_syn"), t("extend_phrase_syn_seq"), t("extend_phrase_seq"), t("extend_phrase_seq_mask"), -1.0)
    with torch.no_grad():
        o_none = lw(*wargs, True, *tail)
        o_mean = lw(*wargs, False, *tail)
    assert o_none["loss"].shape == per.shape and np.allclose(o_none["loss"].cpu().numpy(), g["none_per_caption"], atol=1e-3)
    assert o_none["SA_length_loss"] is None
    assert abs(float(o_mean["loss"]) - float(g["self_dis_losses"][0])) < 1e-3


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_trainer_self_dis_drop_worst_and_norm_clipping(weight_cache, manifest, dtype):
    """XETrainer with opt.self_dis (configs uic_sd*), a drop_worst step and grad_clip_mode 'norm': the step's gradients equal the plain
    criterion's (float32: the fixture; bf16: finite and close), and the update equals torch's clip_grad_norm_ + Adam on the same gradients."""
    from boficap_amd.trainer import XETrainer
    cfg, model = _model(weight_cache, manifest, "tiny_criterion_variants")
    model.eval()
    model.train_dtype = dtype
    g = load_golden("tiny_criterion_variants")
    names = [str(n) for n in g["grad_names"]]
    opt = cfg.to_opt()
    opt.noamopt, opt.learning_rate, opt.self_dis, opt.grad_clip_mode, opt.grad_clip_value = False, 1e-3, True, "norm", 0.5
    opt.drop_worst_rate = float(g["drop_worst_rate"])
    tr = XETrainer(model, opt, graph=True)
    batch = {k: torch.from_numpy(g[k]).cuda() for k in XETrainer._KEYS}
    loss, parts = tr.forward_backward(batch)
    if dtype == torch.float32:
        assert abs(float(loss) - float(g["self_dis_losses"][0])) < 1e-3 and len(parts) == 6
        _grad_norm_check(model, names, g["self_dis_grad_norms"])
    else:
        assert abs(float(loss) - float(g["self_dis_losses"][0])) < 0.05 * float(g["self_dis_losses"][0])
    # the optimiser tail with norm clipping against torch on a copy of the same parameters and gradients
    live = tr.bucket.live_numel
    p0, g0 = tr.bucket.flat[:live].clone(), tr.bucket.grad[:live].clone()
    ref_p = torch.nn.Parameter(p0.clone())
    ref_p.grad = g0.clone()
    total = float(torch.linalg.vector_norm(g0))
    assert total > 0.5, total                                       # the clip must bite
    torch.nn.utils.clip_grad_norm_([ref_p], 0.5)
    adam = torch.optim.Adam([ref_p], lr=1e-3, betas=(tr.beta1, tr.beta2), eps=tr.eps)
    adam.step()
    tr.reduce_and_step()
    assert float((tr.bucket.flat[:live] - ref_p.detach()).abs().max()) < 2e-6
    # a drop_worst step: the loss of the best captions only
    loss_dw, parts_dw = tr.forward_backward(batch, drop_worst=True)
    assert parts_dw == []
    if dtype == torch.float32:
        # (the weights moved by one small step: compare with the plain criterion on the same weights instead of the fixture)
        from boficap_amd import xe
        fc = torch.zeros(g["att_feats"].shape[0], 0, device="cuda")
        with torch.no_grad():
            outs = model(fc, batch["att_feats"], batch["labels"], None, batch["phrase_num"], batch["phrase_length"], batch["phrase_syn"],
                         batch["extend_phrase_syn_seq"], batch["extend_phrase_seq"], batch["extend_phrase_seq_mask"], -1.0)
            per, _ = xe.criterion_uic(outs, batch["phrase_num"], batch["phrase_length"], batch["phrase_syn"], batch["labels"], reduction="none")
            keep = int(per.shape[0] * (1 - opt.drop_worst_rate))
            assert abs(float(loss_dw) - float(torch.topk(per, k=keep, largest=False)[0].mean())) < 1e-3
    assert torch.isfinite(loss_dw)


def test_xe_step_two_layer_bounding_network_vs_reference(weight_cache, manifest):
    """configs/uic_sd_N2.yml (N_len = 2): model(..., mode='forward') -> criterion -> backward against the REAL reference's outputs, losses
    and gradient norms (tests/golden/tiny_n2_train_xe).  The upper bound layer reads every visible row of the lower one, so the
    teacher-forced passes run whole sequences under each pass's tgt_mask (xe.bound_teacher_forced_dense); the trainer takes the same path."""
    from boficap_amd import xe
    from boficap_amd.trainer import XETrainer
    cfg, model = _model(weight_cache, manifest, "tiny_n2_train_xe")
    assert cfg.N_len == 2
    model.eval()
    g = load_golden("tiny_n2_train_xe")
    t = lambda k: torch.from_numpy(g[k]).cuda()
    fc = torch.zeros(g["att_feats"].shape[0], 0, device="cuda")
    outs = model(fc, t("att_feats"), t("labels"), None, t("phrase_num"), t("phrase_length"), t("phrase_syn"),
                 t("extend_phrase_syn_seq"), t("extend_phrase_seq"), t("extend_phrase_seq_mask"), -1.0)
    for i, o in enumerate(outs):
        assert o.shape == g[f"out{i}"].shape
        assert _maxdiff(o, torch.from_numpy(g[f"out{i}"])) < 1e-4, f"output {i}"
    loss, parts = xe.criterion_uic(outs, t("phrase_num"), t("phrase_length"), t("phrase_syn"), t("labels"))
    assert abs(float(loss.detach()) - float(g["losses"][0])) < 1e-3
    assert np.allclose([float(p.detach()) for p in parts], g["losses"][1:], atol=1e-4)
    loss.backward()
    names = [str(n) for n in g["grad_names"]]
    _grad_norm_check(model, names, g["grad_norms"])
    # the trainer (hints from the collate and all): the same loss and gradients through the plain form of the step
    model.zero_grad()
    opt = cfg.to_opt()
    opt.noamopt, opt.learning_rate = False, 1e-3
    tr = XETrainer(model, opt, graph=True)
    batch = {k: t(k) for k in XETrainer._KEYS}
    batch = tr.add_token_rows(dict(batch, max_phrase_num=int(g["phrase_num"].max())), {k: g[k] for k in XETrainer._KEYS if k != "att_feats"})
    loss2, parts2 = tr.forward_backward(batch)
    assert abs(float(loss2) - float(g["losses"][0])) < 1e-3 and len(parts2) == 6
    _grad_norm_check(model, names, g["grad_norms"])
