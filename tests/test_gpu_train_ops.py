"""The training step's kernels (csrc/train_ops.hip, csrc/attn_bwd_mfma.hip) one by one, at the smallest shapes that cross each
dispatch boundary and tile edge.  Every reference is plain torch on the CPU in float64, restated from the formula in the kernel's
header comment.  Two kinds of case per kernel:

  exact probes    the reduced operand holds small integers (or dyadic fractions), so every partial sum is representable in
                  float32 and the result is the same in any summation order, atomics included: the kernel must EQUAL the
                  float64 result.  A dropped, doubled or misplaced row / column / chunk shows whatever the tolerance.
                  Pure data movement (casts, transposes, masks) is compared bit for bit.
  random values   held to the bars the op-level tests of test_gpu_xe.py already use, times max(1, |reference|.max()).

Outputs a kernel leaves partly untouched are prefilled with a sentinel that is checked afterwards; everything a kernel must
write is prefilled with the same sentinel and must come back finite and different from it."""
import numpy as np
import pytest
import torch

import counter_streams as cs

pytestmark = pytest.mark.gpu

SENT = -8192.0                      # exact in float32 and bf16; no test value comes near it
U24 = 2.0 ** -24


def _hip():
    from boficap_amd import hip
    return hip


def _rc(name, *args):
    """Status of the C entry point ``name``; tensors go in as pointers, the current stream is appended."""
    hip = _hip()
    return getattr(hip.lib(), name)(*[hip.ptr(a) if isinstance(a, torch.Tensor) else a for a in args], hip.stream_ptr())


def _ok(name, *args):
    _hip().check(_rc(name, *args), name)


def _refused(name, *args):
    assert _rc(name, *args) != 0, f"{name} accepted arguments its header refuses"
    torch.cuda.synchronize()


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else (t.view(torch.int32) if t.dtype == torch.float32 else t)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _exact(dev, ref64):
    """The device's float32 result equals the float64 reference, which itself must be a float32 number (the probe's premise)."""
    ref32 = ref64.to(torch.float32)
    assert torch.equal(ref32.double(), ref64), "the probe's reference is not representable in float32"
    got = dev.detach().cpu()
    assert got.dtype == torch.float32 and got.shape == ref32.shape and bool(torch.isfinite(got).all())
    return torch.equal(got, ref32)


def _err(dev, ref64):
    got = dev.detach().cpu().double()
    assert got.shape == ref64.shape and bool(torch.isfinite(got).all())
    return float((got - ref64).abs().max()) if got.numel() else 0.0


def _bar(tol, ref64):
    return tol * max(1.0, float(ref64.abs().max()) if ref64.numel() else 0.0)


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _step_word(step):
    return None if step is None else torch.tensor([step], dtype=torch.int64, device="cuda")


# ================================================================================================ 1. LayerNorm backward
# header (train_ops.hip): y = g t / s + b, t = x - mean, sigma = sqrt(sum t^2 / (d-1)), s = sigma + eps;
#   dt = dyh / s - t (sum_j dyh_j t_j) / (s^2 sigma (d-1)) [the second term 0 where sigma = 0], dyh = dy g, dx = dt - mean(dt) (+ add);
#   dgain += sum_rows dy t / s, dbias += sum_rows dy
def _ln_ref(x, gain, dy, add):
    x, gain, dy = x.double(), gain.double(), dy.double()
    d = x.shape[1]
    t = x - x.mean(1, keepdim=True)
    sigma = ((t * t).sum(1, keepdim=True) / (d - 1)).sqrt()
    s = sigma + 1e-6
    dyh = dy * gain
    c = (dyh * t).sum(1, keepdim=True)
    coef = torch.where(sigma > 0, c / (s * s * sigma.clamp_min(1e-300) * (d - 1)), torch.zeros_like(c))
    dt = dyh / s - t * coef
    dx = dt - dt.mean(1, keepdim=True)
    if add is not None:
        dx = dx + add.double()
    return dx, (dy * t / s).sum(0), dy.sum(0)


def _ln_run(x, gain, dy, add, *, ex, dz=None, p=0.0, seed=0, step=None, base=2.0):
    rows, d = x.shape
    xd, gd, dyd = x.cuda(), gain.cuda(), dy.cuda()
    ad = None if add is None else add.cuda()
    dx = torch.full((rows, d), SENT, device="cuda")
    dg, db = torch.full((d,), base, device="cuda"), torch.full((d,), base, device="cuda")
    if ex:
        _ok("bofi_layernorm_bwd_ex", xd, gd, dyd, ad, dx, dg, db, rows, d, dz, p, seed, _step_word(step))
    else:
        _ok("bofi_layernorm_bwd", xd, gd, dyd, ad, dx, dg, db, rows, d)
    torch.cuda.synchronize()
    return dx, dg, db


def _ln_inputs(d, rows, with_add, seed):
    g = torch.Generator().manual_seed(seed)
    x, gain = torch.randn(rows, d, generator=g) * 2, torch.rand(d, generator=g) + 0.5
    add = torch.randn(rows, d, generator=g) if with_add else None
    return g, x, gain, add


LN_SHAPES = ([(d, r) for d in (128, 512) for r in (1, 7, 8, 9, 37)]        # ln_bwd_rows_kernel<2> / <8>: partial workgroup of 8 rows, a wavefront without a row
             + [(128, 4096 + 5)]                                             # 32 rows per workgroup, partial last workgroup
             + [(d, r) for d in (64, 192, 256) for r in (1, 5, 45)])         # generic ln_bwd_kernel: four rows per workgroup


@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("d,rows", LN_SHAPES)
def test_layernorm_bwd_every_kernel_and_rows_per_workgroup(d, rows, with_add):
    g, x, gain, add = _ln_inputs(d, rows, with_add, 1000 * d + rows)
    # random values (bofi_layernorm_bwd): dx 1e-4, dgain / dbias 1e-3
    dy = torch.randn(rows, d, generator=g)
    rdx, rdg, rdb = _ln_ref(x, gain, dy, add)
    dx, dg, db = _ln_run(x, gain, dy, add, ex=False)
    e = (_err(dx, rdx), _err(dg, rdg + 2.0), _err(db, rdb + 2.0))
    print(f"ln_bwd d={d} rows={rows} add={with_add}: |ddx| {e[0]:.3e} |ddgain| {e[1]:.3e} |ddbias| {e[2]:.3e}")
    assert e[0] < _bar(1e-4, rdx) and e[1] < _bar(1e-3, rdg) and e[2] < _bar(1e-3, rdb)
    # exact probe (bofi_layernorm_bwd_ex without dz): integer dy -> dbias is the column sum in any order; a row lost to either
    # rows-per-workgroup arithmetic changes it
    dyi = _ints(g, -8, 8, rows, d)
    rdx, rdg, rdb = _ln_ref(x, gain, dyi, add)
    dx, dg, db = _ln_run(x, gain, dyi, add, ex=True)
    assert _exact(db, rdb + 2.0)
    assert _err(dx, rdx) < _bar(1e-4, rdx) and _err(dg, rdg + 2.0) < _bar(1e-3, rdg)


@pytest.mark.parametrize("d", [128, 512, 192])
def test_layernorm_bwd_constant_row(d):
    """sigma = 0 in one row: the kernel defines coef = 0 there, so dx = (dy g - mean(dy g)) / eps (+ add), finite; torch autograd
    gives NaN for such a row, hence the formula by hand.  The other rows and dgain / dbias must not notice."""
    rows, r0 = 9, 4
    g, x, gain, add = _ln_inputs(d, rows, True, 77 + d)
    x[r0] = 1.5                                                  # the mean is exact: t = 0 in float32 too
    dy = torch.randn(rows, d, generator=g)
    rdx, rdg, rdb = _ln_ref(x, gain, dy, add)
    dyh = dy[r0].double() * gain.double()
    by_hand = (dyh - dyh.mean()) / 1e-6 + add[r0].double()
    assert float((rdx[r0] - by_hand).abs().max()) <= 1e-9 * float(by_hand.abs().max())
    dx, dg, db = _ln_run(x, gain, dy, add, ex=False)
    others = [r for r in range(rows) if r != r0]
    assert _err(dx[r0], by_hand) <= 1e-5 * float(by_hand.abs().max())
    assert _err(dx[others], rdx[others]) < _bar(1e-4, rdx[others])
    assert _err(dg, rdg + 2.0) < _bar(1e-3, rdg) and _err(db, rdb + 2.0) < _bar(1e-3, rdb)


@pytest.mark.parametrize("step", [None, 5])
@pytest.mark.parametrize("d", [128, 512])
def test_layernorm_bwd_hands_over_dz(d, step):
    """dz = bf16(keep ? dx / (1 - p) : 0) of the kernel's own dx, keep = the documented dropout stream over element row * d + col."""
    rows, p, seed = 37, 0.5, 4711
    g, x, gain, add = _ln_inputs(d, rows, True, 5 + d)
    dy = torch.randn(rows, d, generator=g)
    rdx, rdg, rdb = _ln_ref(x, gain, dy, add)
    dz = torch.full((rows, d), SENT, dtype=torch.bfloat16, device="cuda")
    dx, dg, db = _ln_run(x, gain, dy, add, ex=True, dz=dz, p=p, seed=seed, step=step)
    assert _err(dx, rdx) < _bar(1e-4, rdx) and _err(dg, rdg + 2.0) < _bar(1e-3, rdg) and _err(db, rdb + 2.0) < _bar(1e-3, rdb)
    keep = torch.from_numpy(cs.keep_mask(seed, step or 0, p, cs.linear_ids(rows, d)))
    assert 0.3 < float(keep.float().mean()) < 0.7
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    want = torch.where(keep, dx.cpu() * scale, torch.zeros(())).to(torch.bfloat16)
    assert _same_bits(dz, want)
    if step is not None:
        assert not np.array_equal(cs.keep_mask(seed, step, p, cs.linear_ids(rows, d)), cs.keep_mask(seed, 0, p, cs.linear_ids(rows, d)))


def test_layernorm_bwd_refuses_dz_for_other_widths():
    rows, d = 4, 256
    g, x, gain, _ = _ln_inputs(d, rows, False, 1)
    dz = torch.full((rows, d), SENT, dtype=torch.bfloat16, device="cuda")
    dx, dg, db = torch.full((rows, d), SENT, device="cuda"), torch.zeros(d, device="cuda"), torch.zeros(d, device="cuda")
    _refused("bofi_layernorm_bwd_ex", x.cuda(), gain.cuda(), x.cuda(), None, dx, dg, db, rows, d, dz, 0.5, 1, None)
    _refused("bofi_layernorm_bwd_ex", x.cuda(), gain.cuda(), x.cuda(), None, dx, dg, db, rows, 128, None, 1.0, 1, None)
    assert float(dx.max()) == SENT and float(dz.float().max()) == SENT and float(dg.abs().max()) == 0.0


# ================================================================================================ 2. / 3. attention backward
# header: P = softmax(Q K^T / 8 | key < klen), dV = P^T dO, dP = dO V^T, dS = P (dP - rowsum(dP P)), dQ = dS K / 8, dK = dS^T Q / 8;
# captions that share an image's keys (kdiv) add their dK / dV
def _attn_item(q, k, v, do, klen):
    """One item: q, do [n, H * 64], k, v [m, H * 64] float64, klen [n] -> out, dq [n, .], dk, dv [m, .]."""
    n, D = q.shape
    H, m = D // 64, k.shape[0]
    heads = lambda t: t.reshape(-1, H, 64).transpose(0, 1)
    back = lambda t: t.transpose(0, 1).reshape(-1, D)
    qh, kh, vh, doh = heads(q), heads(k), heads(v), heads(do)
    s = qh @ kh.transpose(1, 2) / 8.0
    mask = torch.arange(m).view(1, 1, m) < klen.view(1, n, 1)
    P = torch.softmax(s.masked_fill(~mask, float("-inf")), -1)
    dP = doh @ vh.transpose(1, 2)
    dS = P * (dP - (dP * P).sum(-1, keepdim=True))
    return back(P @ vh), back(dS @ kh / 8.0), back(dS.transpose(1, 2) @ qh / 8.0), back(P.transpose(1, 2) @ doh)


def _attn_ref(q, k, v, do, klen, B, Lq, Lk, kdiv):
    """Padded layout: q, do [B * Lq, D], k, v [B / kdiv * Lk, D], klen [B, Lq]."""
    q, k, v, do = q.double(), k.double(), v.double(), do.double()
    out, dq, dk, dv = torch.zeros_like(q), torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
    for b in range(B):
        qs, ks = slice(b * Lq, (b + 1) * Lq), slice(b // kdiv * Lk, (b // kdiv + 1) * Lk)
        o, a, c, e = _attn_item(q[qs], k[ks], v[ks], do[qs], klen[b])
        out[qs], dq[qs] = o, a
        dk[ks] += c
        dv[ks] += e
    return out, dq, dk, dv


def _probe_inputs(g, B, Lq, Lk, kdiv, zero, max_kl):
    """Exact probe: one of q / k is zero, so every score is 0 and P = 1 / klen with klen a power of two; dO has one +-1 per row
    and head, v and the other of q / k hold -1, 0, 1.  Then dP is -1, 0 or 1, rowsum(dP P) and dS are dyadic fractions with a
    handful of mantissa bits (exact in bf16 up to klen 64), and every sum of the backward is exact in float32."""
    D = 128
    q = torch.zeros(B * Lq, D) if zero == "q" else _ints(g, -1, 1, B * Lq, D)
    k = torch.zeros(B // kdiv * Lk, D) if zero == "k" else _ints(g, -1, 1, B // kdiv * Lk, D)
    v = _ints(g, -1, 1, B // kdiv * Lk, D)
    do = torch.zeros(B * Lq, D)
    col = torch.randint(0, 64, (B * Lq, 2), generator=g)
    sign = torch.randint(0, 2, (B * Lq, 2), generator=g).float() * 2 - 1
    for h in range(2):
        do[torch.arange(B * Lq), h * 64 + col[:, h]] = sign[:, h]
    pows = [1 << a for a in range(8) if (1 << a) <= min(Lk, max_kl)]
    klen = torch.tensor(pows, dtype=torch.int32)[torch.randint(0, len(pows), (B, Lq), generator=g)]
    return q, k, v, do, klen


F32_ATTN_CASES = [(2, 20, 100, 1),          # <32,128>, one chunk, plain stores
                  (4, 40, 70, 2), (5, 33, 65, 5),      # <32,128>, two chunks and shared keys: all atomics
                  (2, 64, 128, 1),          # the largest tile
                  (3, 70, 36, 1),           # <64,64> with two chunks
                  (2, 32, 33, 1), (2, 33, 32, 1),      # the <32,64> / <64,64> boundary
                  (2, 32, 32, 1)]           # <32,32>, full in both directions


def _attention_through_xe(B, Lq, Lk, kdiv, packed, compute, seed):
    from boficap_amd import xe
    H, d = 2, 128
    g = torch.Generator().manual_seed(seed)
    klen = torch.randint(1, Lk + 1, (B, Lq), generator=g).int()
    if packed:
        buf = torch.randn(B * Lq, 3 * d, generator=g)
        qb, kvb, offs = buf, buf, (0, d, 2 * d)
    else:
        qb, kvb, offs = torch.randn(B * Lq, d, generator=g), torch.randn(B // kdiv * Lk, 2 * d, generator=g), (0, 0, d)
    dout = torch.randn(B * Lq, d, generator=g)
    cut = lambda t, o: t[:, o:o + d]
    rout, rdq, rdk, rdv = _attn_ref(cut(qb, offs[0]), cut(kvb, offs[1]), cut(kvb, offs[2]), dout, klen, B, Lq, Lk, kdiv)
    xe._COMPUTE["dtype"] = compute
    xe._STEP_CACHE.clear(); xe._SHADOW_ONLY.clear()
    try:
        qd = qb.clone().cuda().requires_grad_()
        kd = qd if packed else kvb.clone().cuda().requires_grad_()
        out = xe.attention(qd, kd, offs[0], offs[1], offs[2], B, H, Lq, Lk, kdiv, klen.cuda().contiguous(), Lq, 1, 0)
        e_out = _err(out, rout)
        out.backward(dout.cuda())
        torch.cuda.synchronize()
    finally:
        xe._COMPUTE["dtype"] = torch.float32
        xe._STEP_CACHE.clear(); xe._SHADOW_ONLY.clear()
    want_q = torch.cat([rdq, rdk, rdv], 1) if packed else rdq
    e = [e_out, _err(qd.grad, want_q), 0.0 if packed else _err(kd.grad, torch.cat([rdk, rdv], 1))]
    print(f"attention B={B} Lq={Lq} Lk={Lk} kdiv={kdiv} packed={packed}: |dout| {e[0]:.3e} |d dq| {e[1]:.3e} |d dkv| {e[2]:.3e}")
    assert e[0] < 1e-4
    assert e[1] < _bar(2e-4, want_q)
    if not packed:
        assert e[2] < _bar(2e-4, torch.cat([rdk, rdv], 1))


@pytest.mark.parametrize("B,Lq,Lk,kdiv", F32_ATTN_CASES)
def test_attention_bwd_f32_random(B, Lq, Lk, kdiv):
    _attention_through_xe(B, Lq, Lk, kdiv, False, torch.float32, 100 * B + Lq + Lk)


def test_attention_bwd_f32_packed_self_attention():
    _attention_through_xe(2, 40, 40, 1, True, torch.float32, 4040)


def test_attention_bf16_mode_takes_the_f32_kernel_beyond_64_keys():
    """max_boxes = 100 regions in bf16 compute mode: no MFMA backward exists for 65..128 keys, AttentionFn must take the float32
    kernels -- and then meet the float32 bar."""
    _attention_through_xe(2, 20, 100, 1, False, torch.bfloat16, 20100)


def _attn_bwd_direct(q, k, v, do, klen, B, Lq, Lk, kdiv, plain):
    H = 2
    qd, kd, vd, dod = q.cuda(), k.cuda(), v.cuda(), do.cuda()
    dq = torch.full_like(qd, SENT)
    dk, dv = (torch.full_like(kd, SENT), torch.full_like(vd, SENT)) if plain else (torch.zeros_like(kd), torch.zeros_like(vd))
    _ok("bofi_attention_bwd", qd, 128, kd, 128, vd, 128, dod, 128, dq, dk, dv, B, H, Lq, Lk, kdiv, klen.cuda().contiguous(), Lq, 1, 0, None, None, 0)
    torch.cuda.synchronize()
    return dq, dk, dv


@pytest.mark.parametrize("zero", ["q", "k"])
@pytest.mark.parametrize("B,Lq,Lk,kdiv", F32_ATTN_CASES)
def test_attention_bwd_f32_exact_probe(B, Lq, Lk, kdiv, zero):
    """bofi_attention_bwd directly: the key-side sums over query chunks (gridDim.y) and over the captions of an image (kdiv) meet in
    atomics; with the probe's operands the result does not depend on their order, so a lost or doubled chunk shows exactly."""
    g = torch.Generator().manual_seed(7 * B + Lq + Lk)
    q, k, v, do, klen = _probe_inputs(g, B, Lq, Lk, kdiv, zero, 128)
    _, rdq, rdk, rdv = _attn_ref(q, k, v, do, klen, B, Lq, Lk, kdiv)
    plain = kdiv == 1 and Lq <= 32                              # one workgroup per (item, head) in every tile: plain stores, no zeroing needed
    dq, dk, dv = _attn_bwd_direct(q, k, v, do, klen, B, Lq, Lk, kdiv, plain)
    assert float(rdv.abs().max()) > 0 and float((rdq if zero == "q" else rdk).abs().max()) > 0
    assert _exact(dq, rdq) and _exact(dk, rdk) and _exact(dv, rdv)


@pytest.mark.parametrize("self_attn", [False, True])
def test_attention_bwd_f32_unpadded_rows(self_attn):
    """q_start / q_count with padding rows behind the last item.  Cross-attention to R = 100 dense keys shared by five captions
    (<32,128>, atomics); self-attention over each item's own rows (k_ragged) with up to 40 of them (<64,64>, plain stores)."""
    H, d, B = 2, 128, 5
    g = torch.Generator().manual_seed(55 + self_attn)
    counts = torch.tensor([40, 33, 0, 7, 20] if self_attn else [16, 20, 0, 7, 20], dtype=torch.int32)
    Lmax, R, kdiv = (40, 40, 1) if self_attn else (20, 100, 5)
    starts = torch.cumsum(torch.cat([torch.zeros(1, dtype=torch.int32), counts[:-1]]), 0).to(torch.int32)
    T = int(counts.sum())
    Tp = T + 9
    klen = torch.zeros(Tp, dtype=torch.int32)
    for b in range(B):
        n, s0 = int(counts[b]), int(starts[b])
        if n:
            klen[s0:s0 + n] = torch.randint(1, (n if self_attn else R) + 1, (n,), generator=g).int()
    do = torch.randn(Tp, d, generator=g)
    if self_attn:
        buf = torch.randn(Tp, 3 * d, generator=g)
        q, k, v, ldq, ldk = buf[:, :d], buf[:, d:2 * d], buf[:, 2 * d:], 3 * d, 3 * d
    else:
        q, kv = torch.randn(Tp, d, generator=g), torch.randn(R, 2 * d, generator=g)
        k, v, ldq, ldk = kv[:, :d], kv[:, d:], d, 2 * d
    rdq, rdk, rdv = torch.zeros(Tp, d).double(), torch.zeros(k.shape).double(), torch.zeros(k.shape).double()
    for b in range(B):
        n, s0 = int(counts[b]), int(starts[b])
        if n == 0:
            continue
        rows = slice(s0, s0 + n)
        ks = rows if self_attn else slice(0, R)
        _, a, c, e = _attn_item(q[rows].double(), k[ks].double(), v[ks].double(), do[rows].double(), klen[rows])
        rdq[rows] = a
        rdk[ks] += c
        rdv[ks] += e
    hip = _hip()
    off = lambda t, col: hip.C.c_void_p(t.data_ptr() + 4 * col)
    if self_attn:
        src = buf.cuda()
        grad = torch.full_like(src, SENT)                       # plain stores: everything outside the segments keeps the sentinel
        args = (off(src, 0), ldq, off(src, d), ldk, off(src, 2 * d), ldk, do.cuda(), d, off(grad, 0), off(grad, d), off(grad, 2 * d))
    else:
        qd, kvd = q.cuda(), kv.cuda()
        gq, gkv = torch.full_like(qd, SENT), torch.zeros_like(kvd)
        args = (qd, ldq, off(kvd, 0), ldk, off(kvd, d), ldk, do.cuda(), d, gq, off(gkv, 0), off(gkv, d))
    _ok("bofi_attention_bwd", *args, B, H, Lmax, R, kdiv, klen.cuda(), 0, 1, 0, starts.cuda(), counts.cuda(), int(self_attn))
    torch.cuda.synchronize()
    if self_attn:
        got_q, got_k, got_v = grad[:, :d], grad[:, d:2 * d], grad[:, 2 * d:]
        assert bool((grad[T:] == SENT).all())
        assert _err(got_k[:T], rdk[:T]) < _bar(2e-4, rdk) and _err(got_v[:T], rdv[:T]) < _bar(2e-4, rdv)
    else:
        got_q = gq
        assert bool((gq[T:] == SENT).all())
        assert _err(gkv[:, :d], rdk) < _bar(2e-4, rdk) and _err(gkv[:, d:], rdv) < _bar(2e-4, rdv)
    assert _err(got_q[:T], rdq[:T]) < _bar(2e-4, rdq)


MFMA_CASES = [(3, 32, 32, 1),               # <2,2,1>
              (4, 20, 36, 2),               # <2,4,2>: two wavefronts share an image's captions, dK / dV meet in LDS
              (3, 20, 36, 1),               # <2,4,1>
              (2, 64, 64, 1), (2, 33, 64, 1)]          # <4,4,1>
MFMA_IO = [("f32", "f32", "f32"), ("bf16", "f32", "f32"), ("bf16", "bf16", "f32"), ("bf16", "bf16", "bf16")]
_DT = {"f32": torch.float32, "bf16": torch.bfloat16}


def _attn_bwd_mfma(q, k, v, do, klen, B, Lq, Lk, kdiv, io):
    hip = _hip()
    code = {"f32": hip.DT_F32, "bf16": hip.DT_BF16}
    qd, kd, vd = [t.cuda().to(_DT[io[0]]) for t in (q, k, v)]
    dq = torch.full(q.shape, SENT, dtype=_DT[io[1]], device="cuda")
    dk, dv = [torch.full(k.shape, SENT, dtype=_DT[io[2]], device="cuda") for _ in range(2)]
    rc = _rc("bofi_attention_bwd_mfma", qd, 128, kd, 128, vd, 128, code[io[0]], do.cuda(), 128, dq, 128, dk, dv, 128, code[io[1]], code[io[2]],
             B, 2, Lq, Lk, kdiv, klen.cuda().contiguous(), Lq, 1, 0, 0.0, 0, None, None, None, 0, 0)
    torch.cuda.synchronize()
    return rc, dq, dk, dv


@pytest.mark.parametrize("io", MFMA_IO, ids=["-".join(t) for t in MFMA_IO])
@pytest.mark.parametrize("B,Lq,Lk,kdiv", MFMA_CASES)
def test_attention_bwd_mfma_random(B, Lq, Lk, kdiv, io):
    """The four instantiations of launch_t by their selecting shapes, float32 and bf16 operands, and the bf16 gradient outputs that
    grad_bf16 selects (dq; dk / dv as well for a packed self-attention).  The operands are bf16 numbers in either dtype."""
    g = torch.Generator().manual_seed(13 * B + Lq + Lk)
    rnd = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).float()
    q, k, v = rnd(B * Lq, 128), rnd(B // kdiv * Lk, 128), rnd(B // kdiv * Lk, 128)
    do = torch.randn(B * Lq, 128, generator=g)
    klen = torch.randint(1, Lk + 1, (B, Lq), generator=g).int()
    _, rdq, rdk, rdv = _attn_ref(q, k, v, do, klen, B, Lq, Lk, kdiv)
    rc, dq, dk, dv = _attn_bwd_mfma(q, k, v, do, klen, B, Lq, Lk, kdiv, io)
    assert rc == 0
    e = (_err(dq.float(), rdq), _err(dk.float(), rdk), _err(dv.float(), rdv))
    print(f"attn_bwd_mfma B={B} Lq={Lq} Lk={Lk} kdiv={kdiv} {io}: |d dq| {e[0]:.3e} |d dk| {e[1]:.3e} |d dv| {e[2]:.3e}")
    assert e[0] < _bar(3e-2, rdq) and e[1] < _bar(3e-2, rdk) and e[2] < _bar(3e-2, rdv)


@pytest.mark.parametrize("zero", ["q", "k"])
@pytest.mark.parametrize("B,Lq,Lk,kdiv", MFMA_CASES)
def test_attention_bwd_mfma_exact_probe(B, Lq, Lk, kdiv, zero):
    g = torch.Generator().manual_seed(17 * B + Lq + Lk)
    q, k, v, do, klen = _probe_inputs(g, B, Lq, Lk, kdiv, zero, 64)
    _, rdq, rdk, rdv = _attn_ref(q, k, v, do, klen, B, Lq, Lk, kdiv)
    rc, dq, dk, dv = _attn_bwd_mfma(q, k, v, do, klen, B, Lq, Lk, kdiv, ("bf16", "f32", "f32"))
    assert rc == 0
    assert _exact(dq, rdq) and _exact(dk, rdk) and _exact(dv, rdv)


@pytest.mark.parametrize("B,Lq,Lk,kdiv", [(2, 20, 65, 1), (2, 65, 36, 1), (3, 20, 36, 2)], ids=["Lk>64", "Lq>64-no-row-list", "B%kdiv"])
def test_attention_bwd_mfma_refusals(B, Lq, Lk, kdiv):
    g = torch.Generator().manual_seed(3)
    nk = (B + kdiv - 1) // kdiv * Lk
    q, k, v, do = [torch.randn(n, 128, generator=g) for n in (B * Lq, nk, nk, B * Lq)]
    klen = torch.full((B, Lq), Lk, dtype=torch.int32)
    rc, dq, dk, dv = _attn_bwd_mfma(q, k, v, do, klen, B, Lq, Lk, kdiv, ("f32", "f32", "f32"))
    assert rc != 0
    assert all(bool((t == SENT).all()) for t in (dq, dk, dv))    # nothing was launched


# ================================================================================================ 4. log-softmax / NLL backward
VOCABS = [1, 61, 255, 256, 257, 9491]       # one element; one wavefront with data; the 256-thread stride's edge; the model's vocabulary


def _logp(g, rows, V):
    return torch.log_softmax(torch.randn(rows, V, generator=g).double() * 3, 1).float()


@pytest.mark.parametrize("V", VOCABS)
def test_logsoftmax_bwd(V):
    """dx = dy - exp(y) rowsum(dy)."""
    rows = 3
    g = torch.Generator().manual_seed(V)
    y, dy = _logp(g, rows, V), torch.randn(rows, V, generator=g)
    ref = dy.double() - y.double().exp() * dy.double().sum(1, keepdim=True)
    dx = torch.full((rows, V), SENT, device="cuda")
    _ok("bofi_logsoftmax_bwd", y.cuda(), dy.cuda(), dx, rows, V)
    e = _err(dx, ref)
    print(f"logsoftmax_bwd V={V}: {e:.3e}")
    assert e < _bar(1e-5, ref)
    # exact probe: y = 0 (exp = 1 exactly) and integer dy: dx = dy - rowsum(dy), whichever wavefront and stride held which element
    dyi = _ints(g, -4, 4, rows, V)
    dx = torch.full((rows, V), SENT, device="cuda")
    _ok("bofi_logsoftmax_bwd", torch.zeros(rows, V, device="cuda"), dyi.cuda(), dx, rows, V)
    assert _exact(dx, dyi.double() - dyi.double().sum(1, keepdim=True))


def _nll_ref(y, labels, gp):
    onehot = torch.zeros(y.shape, dtype=torch.float64)
    onehot[torch.arange(y.shape[0]), labels] = 1.0
    return gp.double().view(-1, 1) * (onehot - y.double().exp())


@pytest.mark.parametrize("V", VOCABS)
def test_nll_bwd_float32(V):
    """dx[r][c] = dpicked[r] ((c == label[r]) - exp(y[r][c])); a row with dpicked == 0 is exactly zero."""
    hip = _hip()
    rows = 3
    g = torch.Generator().manual_seed(V + 1)
    y, labels = _logp(g, rows, V), torch.randint(0, V, (rows,), generator=g)
    gp = torch.tensor([0.75, 0.0, -1.3])
    ref = _nll_ref(y, labels, gp)
    dx = torch.full((rows, V), SENT, device="cuda")
    _ok("bofi_nll_bwd", y.cuda(), labels.cuda(), gp.cuda(), dx, hip.DT_F32, V, rows, V)
    e = _err(dx, ref)
    print(f"nll_bwd f32 V={V}: {e:.3e}")
    assert e < _bar(1e-5, ref)
    assert bool((_bits(dx[1]) == 0).all())
    # exact probe: y = 0 and dpicked in eighths
    gp = torch.tensor([0.625, 0.0, -1.5])
    dx = torch.full((rows, V), SENT, device="cuda")
    _ok("bofi_nll_bwd", torch.zeros(rows, V, device="cuda"), labels.cuda(), gp.cuda(), dx, hip.DT_F32, V, rows, V)
    assert _exact(dx, _nll_ref(torch.zeros(rows, V), labels, gp))
    # float32 output has no row stride of its own; no output is narrower than V
    dx = torch.full((rows, V + 64), SENT, device="cuda")
    _refused("bofi_nll_bwd", y.cuda(), labels.cuda(), gp.cuda(), dx, hip.DT_F32, V + 64, rows, V)
    if V > 1:
        _refused("bofi_nll_bwd", y.cuda(), labels.cuda(), gp.cuda(), dx, hip.DT_F32, V - 1, rows, V)
        _refused("bofi_nll_bwd", y.cuda(), labels.cuda(), gp.cuda(), dx, hip.DT_BF16, V - 1, rows, V)
    assert bool((dx == SENT).all())


@pytest.mark.parametrize("V", VOCABS)
def test_nll_bwd_bf16_with_pad_columns(V):
    """The bf16 operand of the vocabulary projection's backward GEMMs: row stride V rounded up to 64, pad columns zero."""
    hip = _hip()
    rows, ld = 3, (V + 63) // 64 * 64
    g = torch.Generator().manual_seed(V + 2)
    y, labels = _logp(g, rows, V), torch.randint(0, V, (rows,), generator=g)
    gp = torch.tensor([0.75, 0.0, -1.3])
    ref = _nll_ref(y, labels, gp)
    dx = torch.full((rows, ld), SENT, dtype=torch.bfloat16, device="cuda")
    _ok("bofi_nll_bwd", y.cuda(), labels.cuda(), gp.cuda(), dx, hip.DT_BF16, ld, rows, V)
    torch.cuda.synchronize()
    assert bool((_bits(dx[:, V:]) == 0).all()) and bool((_bits(dx[1]) == 0).all())
    # bf16 of the float32 formula: within one bf16 ulp (2^-7 of the value's binade) of the float64 value
    got = dx[:, :V].float().cpu().double()
    ulp = torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126))) - 7)
    assert bool(torch.isfinite(got).all()) and bool(((got - ref).abs() <= ulp).all())
    # exact probe: y = 0, dpicked in eighths -> +-dpicked or 0, bf16 numbers themselves
    gp = torch.tensor([0.625, 0.0, -1.5])
    dx = torch.full((rows, ld), SENT, dtype=torch.bfloat16, device="cuda")
    _ok("bofi_nll_bwd", torch.zeros(rows, V, device="cuda"), labels.cuda(), gp.cuda(), dx, hip.DT_BF16, ld, rows, V)
    want = torch.zeros(rows, ld, dtype=torch.float64)
    want[:, :V] = _nll_ref(torch.zeros(rows, V), labels, gp)
    assert bool((_bits(dx[:, V:]) == 0).all()) and bool((_bits(dx[1]) == 0).all())
    assert _exact(dx.float(), want)


# ================================================================================================ 5. UIC criterion
def _uic_case(N, Pm, L, c_len, c_syn, T, seed):
    g = torch.Generator().manual_seed(seed)
    eighths = lambda *s: torch.randint(-32, 1, s, generator=g).float() / 8
    lp = [eighths(N, Pm, c) for c in (c_len, c_syn, c_len, c_syn)]
    pnum = torch.randint(0, Pm + 1, (N,), generator=g)
    pnum[0] = Pm
    if N > 1:
        pnum[1] = 0
    plen, psyn = torch.randint(0, c_len, (N, L), generator=g), torch.randint(0, c_syn, (N, L), generator=g)
    picked = eighths(T)
    choice = torch.tensor([0.0, 1.0, 0.5])
    w_sa, w_na = choice[torch.randint(0, 3, (T,), generator=g)], choice[torch.randint(0, 3, (T,), generator=g)]
    w_sa[0] = 1.0                                                # the denominator is never zero
    dead = (w_sa == 0) & (w_na == 0)
    picked[dead & (torch.arange(T) % 2 == 0)] = float("-inf")    # a zero-weight row's log-prob must not reach the sums
    return lp, pnum, plen, psyn, picked, w_sa, w_na


def _uic_ref(lp, pnum, plen, psyn, picked, w_sa, w_na, Pm):
    """losses.py:319-369, reduction 'mean', in float64: the slot terms gather the log-probs at the labels of columns 1..Pm and are
    masked to the first phrase_num slots; the token terms are the picked log-probs under the SA / NA row weights; every part is
    divided by the number of counted SA tokens."""
    N = pnum.numel()
    mask = (torch.arange(Pm).view(1, Pm) < pnum.view(N, 1)).double()
    labels = [plen[:, 1:Pm + 1], psyn[:, 1:Pm + 1], plen[:, 1:Pm + 1], psyn[:, 1:Pm + 1]]
    slot = [-(t.double().gather(2, lab.unsqueeze(2)).squeeze(2) * mask).sum() for t, lab in zip(lp, labels)]
    pk = picked.double()
    tok = [-(torch.where(w != 0, pk * w.double(), torch.zeros_like(pk))).sum() for w in (w_sa, w_na)]
    denom = w_sa.double().sum()
    parts = torch.stack([slot[0], tok[0], slot[1], slot[2], tok[1], slot[3]]) / denom
    return parts, parts.sum(), denom, mask, labels


@pytest.mark.parametrize("N,Pm,L,c_len,c_syn,T", [(70, 17, 20, 9, 13, 2100 + 37), (1, 1, 2, 9, 13, 1)], ids=["strided", "smallest"])
def test_uic_criterion_forward_and_backward(N, Pm, L, c_len, c_syn, T):
    """One workgroup of 1024 threads walks N * Pm = 1190 slots and T = 2137 token rows: more than one stride of each.  All inputs
    are eighths and the weights 0, 1, 0.5, so the seven sums are exact; a part is one division, the loss a sum of six."""
    lp, pnum, plen, psyn, picked, w_sa, w_na = _uic_case(N, Pm, L, c_len, c_syn, T, 9 * N + T)
    parts, loss, denom, mask, labels = _uic_ref(lp, pnum, plen, psyn, picked, w_sa, w_na, Pm)
    dev = [t.cuda() for t in (*lp, pnum, plen, psyn, picked, w_sa, w_na)]
    head = (*dev[:4], N, Pm, c_len, c_syn, dev[4], dev[5], dev[6], L, dev[7], dev[8], dev[9], T)
    out = torch.full((8,), SENT, device="cuda")
    _ok("bofi_uic_criterion", *head, out)
    torch.cuda.synchronize()
    got = out.cpu().double()
    assert bool(torch.isfinite(got).all())
    assert float(got[7]) == float(denom)
    assert bool(((got[:6] - parts).abs() <= 8 * U24 * parts.abs()).all()), (got[:6], parts)
    assert abs(float(got[6] - loss)) <= 8 * U24 * abs(float(loss))
    # backward for dL/d(loss) = g
    gval = 0.75
    gl = torch.tensor([gval], device="cuda")
    d = [torch.full(t.shape, SENT, device="cuda") for t in lp] + [torch.full((T,), SENT, device="cuda")]
    _ok("bofi_uic_criterion_bwd", *head, gl, out, *d)
    torch.cuda.synchronize()
    scale = -gval / float(denom)
    for k in range(4):
        want = torch.zeros(lp[k].shape, dtype=torch.float64)
        want.scatter_(2, labels[k].unsqueeze(2), (mask * scale).unsqueeze(2))
        gk = d[k].cpu().double()
        assert bool(torch.isfinite(gk).all())
        assert bool((gk[want == 0] == 0).all())                  # exactly zero off the label of a counted slot
        assert bool(((gk - want).abs() <= 2 * U24 * want.abs()).all())
    want = scale * (w_sa.double() + w_na.double())
    gp = d[4].cpu().double()
    assert bool(torch.isfinite(gp).all()) and bool(((gp - want).abs() <= 2 * U24 * want.abs()).all())


# ================================================================================================ 6. column sums and embeddings
@pytest.mark.parametrize("M,N", [(1, 1), (63, 255), (64, 256), (65, 257)])
def test_colsum_add_exact(M, N):
    """out[n] += sum_m x[m][n]: 64-row slabs (gridDim.y) meet in atomics, 256 columns per workgroup."""
    g = torch.Generator().manual_seed(M + N)
    x, base = _ints(g, -8, 8, M, N), _ints(g, -5, 5, N)
    out = base.clone().cuda()
    _ok("bofi_colsum_add", x.cuda(), out, M, N)
    assert _exact(out, base.double() + x.double().sum(0))


def _embed_ids():
    """70 rows = two 32-row blocks and a rest.  tok: an all-BOS block; a negative id at the start, in the middle and at the end of
    the second block; ids alternating every row; runs inside a block.  syn: a negative id in the very first row and inside a
    block, runs that cross the 32- and the 64-row boundary."""
    tok = [5] * 32 + [-1] + [1, 2] * 4 + [7] * 7 + [-1] + [3] * 7 + [9] * 7 + [-1] + [4] * 3 + [-1] * 2 + [4]
    syn = [-1] + [2] * 19 + [6] * 24 + [1] * 9 + [-1] + [8] * 16
    assert len(tok) == 70 and len(syn) == 70
    return torch.tensor(tok), torch.tensor(syn)


def _embed_bwd_ref(dx, ids, n, scale):
    out = torch.zeros(n, dx.shape[1], dtype=torch.float64)
    on = ids >= 0
    out.index_add_(0, ids[on], dx.double()[on] * scale)
    return out


@pytest.mark.parametrize("d,exact", [(256, True), (128, False)])
def test_embed_bwd_runs_blocks_and_negative_ids(d, exact):
    """d_lut[id[r]] += sqrt(d) dx[r] through xe.embed's backward.  d = 256: the scale is 16 and dx integer, so both tables equal
    index_add in float64 however the runs were cut (two 128-column slices); d = 128: random values at the 1e-3 bar."""
    from boficap_amd import xe
    g = torch.Generator().manual_seed(d)
    tok, syn = _embed_ids()
    rows, L = tok.numel(), 10
    lut_t, lut_s, pe = torch.randn(30, d, generator=g), torch.randn(10, d, generator=g), torch.randn(L, d, generator=g)
    dx = _ints(g, -8, 8, rows, d) if exact else torch.randn(rows, d, generator=g)
    td, sd = lut_t.clone().cuda().requires_grad_(), lut_s.clone().cuda().requires_grad_()
    xe.embed(td, sd, pe.cuda(), tok.cuda(), syn.cuda(), L).backward(dx.cuda())
    torch.cuda.synchronize()
    rt, rs = _embed_bwd_ref(dx, tok, 30, float(d) ** 0.5), _embed_bwd_ref(dx, syn, 10, float(d) ** 0.5)
    if exact:
        assert _exact(td.grad, rt) and _exact(sd.grad, rs)
    else:
        assert _err(td.grad, rt) < _bar(1e-3, rt) and _err(sd.grad, rs) < _bar(1e-3, rs)


@pytest.mark.parametrize("d", [64, 256])
@pytest.mark.parametrize("which", ["tok", "syn", "both", "pos"])
def test_embed_rows_bit_exact(which, d):
    """x[r] = (tok . sqrt(d) + syn . sqrt(d)) + pe[pos or r % L], float32, in that order; a negative id leaves its term out.  The
    widths are those with sqrt(d) a power of two (half a 128-thread stride, and two of them): each product is then exact, so the
    float32 restatement holds bit for bit whether or not the compiler contracts a product into the following sum."""
    g = torch.Generator().manual_seed(d + len(which))
    tok, syn = _embed_ids()
    rows, L = tok.numel(), 7
    lut_t, lut_s, pe = torch.randn(30, d, generator=g), torch.randn(10, d, generator=g), torch.randn(40, d, generator=g)
    pos = torch.randint(0, 40, (rows,), generator=g) if which == "pos" else None
    use_t, use_s = which != "syn", which != "tok"
    sq = torch.tensor(float(np.float32(np.sqrt(np.float64(d)))))
    term = lambda lut, ids: torch.where((ids >= 0).view(-1, 1), lut[ids.clamp_min(0)] * sq, torch.zeros(()))
    pr = pe[pos] if pos is not None else pe[torch.arange(rows) % L]
    if use_t and use_s:
        both = ((tok >= 0) & (syn >= 0)).view(-1, 1)
        want = torch.where(both, (term(lut_t, tok) + term(lut_s, syn)) + pr, torch.where((tok >= 0).view(-1, 1), term(lut_t, tok) + pr,
                           torch.where((syn >= 0).view(-1, 1), term(lut_s, syn) + pr, pr)))
    else:
        lut, ids = (lut_t, tok) if use_t else (lut_s, syn)
        want = torch.where((ids >= 0).view(-1, 1), term(lut, ids) + pr, pr)
    x = torch.full((rows, d), SENT, device="cuda")
    _ok("bofi_embed_rows", lut_t.cuda() if use_t else None, lut_s.cuda() if use_s else None, pe.cuda(), tok.cuda() if use_t else None,
        syn.cuda() if use_s else None, None if pos is None else pos.cuda(), rows, L, d, x)
    torch.cuda.synchronize()
    assert _same_bits(x, want)


# ================================================================================================ 7. casts and transposes
@pytest.mark.parametrize("colsum", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("M,N,Mpad", [(1, 1, 64), (31, 33, 64), (70, 61, 128), (64, 64, 64)])
def test_transpose_pad(M, N, Mpad, dtype, colsum):
    """xt[n][m] = x[m][n] in the output dtype (round to nearest even), zero for M <= m < Mpad; colsum[n] += sum_m x[m][n]."""
    hip = _hip()
    g = torch.Generator().manual_seed(M + N + Mpad)
    ldx = N + 3                                                 # a row stride of its own; the columns behind N must not be read
    x = torch.full((M, ldx), 777.0)
    x[:, :N] = _ints(g, -8, 8, M, N) if colsum else torch.randn(M, N, generator=g)
    xt = torch.full((N, Mpad), SENT, dtype=dtype, device="cuda")
    base = _ints(g, -5, 5, N)
    acc = base.clone().cuda()
    _ok("bofi_transpose_pad", x.cuda(), ldx, xt, hip.dtype_code(xt), M, N, Mpad, acc if colsum else None)
    torch.cuda.synchronize()
    want = torch.zeros(N, Mpad)
    want[:, :M] = x[:, :N].t()
    assert _same_bits(xt, want.to(dtype))
    assert bool((_bits(xt[:, M:]) == 0).all())
    assert _exact(acc, base.double() + (x[:, :N].double().sum(0) if colsum else 0.0))


CAST_SHAPES = [(1, 1, 1, 4),                # scalar form, one element
               (33, 61, 61, 64),            # scalar form (ldx % 4 != 0), two row tiles
               (33, 61, 64, 64),            # vector form with the column tail inside a quad
               (70, 256, 256, 256),         # vector form, full tile, three row tiles
               (32, 258, 260, 320),         # a second column block: two data columns, then zeros
               (5, 1000, 1000, 1024)]       # four column blocks, a whole zero block of quads
CAST_MODES = ["plain", "relu", "drop", "drop-step", "relu-drop-step", "colsum", "colsum-relu-drop"]


@pytest.mark.parametrize("mode", CAST_MODES)
@pytest.mark.parametrize("M,N,ldx,ldy", CAST_SHAPES)
def test_cast_bf16(M, N, ldx, ldy, mode):
    """y[m][n] = bf16(x'[m][n]), zero for N <= n < ldy; x' = x where relu_y > 0 (else 0), then keep ? x / (1 - p) : 0 with the
    documented dropout stream over element m * N + n; colsum[n] += sum_m x'[m][n]."""
    g = torch.Generator().manual_seed(M + N + ldx + len(mode))
    sums, relu, drop = "colsum" in mode, "relu" in mode, "drop" in mode
    step = 5 if "step" in mode else None
    p, seed = (0.5, 2 ** 63 + 99) if drop else (0.0, 0)
    x = torch.full((M, ldx), 777.0)
    x[:, :N] = _ints(g, -8, 8, M, N) if sums else torch.randn(M, N, generator=g)
    ry = None
    if relu:
        ry = torch.randn(M, ldx, generator=g)
        ry[torch.rand(M, ldx, generator=g) < 0.2] = 0.0
        ry[torch.rand(M, ldx, generator=g) < 0.2] = -0.0
        ry[:, N:] = 1.0
    v = x[:, :N].clone()
    if relu:
        v = torch.where(ry[:, :N] > 0, v, torch.zeros(()))
    if drop:
        keep = torch.from_numpy(cs.keep_mask(seed, step or 0, p, cs.linear_ids(M, N)))
        v = torch.where(keep, v * float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))), torch.zeros(()))
    want = torch.zeros(M, ldy)
    want[:, :N] = v
    y = torch.full((M, ldy), SENT, dtype=torch.bfloat16, device="cuda")
    base = _ints(g, -5, 5, N)
    acc = base.clone().cuda()
    _ok("bofi_cast_bf16", x.cuda(), ldx, y, ldy, M, N, acc if sums else None, None if ry is None else ry.cuda(), p, seed, _step_word(step))
    torch.cuda.synchronize()
    assert _same_bits(y, want.to(torch.bfloat16))
    assert bool((_bits(y[:, N:]) == 0).all())
    assert _exact(acc, base.double() + (v.double().sum(0) if sums else 0.0))


def test_cast_bf16_refusals():
    x, y = torch.randn(4, 61).cuda(), torch.full((4, 64), SENT, dtype=torch.bfloat16, device="cuda")
    _refused("bofi_cast_bf16", x, 61, y, 62, 4, 61, None, None, 0.0, 0, None)          # ldy % 4
    _refused("bofi_cast_bf16", x, 61, y, 64, 4, 61, None, None, 1.0, 0, None)          # p = 1
    assert bool((y == SENT).all())


def test_transpose_many():
    """One table of four bf16 matrices [N, K] -> [K, Np], Np = N rounded up to 64; the columns N..Np-1 are the caller's."""
    shapes = [(64, 64), (20, 128), (130, 70), (61, 200)]
    g = torch.Generator().manual_seed(21)
    mats = [torch.randn(n, k, generator=g).to(torch.bfloat16) for n, k in shapes]
    order = [2, 0, 3, 1]                                        # where each matrix sits in the source: not in table order
    src_off, pos = {}, 5 * 8                                    # (and not at offset 0)
    for e in order:
        src_off[e] = pos
        pos += mats[e].numel() + 8
    src = torch.full((pos,), 3.0, dtype=torch.bfloat16)
    for e, m in enumerate(mats):
        src[src_off[e]:src_off[e] + m.numel()] = m.reshape(-1)
    table, tile_first, dst_off, tiles = [], [0], [], 0
    dpos = 0
    for e, (n, k) in enumerate(shapes):
        npad = (n + 63) // 64 * 64
        dst_off.append(dpos)
        table.append([src_off[e], dpos, n, k, npad])
        dpos += k * npad
        tiles += ((n + 63) // 64) * ((k + 63) // 64)
        tile_first.append(tiles)
    dst = torch.full((dpos,), SENT, dtype=torch.bfloat16, device="cuda")
    tab, tf = torch.tensor(table, dtype=torch.int64).cuda(), torch.tensor(tile_first, dtype=torch.int32).cuda()
    _ok("bofi_transpose_many", src.cuda(), dst, tab, tf, 0, 0)   # n = 0: nothing happens
    torch.cuda.synchronize()
    assert bool((dst == SENT).all())
    _ok("bofi_transpose_many", src.cuda(), dst, tab, tf, len(shapes), tiles)
    torch.cuda.synchronize()
    out = dst.cpu()
    for e, (n, k) in enumerate(shapes):
        npad = (n + 63) // 64 * 64
        got = out[dst_off[e]:dst_off[e] + k * npad].view(k, npad)
        assert _same_bits(got[:, :n].contiguous(), mats[e].t().contiguous())
        assert bool((got[:, n:] == SENT).all())


@pytest.mark.parametrize("n", [1, 255, 256 * 4096 + 3])
def test_relu_bwd(n):
    """dx = dy where y > 0, else 0; the last size is past the 4096-workgroup grid cap (grid-stride loop)."""
    g = torch.Generator().manual_seed(n % 1000)
    y, dy = torch.randn(n, generator=g), torch.randn(n, generator=g)
    y[1::5] = 0.0
    y[2::5] = -0.0
    if n == 1:
        y[0] = 0.5
    dx = torch.full((n,), SENT, device="cuda")
    _ok("bofi_relu_bwd", y.cuda(), dy.cuda(), dx, n)
    torch.cuda.synchronize()
    assert _same_bits(dx, torch.where(y > 0, dy, torch.zeros(())))
    if n == 1:
        _ok("bofi_relu_bwd", torch.tensor([-0.0]).cuda(), dy.cuda(), dx, n)
        assert _same_bits(dx, torch.zeros(1))
