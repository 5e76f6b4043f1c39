"""The decode engine's packed operands (bofi_engine::repack: boficap_amd/csrc/repack.hip, pack_frag16_kernel / bound_q0_kernel / bound_tables_kernel
of bound_loop.hip) against an independent restatement of the packing on the CPU, from the float32 state dict alone.

Every buffer a decode kernel reads is copied back with bofi_engine_debug_copy and compared with what the kernels' stated arithmetic gives in
numpy / torch: bit for bit where the arithmetic is a copy, one float32 product, one rounding or an exact (double) sum; under a bar derived from the
summation length and the terms' magnitudes where it is a float32 accumulation.  Nothing here imports a packing, folding or permuting helper of the
product: the fold, the stacking order, the fragment-major permutation and the tables are written out below.

The comparisons run after load_state_dict, after a refresh_from_device with a second weight set (descriptor tables uploaded anew, the caller's
stream), after a refresh back to the first set from other tensors (bit-equal to the first read-back) and after a refresh from the same tensors
overwritten in place (the cached descriptor tables)."""
import dataclasses
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED_A, SEED_B = 11, 12          # two weight sets; a seed that misses one of the input conditions of test_restatement_tells_wrong_packings_apart is replaced


def _configs():
    from boficap_amd.config import FULL, TINY
    loop = dataclasses.replace(FULL, vocab_size=60, att_feat_size=64, d_ff=512, N_enc=1, N_dec=1)      # the smallest shape the persistent bounding-loop kernel takes
    dec8 = dataclasses.replace(TINY, N_dec=8)                                                        # kv_all stacks 18 matrices: two descriptor-table entries
    return {"tiny": TINY, "loop": loop, "dec8": dec8}


CASES = [("tiny", "f32"), ("tiny", "bf16"), ("loop", "bf16"), ("dec8", "f32"), ("dec8", "bf16")]
BL = "model.length_predictor.LengthPredictor.0"
LP = "model.length_predictor"


# ------------------------------------------------------------------------------------------------------------------------------
# what the engine declares (the make_lin / make_norm calls of bofi_engine_finalize, N_len = 1)
@dataclasses.dataclass(frozen=True)
class LinDecl:
    first: str               # first stacked prefix: the read-back name
    prefixes: tuple
    n_each: int
    K: int
    fold: str                # prefix of the pre-norm LayerNorm folded in ("" = none)
    pad_to: int
    frag: bool               # a fragment-major bf16 copy is kept (bf16 engine)
    f16: bool                # an fp16 fragment-major copy is kept (loop configuration)
    nth: int                 # this is the nth declared Linear that starts with `first`

    @property
    def N(self):
        return self.n_each * len(self.prefixes)

    @property
    def Npad(self):
        return -(-self.N // self.pad_to) * self.pad_to if self.pad_to else self.N

    def name(self, field):
        return f"{field}@{self.first}" + (f"#{self.nth}" if self.nth else "")


def _loop_config(cfg, bf16):
    return bf16 and cfg.d_model == 512 and cfg.h == 8 and cfg.d_ff % 512 == 0 and cfg.d_ff <= 2048 and cfg.seq_length + 2 <= 24 and cfg.head_hidden <= 128 and cfg.N_len == 1


def lin_table(cfg, bf16):
    assert cfg.N_len == 1
    d, dff, V, hh = cfg.d_model, cfg.d_ff, cfg.tgt_vocab, cfg.head_hidden
    loop = _loop_config(cfg, bf16)
    rows = []

    def lin(prefixes, n_each, K, fold="", pad_to=0, frag=False, f16=False):
        rows.append((tuple(prefixes), n_each, K, fold, pad_to, frag, f16))

    def attn(p):
        return [f"{p}.linears.{i}" for i in range(3)]

    lin(["att_embed.0"], d, cfg.att_feat_size)
    for l in range(cfg.N_enc):
        p = f"model.encoder.layers.{l}"
        lin(attn(f"{p}.self_attn"), d, d, f"{p}.sublayer.0.norm", 0, True)
        lin([f"{p}.self_attn.linears.3"], d, d, "", 0, True)
        lin([f"{p}.feed_forward.w_1"], dff, d, f"{p}.sublayer.1.norm", 0, True)
        lin([f"{p}.feed_forward.w_2"], d, dff, "", 0, True)
    kvs = [f"{BL}.src_attn.linears.1", f"{BL}.src_attn.linears.2"]
    for l in range(cfg.N_dec):
        p = f"model.decoder.layers.{l}"
        lin(attn(f"{p}.self_attn"), d, d, f"{p}.sublayer.0.norm", 0, True)
        lin([f"{p}.self_attn.linears.3"], d, d, "", 0, True)
        lin([f"{p}.src_attn.linears.0"], d, d, f"{p}.sublayer.1.norm", 0, True)
        lin([f"{p}.src_attn.linears.3"], d, d, "", 0, True)
        lin([f"{p}.feed_forward.w_1"], dff, d, f"{p}.sublayer.2.norm", 0, True)
        lin([f"{p}.feed_forward.w_2"], d, dff, "", 0, True)
        kvs += [f"{p}.src_attn.linears.1", f"{p}.src_attn.linears.2"]
    lin(kvs, d, d, "model.encoder.norm", 0, True)
    lin(["model.generator.proj"], V, d, "model.decoder.norm", 128, True)
    lin([f"{BL}.self_attn.linears.3"], d, d, f16=loop)
    lin([f"{BL}.src_attn.linears.0"], d, d, f"{BL}.sublayer.1.norm", f16=loop)
    lin([f"{BL}.src_attn.linears.3"], d, d, f16=loop)
    lin([f"{BL}.ff.w_1"], dff, d, f"{BL}.sublayer.2.norm", f16=loop)
    lin([f"{BL}.ff.w_2"], d, dff, f16=loop)
    if loop:
        lin([f"{LP}.Length_classifier1", f"{LP}.Syntactic_classifier1"], hh, d, f"{LP}.norm", 256, f16=True)
    lin([f"{BL}.self_attn.linears.1", f"{BL}.self_attn.linears.2"], d, d)
    lin([f"{BL}.self_attn.linears.0"], d, d)
    lin([f"{BL}.self_attn.linears.1", f"{BL}.self_attn.linears.2"], d, d, f"{BL}.sublayer.0.norm")
    seen, out = {}, []
    for prefixes, n_each, K, fold, pad_to, frag, f16 in rows:
        nth = seen.get(prefixes[0], 0)
        seen[prefixes[0]] = nth + 1
        out.append(LinDecl(prefixes[0], prefixes, n_each, K, fold, pad_to, frag, f16, nth))
    return out


def norm_table(cfg):
    out = []
    for l in range(cfg.N_enc):
        out += [f"model.encoder.layers.{l}.sublayer.{k}.norm" for k in range(2)]
    out.append("model.encoder.norm")
    for l in range(cfg.N_dec):
        out += [f"model.decoder.layers.{l}.sublayer.{k}.norm" for k in range(3)]
    out.append("model.decoder.norm")
    out += [f"{BL}.sublayer.{k}.norm" for k in range(3)]
    out.append(f"{LP}.norm")
    return out


def has_wp(l, bf16):
    return l.frag and bf16 and l.Npad % 64 == 0 and l.K % 32 == 0


# ------------------------------------------------------------------------------------------------------------------------------
# the restatement
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _cast(x32, bf16):
    """float32 tensor -> the compute dtype (bf16: round to nearest even, torch's conversion)."""
    return x32.to(torch.bfloat16) if bf16 else x32


def frag_major(w):
    """[Npad][K] -> [Npad/64 chunks][K/32 steps][4 tiles][64 lanes][8]: lane l of tile t holds row chunk*64 + t*16 + (l & 15), columns step*32 + (l >> 4)*8 .. +7
    (the layout test_pack_frag_layout asserts of the stand-alone kernel)."""
    Npad, K = w.shape
    v = w.reshape(Npad // 64, 4, 16, K // 32, 4, 8)          # chunk, tile, lane & 15, step, lane >> 4, element
    return v.permute(0, 3, 1, 4, 2, 5).contiguous().reshape(-1)


def restate_lin(sd, l, bf16):
    """w (compute dtype, [Npad][K]), b and cs (float32 [Npad], cs None without a fold), and -- loop configuration -- the fp16 [Npad][K] matrix behind wp16."""
    W = torch.cat([_t(sd[p + ".weight"]) for p in l.prefixes], 0)             # float32 [N][K], recipe order
    b = torch.cat([_t(sd[p + ".bias"]) for p in l.prefixes], 0)
    assert W.shape == (l.N, l.K) and W.dtype == torch.float32
    w_pad = torch.zeros(l.Npad, l.K, dtype=torch.bfloat16 if bf16 else torch.float32)
    b_pad = torch.zeros(l.Npad)
    cs_pad, prod = None, W
    if l.fold:
        gain, bln = _t(sd[l.fold + ".a_2"]), _t(sd[l.fold + ".b_2"])
        prod = W * gain[None, :]                                                # ONE float32 product
        c = b.double() + (W.double() * bln.double()[None, :]).sum(1)            # of w, not of w * gain; every product exact in double
        b_pad[:l.N] = c.float()
    else:
        b_pad[:l.N] = b
    w_pad[:l.N] = _cast(prod, bf16)
    if l.fold:
        cs_pad = torch.zeros(l.Npad)
        cs_pad[:l.N] = w_pad[:l.N].double().sum(1).float()                      # of the weight AS STORED
    w16 = None
    if l.f16:
        w16 = torch.zeros(l.Npad, l.K, dtype=torch.float16)
        w16[:l.N] = prod.clamp(-65504.0, 65504.0).to(torch.float16)             # float32 product, clamp, round to nearest even
    return w_pad, b_pad, cs_pad, w16


def layer_norm64(x, gain, bias):
    """LayerNorm of the reference: unbiased std, eps added to the std."""
    x = x.double()
    mean = x.mean(-1, keepdim=True)
    std = x.std(-1, keepdim=True)
    return gain.double() * (x - mean) / (std + 1e-6) + bias.double()


def restate_input_tables(sd, cfg, pe):
    """xt [L*10][d], x0, x0_sa, x0b: the product is rounded to float32 before the sum."""
    d, L = cfg.d_model, cfg.seq_length + 2
    sq = np.float32(math.sqrt(float(d)))
    syn, tok = sd["model.syn_embed.lut.weight"], sd["model.tgt_embed.lut.weight"]
    prod = (syn * sq).astype(np.float32)                                        # [10][d]
    xt = (prod[None, :, :] + pe[:L, None, :]).astype(np.float32).reshape(L * 10, d)
    x0 = xt[cfg.len_idx].copy()
    x0_sa = ((tok[cfg.len_idx] * sq).astype(np.float32) + pe[0]).astype(np.float32)
    x0b = (x0 + sd[f"{BL}.self_attn.linears.3.bias"]).astype(np.float32)
    fused = (syn.astype(np.float64)[None] * float(sq) + pe[:L, None, :].astype(np.float64)).astype(np.float32).reshape(L * 10, d)      # what a contraction to one FMA gives
    return dict(xt=xt, x0=x0, x0_sa=x0_sa, x0b=x0b), fused


def restate_w1(sd, cfg, bf16):
    d, hh = cfg.d_model, cfg.head_hidden
    w1t = np.concatenate([sd[f"{LP}.Length_classifier1.weight"].T, sd[f"{LP}.Syntactic_classifier1.weight"].T], 1).astype(np.float32)      # [d][2*hh]
    b1 = np.concatenate([sd[f"{LP}.Length_classifier1.bias"], sd[f"{LP}.Syntactic_classifier1.bias"]]).astype(np.float32)
    # pack_w1p_kernel: w1p[((slice*nld + u)*ng + grp)*EPL + kk*4 + o] = w1t[(slice*kps + u*KPL + kk)*nh + grp*4 + o], EPL elements per 16 bytes, KPL = EPL / 4
    nh = 2 * hh
    epl = 8 if bf16 else 4
    kpl, ng, kps = epl // 4, nh // 4, d // 8
    nld = kps // kpl
    v = _cast(_t(w1t), bf16).reshape(8, nld, kpl, ng, 4)                       # slice, u, kk, grp, o
    w1p = v.permute(0, 1, 3, 2, 4).contiguous().reshape(-1)
    return w1t, b1, w1p


def restate_gemm_tables(sd, cfg, bf16, tabs):
    """kvtab / q0 / q0_sa in float64: from the operands as they are (a) and with LayerNorm output and weight rounded to the compute dtype (b)."""
    g, nb = _t(sd[f"{BL}.sublayer.0.norm.a_2"]), _t(sd[f"{BL}.sublayer.0.norm.b_2"])
    wkv = torch.cat([_t(sd[f"{BL}.self_attn.linears.{i}.weight"]) for i in (1, 2)], 0)
    bkv = torch.cat([_t(sd[f"{BL}.self_attn.linears.{i}.bias"]) for i in (1, 2)], 0)
    wq, bq = _t(sd[f"{BL}.self_attn.linears.0.weight"]), _t(sd[f"{BL}.self_attn.linears.0.bias"])

    def rnd(x64):
        return _cast(x64.float(), bf16).double() if bf16 else x64

    out = {}
    for name, x, w, b in (("kvtab", tabs["xt"], wkv, bkv), ("q0", tabs["x0"][None], wq, bq), ("q0_sa", tabs["x0_sa"][None], wq, bq)):
        xn = layer_norm64(_t(x), g, nb)
        a = xn @ w.double().T + b.double()
        bb = rnd(xn) @ rnd(w.double()).T + b.double()
        out[name] = (a, bb)
    return out


def restate_loop_tables(sd, cfg, tabs):
    """q0_32 [d], sctab [L*10][H], vtab [L*10][d] in float64, and next to each value the sum of the absolute values of the terms of its dot products."""
    d, H = cfg.d_model, cfg.h
    g, nb = _t(sd[f"{BL}.sublayer.0.norm.a_2"]), _t(sd[f"{BL}.sublayer.0.norm.b_2"])
    W = [_t(sd[f"{BL}.self_attn.linears.{i}.weight"]).double() for i in range(3)]
    B = [_t(sd[f"{BL}.self_attn.linears.{i}.bias"]).double() for i in range(3)]
    xn0 = layer_norm64(_t(tabs["x0"])[None], g, nb)
    xn = layer_norm64(_t(tabs["xt"]), g, nb)
    q0, q0_abs = (xn0 @ W[0].T + B[0])[0], (xn0.abs() @ W[0].abs().T + B[0].abs())[0]
    k, k_abs = xn @ W[1].T + B[1], xn.abs() @ W[1].abs().T + B[1].abs()
    v, v_abs = xn @ W[2].T + B[2], xn.abs() @ W[2].abs().T + B[2].abs()
    sc = (q0[None] * k).reshape(-1, H, d // H).sum(-1) / 8.0
    sc_abs = (q0_abs[None] * k_abs).reshape(-1, H, d // H).sum(-1) / 8.0       # an error of q0 or of k enters through the other's magnitude: bounded by the product of the two sums
    return dict(q0_32=(q0, q0_abs), sctab=(sc, sc_abs), vtab=(v, v_abs))


@functools.lru_cache(maxsize=None)
def restatement(cfg_name, dt, seed):
    from boficap_amd import weights as W
    cfg, bf16 = _configs()[cfg_name], dt == "bf16"
    sd = W.make_state_dict(cfg, seed, bound_preset=False)
    pe = sd["model.pos_embed.pe"][0]          # (a buffer, the same in every state dict: refreshes do not carry it)
    exp = {"sd": sd, "lins": {}}
    for l in lin_table(cfg, bf16):
        exp["lins"][l] = restate_lin(sd, l, bf16)
    exp["tabs"], exp["xt_fused"] = restate_input_tables(sd, cfg, pe)
    exp["w1t"], exp["b1"], exp["w1p"] = restate_w1(sd, cfg, bf16)
    exp["gemm"] = restate_gemm_tables(sd, cfg, bf16, exp["tabs"])
    if _loop_config(cfg, bf16):
        exp["loop"] = restate_loop_tables(sd, cfg, exp["tabs"])
    return exp


# ------------------------------------------------------------------------------------------------------------------------------
# reading the engine back
def _read(eng, name, numel, dtype):
    from boficap_amd import hip as H
    t = torch.empty(numel, dtype=dtype, device="cuda")
    H.check(H.lib().bofi_engine_debug_copy(eng._h, name.encode(), H.ptr(t), t.numel() * t.element_size(), H.stream_ptr()), name)
    return t


def read_all(eng, cfg, bf16):
    cd = torch.bfloat16 if bf16 else torch.float32
    d, hh, H, rows = cfg.d_model, cfg.head_hidden, cfg.h, (cfg.seq_length + 2) * 10
    got = {}
    for l in lin_table(cfg, bf16):
        got[l.name("w")] = _read(eng, l.name("w"), l.Npad * l.K, cd)
        got[l.name("b")] = _read(eng, l.name("b"), l.Npad, torch.float32)
        if l.fold:
            got[l.name("cs")] = _read(eng, l.name("cs"), l.Npad, torch.float32)
        if has_wp(l, bf16):
            got[l.name("wp")] = _read(eng, l.name("wp"), l.Npad * l.K, torch.bfloat16)
        if l.f16:
            got[l.name("wp16")] = _read(eng, l.name("wp16"), l.Npad * l.K, torch.float16)
    for p in norm_table(cfg):
        got["g@" + p] = _read(eng, "g@" + p, d, torch.float32)
        got["nb@" + p] = _read(eng, "nb@" + p, d, torch.float32)
    for name, n, dtp in (("xt", rows * d, torch.float32), ("x0", d, torch.float32), ("x0_sa", d, torch.float32), ("x0b", d, torch.float32),
                         ("kvtab", rows * 2 * d, cd), ("q0", d, cd), ("q0_sa", d, cd), ("votab", rows * H * d, cd),
                         ("w1p", d * 2 * hh, cd), ("w1t", d * 2 * hh, torch.float32), ("b1", 2 * hh, torch.float32),
                         ("len_w2", 20 * hh, torch.float32), ("len_b2", 20, torch.float32), ("syn_w2", 10 * hh, torch.float32), ("syn_b2", 10, torch.float32)):
        got[name] = _read(eng, name, n, dtp)
    if _loop_config(cfg, bf16):
        got["q0_32"] = _read(eng, "q0_32", d, torch.float32)
        got["sctab"] = _read(eng, "sctab", rows * H, torch.float32)
        got["vtab"] = _read(eng, "vtab", rows * d, torch.float32)
        got["wsat"] = _read(eng, "wsat", 1, torch.int32)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in got.items()}


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}_{c[1]}")
def packed(request):
    """One engine per case, read back at four stages: [0] load_state_dict(A), [1] refresh_from_device(B), [2] refresh_from_device(A) from other tensors,
    [3] refresh_from_device of stage 2's tensors overwritten in place with B (same addresses: the cached descriptor tables)."""
    from boficap_amd import hip
    from boficap_amd.engine import BofiEngine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    hip.lib()
    cfg_name, dt = request.param
    cfg, bf16 = _configs()[cfg_name], dt == "bf16"
    ea, eb = restatement(cfg_name, dt, SEED_A), restatement(cfg_name, dt, SEED_B)
    eng = BofiEngine(cfg, torch.bfloat16 if bf16 else torch.float32, max_batch=4, max_regions=8)
    eng.load_state_dict(ea["sd"])
    stages = [read_all(eng, cfg, bf16)]
    dev_b = {k: torch.from_numpy(v).cuda().contiguous() for k, v in eb["sd"].items()}
    eng.refresh_from_device(dev_b)
    stages.append(read_all(eng, cfg, bf16))
    dev_a = {k: torch.from_numpy(v).cuda().contiguous() for k, v in ea["sd"].items()}      # (dev_b is still alive: other addresses)
    eng.refresh_from_device(dev_a)
    stages.append(read_all(eng, cfg, bf16))
    for k, v in dev_a.items():
        v.copy_(dev_b[k])
    eng.refresh_from_device(dev_a)
    stages.append(read_all(eng, cfg, bf16))
    torch.cuda.synchronize()
    return dict(name=f"{cfg_name}_{dt}", cfg=cfg, bf16=bf16, eng=eng, stages=stages, exp=[ea, eb])


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same_bits(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and torch.equal(_bits(got), _bits(want))


def _ulps(a, b):
    """distance of two float32 arrays in units of the last place (ordered-integer view)."""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def _half_ulp(x, bf16):
    """half a unit of the last place of the output type at magnitude x (8 / 24 significand bits)."""
    e = np.floor(np.log2(np.maximum(np.abs(x), 1e-30)))
    return np.exp2(e - (8 if bf16 else 24))


# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stage", [0, 1])
def test_every_linear_equals_the_restatement(packed, stage):
    """w: the float32 product w * gain (or w), rounded once to the compute dtype, stacked in recipe order, rows N .. Npad zero.  cs: the float32 of the exact
    sum of the weight as stored -- the double sum of at most 2048 such values is exact far beyond float32, so one ulp is a finding.  b: the bias, plus -- with a
    fold -- sum_k b_ln[k] w[n][k] of the UNSCALED weight, within 1 ulp (products exact in double, the summation order differs: a rounding tie).  wp: the
    fragment-major permutation of the read-back w, whole tensor.  wp16: the same permutation of fp16(clamp(w * gain)), product in float32."""
    cfg, bf16, got, exp = packed["cfg"], packed["bf16"], packed["stages"][stage], packed["exp"][stage]
    bad = []
    padded = 0
    for l in lin_table(cfg, bf16):
        w, b, cs, w16 = exp["lins"][l]
        gw = got[l.name("w")].reshape(l.Npad, l.K)
        if not _same_bits(gw, w):
            rows_off = (_bits(gw) != _bits(w)).any(1).nonzero().flatten()
            bad.append(f"{l.name('w')}: {len(rows_off)} of {l.Npad} rows differ, first {int(rows_off[0])}")
        gb = got[l.name("b")]
        if l.fold:
            u = _ulps(gb.numpy(), b.numpy())
            if u.max() > 1:
                bad.append(f"{l.name('b')}: {int((u > 1).sum())} rows more than 1 ulp off, worst {int(u.max())} ulp at row {int(u.argmax())}")
            gcs = got[l.name("cs")]
            if not _same_bits(gcs, cs):
                off = (_bits(gcs) != _bits(cs)).nonzero().flatten()
                bad.append(f"{l.name('cs')}: {len(off)} of {l.Npad} rows differ, first {int(off[0])}, worst {int(_ulps(gcs.numpy(), cs.numpy()).max())} ulp")
        elif not _same_bits(gb, b):
            bad.append(f"{l.name('b')}: the bias is not the parameter")
        if l.Npad > l.N:
            padded += 1
            assert not gw[l.N:].float().any() and not gb[l.N:].any() and (not l.fold or not got[l.name("cs")][l.N:].any()), l.name("w") + ": padding rows are not zero"
        if has_wp(l, bf16) and not _same_bits(got[l.name("wp")], frag_major(gw)):
            bad.append(f"{l.name('wp')}: not the fragment-major permutation of the packed weight")
        if l.f16:
            g16, e16 = got[l.name("wp16")], frag_major(w16)
            if not _same_bits(g16, e16):          # (fp16 subnormals included: the MI355X's conversion keeps them, measured -- nothing is flushed on either side)
                differ = _bits(g16) != _bits(e16)
                sub = e16.float().abs() < 2.0 ** -14
                bad.append(f"{l.name('wp16')}: {int(differ.sum())} elements differ, {int((differ & ~sub).sum())} of them at normal fp16 values")
    assert not bad, "\n".join(bad)
    assert padded >= (2 if _loop_config(cfg, bf16) else 1)          # the generator (pad_to 128) and, in the loop configuration, b_heads (pad_to 256)
    if _loop_config(cfg, bf16):
        assert int(got["wsat"][0]) == 0


@pytest.mark.parametrize("stage", [0, 1])
def test_norms_head_vectors_and_input_tables_are_bit_equal(packed, stage):
    cfg, bf16, got, exp = packed["cfg"], packed["bf16"], packed["stages"][stage], packed["exp"][stage]
    sd = exp["sd"]
    bad = []

    def same(name, want):
        want = want if torch.is_tensor(want) else _t(np.asarray(want))
        if not _same_bits(got[name], want.reshape(-1)):
            bad.append(name)

    for p in norm_table(cfg):
        same("g@" + p, sd[p + ".a_2"])
        same("nb@" + p, sd[p + ".b_2"])
    same("len_w2", sd[f"{LP}.Length_classifier2.weight"]); same("len_b2", sd[f"{LP}.Length_classifier2.bias"])
    same("syn_w2", sd[f"{LP}.Syntactic_classifier2.weight"]); same("syn_b2", sd[f"{LP}.Syntactic_classifier2.bias"])
    same("w1t", exp["w1t"]); same("b1", exp["b1"]); same("w1p", exp["w1p"])
    for k in ("xt", "x0", "x0_sa", "x0b"):          # float32(float32(lut * sqrt(d)) + pe): two roundings
        same(k, exp["tabs"][k])
    assert not bad, f"not bit-equal to the restatement: {bad}"


@pytest.mark.parametrize("stage", [0, 1])
def test_accumulated_tables_stay_under_their_derived_bars(packed, stage):
    from conftest import record_parity
    cfg, bf16, got, exp = packed["cfg"], packed["bf16"], packed["stages"][stage], packed["exp"][stage]
    d, H, rows = cfg.d_model, cfg.h, (cfg.seq_length + 2) * 10
    tag = f"repack_{packed['name']}_s{stage}"
    bad = []

    # votab[row][h][c] = sum_e wo[c][h*64 + e] V[row][h*64 + e] from the engine's own kvtab and packed W_o: float32 fmaf over 64 terms, one rounding to the output type
    wo_l = next(l for l in lin_table(cfg, bf16) if l.first == f"{BL}.self_attn.linears.3")
    wo = got[wo_l.name("w")].double().reshape(d, H, 64)
    V = got["kvtab"].double().reshape(rows, 2 * d)[:, d:].reshape(rows, H, 64)
    ref = torch.einsum("che,rhe->rhc", wo, V).numpy()
    mag = torch.einsum("che,rhe->rhc", wo.abs(), V.abs()).numpy()
    bar = 64 * 2.0 ** -24 * mag
    bar = bar + _half_ulp(np.abs(ref) + bar, bf16)
    err = np.abs(got["votab"].double().numpy().reshape(rows, H, d) - ref)
    worst = float((err / bar).max())
    record_parity(tag + "_votab", worst, 1.0, "largest |error| / bar; bar = 64 * 2^-24 * sum|wo v| + half an ulp of the output type")
    print(f"{tag} votab: worst error / bar = {worst:.3f}, max |error| = {err.max():.3e}")
    if not worst <= 1.0:
        bad.append(f"votab: error / bar = {worst:.3f}")

    # kvtab, q0, q0_sa: outputs of the engine's linear (LayerNorm kernel, then the GEMM on compute-dtype operands).  Bar: twice the largest distance between the
    # float64 restatement from the operands as they are and the one with LayerNorm output and weight rounded to the compute dtype (the size of the operand
    # rounding, doubled for the output rounding), each table's own; where it is 0 (float32) test_linear_f32's 2e-5 * sqrt(K).  Compared with the
    # rounded-operand restatement, which is what the kernel is given.
    for name, (a, b) in exp["gemm"].items():
        dist = float((a - b).abs().max())
        gbar = 2.0 * dist if dist > 0 else 2e-5 * math.sqrt(d)
        assert bf16 == (dist > 0)
        e = float((got[name].double().reshape(b.shape) - b).abs().max())
        record_parity(f"{tag}_{name}", e, gbar, "engine linear behind the bound tables vs float64 on rounded operands; bar from the two restatements alone")
        print(f"{tag} {name}: max |error| = {e:.3e}, bar = {gbar:.3e}")
        if not e <= gbar:
            bad.append(f"{name}: {e:.3e} > {gbar:.3e}")

    # the loop kernel's float32 tables: LayerNorm, three projections of K = d terms, a per-head dot product / 8.  Bar per element: K * 2^-24 * sum |terms|
    if _loop_config(cfg, bf16):
        for name, (val, mag) in exp["loop"].items():
            bar = d * 2.0 ** -24 * mag.numpy()
            err = np.abs(got[name].double().numpy().reshape(val.shape) - val.numpy())
            worst = float((err / bar).max())
            record_parity(f"{tag}_{name}", worst, 1.0, "largest |error| / bar; bar = K * 2^-24 * sum of |terms| per element")
            print(f"{tag} {name}: worst error / bar = {worst:.3f}, max |error| = {err.max():.3e}")
            if not worst <= 1.0:
                bad.append(f"{name}: error / bar = {worst:.3f}")
    else:
        assert "q0_32" not in got
    assert not bad, "\n".join(bad)


def test_refreshing_back_restores_every_bit(packed):
    """Stage 2 (first weight set again, from tensors at other addresses) against stage 0, stage 3 (second set written over stage 2's tensors: the descriptor
    tables are the cached ones) against stage 1: every read-back buffer, bit for bit."""
    s = packed["stages"]
    for a, b in ((0, 2), (1, 3)):
        assert s[a].keys() == s[b].keys()
        off = [k for k in s[a] if not _same_bits(s[a][k], s[b][k])]
        assert not off, f"stage {b} differs from stage {a} in {off}"
    differ = [k for k in s[0] if not _same_bits(s[0][k], s[1][k])]
    assert len(differ) >= len(s[0]) - 1, sorted(set(s[0]) - set(differ))          # (the two weight sets share nothing but wsat = 0: a refresh that did nothing would show)


@pytest.mark.parametrize("cfg_name,dt", [c for c in CASES if c[1] == "bf16"])
@pytest.mark.parametrize("seed", [SEED_A, SEED_B])
def test_restatement_tells_wrong_packings_apart(cfg_name, dt, seed):
    """Conditions on the INPUTS (no kernel output enters): the wrong variants a bit-equal comparison is meant to catch differ from the right ones on these weights."""
    cfg = _configs()[cfg_name]
    exp = restatement(cfg_name, dt, seed)
    sd = exp["sd"]
    gained16 = 0
    for l in lin_table(cfg, True):
        if not l.fold:
            continue
        W = torch.cat([_t(sd[p + ".weight"]) for p in l.prefixes], 0)
        b = torch.cat([_t(sd[p + ".bias"]) for p in l.prefixes], 0)
        gain, bln = _t(sd[l.fold + ".a_2"]), _t(sd[l.fold + ".b_2"])
        prod = W * gain[None, :]
        _, c, cs, w16 = exp["lins"][l]
        cs_unrounded = prod.double().sum(1).float()
        assert (_bits(cs_unrounded) != _bits(cs[:l.N])).float().mean() >= 0.5, l.name("cs")
        c_scaled = (b.double() + (prod.double() * bln.double()[None, :]).sum(1)).float()
        assert (_ulps(c_scaled.numpy(), c[:l.N].numpy()) > 1).mean() >= 0.5, l.name("b")
        if l.f16:
            gained16 += 1
            assert (_bits(W.to(torch.float16)) != _bits(w16[:l.N])).float().mean() >= 0.5, l.name("wp16")
    assert gained16 == (3 if _loop_config(cfg, True) else 0)
    assert (exp["xt_fused"].view(np.int32) != exp["tabs"]["xt"].view(np.int32)).any()
    if cfg.N_dec == 8:          # the second kv_all entry starts at row 16 * d: its rows are not a copy of the first entry's
        l = next(l for l in lin_table(cfg, True) if len(l.prefixes) == 18)
        w = exp["lins"][l][0]
        assert not torch.equal(w[:2 * cfg.d_model], w[16 * cfg.d_model:])


def test_readback_refuses_what_the_engine_does_not_hold(packed):
    from boficap_amd import hip as H
    cfg, bf16, eng = packed["cfg"], packed["bf16"], packed["eng"]
    d = cfg.d_model
    buf = torch.zeros(4 * d * d + 64, dtype=torch.float32, device="cuda")

    def rc(name, nbytes):
        return H.lib().bofi_engine_debug_copy(eng._h, name.encode(), H.ptr(buf), nbytes, H.stream_ptr())

    plain = f"{BL}.self_attn.linears.1"          # t_kvself: no fold; "#1" is b_kv_self with sublayer.0.norm folded in
    assert rc(f"w@{plain}", 16) == 0 and rc(f"cs@{plain}#1", 2 * d * 4) == 0
    assert rc(f"cs@{plain}", 16) != 0                                    # a field the Linear does not have
    assert rc(f"w@{plain}#2", 16) != 0 and rc(f"w@{plain}#x", 16) != 0 and rc("w@no.such.linear", 16) != 0 and rc(f"v@{plain}", 16) != 0
    assert rc(f"cs@{plain}#1", 2 * d * 4 + 4) != 0 and rc("x0", d * 4 + 4) != 0 and rc(f"g@{BL}.sublayer.0.norm", d * 4 + 4) != 0      # more than the buffer holds
    assert rc(f"g@{BL}.sublayer.0.norm", d * 4) == 0 and rc("g@no.such.norm", 4) != 0
    assert (rc("q0_32", 4) == 0) == _loop_config(cfg, bf16) and (rc(f"wp16@{BL}.ff.w_2", 16) == 0) == _loop_config(cfg, bf16)
    assert (rc("wp@model.generator.proj", 16) == 0) == bf16 and rc("wp@att_embed.0", 16) != 0
    assert rc("counters", 32) == 0 and rc("nothing", 4) != 0             # today's names keep their behaviour
    torch.cuda.synchronize()
