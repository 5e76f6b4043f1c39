"""The forward GEMM family (csrc/gemm_glds.hip, gemm_pers.hip, gemm.hip, gemm_tn.hip) through its C entries, at the smallest shapes that
reach each tile, feature set, epilogue path and tile order of the dispatch (launch_glds_t, launch_gemm_pers, launch_tiles,
launch_gemm_tn*).  Every reference is plain torch on the CPU in float64.  Two kinds of case:

  exact probes    operands in {-1, 0, 1} (exact in bf16), bias and residual small integers: every partial sum is an integer far below
                  2^24, so the result is the same in any summation order and the kernel must EQUAL the float64 product.  The residual
                  differs from row to row and column to column, so a misplaced, lost or doubled tile shows whatever the tolerance.  Where
                  the output, its bf16 copy or the row statistics must be exact too, x holds at most 64 non-zeros per row and the residual
                  stays below 61: |result| <= 256, exact in bf16, and a 32-column sum of squares stays below 2^22.
  random values   float64 on the bf16-rounded operands, held to the bars tests/test_gpu_kernels.py uses for the same operator:
                  2e-5 sqrt(K) (float32), 1e-4 sqrt(K) (bf16 operands, float32 out), 1e-2 scale (bf16 out), 2e-5 * 8 * scale (LayerNorm
                  fold), rtol 1e-4 / atol 1e-3 (row statistics).  The LayerNorm fold has no exact probe (1 / (std + eps) is not exact).

Every output buffer is prefilled with a sentinel and has a pitch wider than N in at least one case per epilogue path: nothing outside
[M, N] (or, for a row list, outside the listed rows) may change.  Which kernel a shape reaches follows from the rules quoted at each
table; a test cannot observe it, so each shape names the rule and the edge it is there for.  Knobs are set through the ``knobs`` fixture,
which restores the environment and reloads it whatever the test does."""
import ctypes as C
import math

import pytest
import torch

import counter_streams as cs

pytestmark = pytest.mark.gpu

SENT = -8192.0                      # exact in float32 and bf16; no test value comes near it
BF, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def H():
    from boficap_amd import hip
    assert torch.cuda.is_available(), "these tests need the MI355X"
    hip.lib()
    return hip


@pytest.fixture
def knobs(H, monkeypatch):
    """set(BOFI_X=value | None, ...): puts the knobs into the environment (None: removes one) and has the library read them again.
    On the way out -- passed or failed -- the environment is restored and read once more: the next test sees the defaults."""
    def set_knobs(**kw):
        for k, v in kw.items():
            if v is None:
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, str(v))
        H.lib().bofi_reload_env()
    try:
        yield set_knobs
    finally:
        monkeypatch.undo()
        H.lib().bofi_reload_env()


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16) if t.dtype == BF else (t.view(torch.int32) if t.dtype == F32 else t)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _tern(g, rows, cols, nnz=None):
    """{-1, 0, 1}, at most ``nnz`` non-zeros per row"""
    t = torch.randint(-1, 2, (rows, cols), generator=g).float()
    if nnz is not None and cols > nnz:
        rank = torch.rand(rows, cols, generator=g).argsort(1).argsort(1)
        t = t * (rank < nnz)
    return t


def _row_stats(v, groups):
    """partial (sum, sum of squares) per row and column group, as the producers write them: [M][groups][2]"""
    M, d = v.shape
    v = v.view(M, groups, d // groups)
    return torch.stack([v.sum(-1), (v * v).sum(-1)], -1).contiguous()


RPG = 7                              # rows per group of the row_len cases: odd, so groups straddle every tile edge


def _row_keep(M):
    lens = torch.tensor([(i * 3 + 2) % (RPG + 1) for i in range((M + RPG - 1) // RPG)], dtype=torch.int32)
    m = torch.arange(M)
    return lens, (m % RPG) < lens[m // RPG]


def _linear(H, M, N, K, *, dt="bf16", ydt=F32, bias=True, bias_off=0, res="full", ldr_pad=0, ldy_pad=0, relu=0, row_len=False, drop=None,
            y2=False, stats=False, ln=0, rows=None, mask=False, ex=False, exact=True, seed=0):
    """One call of the bofi_linear family on operands made from (shape, seed) alone, and its float64 reference.
    dt: "bf16" / "f32" (x and w alike) or "mixed" (float32 x, bf16 w: the register-staged kernel).  res: "full" / "bcast" (ldr = 0) / None.
    drop: None, or the dropout step (0: no device word) at p = 0.5, seed 4711.  ln: statistic groups of the folded LayerNorm (0: none).
    rows: length of the row list (bofi_linear_rows), None: dense.  mask: bofi_linear_masked with scale 2.
    Returns dict(rc; y, y2, st: the whole padded buffers; ref: float64 [M, N]; listed: the rows of the row list, or None)."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * M + 31 * N + K)
    small = ydt == BF or y2 or stats or mask
    xdt = F32 if dt in ("f32", "mixed") else BF
    wdt = F32 if dt == "f32" else BF
    x32 = None
    if exact:
        x, w = _tern(g, M, K, 64 if small else None), _tern(g, N, K)
        b = torch.randint(-4, 5, (N,), generator=g).float() if bias else None
        mm, nn = torch.arange(M)[:, None], torch.arange(N)[None, :]
        r = ((mm * 5 + nn * 3) % 61).float() if small else (mm * 4 + nn % 4).float()
    else:
        x32 = torch.randn(M, K, generator=g) * (1.5 if ln else 1.0) + (0.2 if ln else 0.0)
        x = x32 if dt == "f32" else x32.to(BF).float()
        w = torch.randn(N, K, generator=g) / math.sqrt(K)
        w = w if dt == "f32" else w.to(BF).float()
        b = torch.randn(N, generator=g) * (0.1 if ln else 1.0) if bias else None
        r = torch.randn(M, N, generator=g)
    if res == "bcast":
        r = r[M // 2:M // 2 + 1].clone()
    if mask:
        r = torch.randint(-1, 2, (M, N), generator=g).float() * 0.5            # a third each: negative, exactly 0, positive
        assert bool((r == 0).any()) and bool((r < 0).any())
    ldy, ldr = N + ldy_pad, (0 if res == "bcast" else N + ldr_pad)
    xd, wd = x.to(xdt).cuda(), w.to(wdt).cuda()
    bd = None
    if b is not None:
        bbuf = torch.zeros(N + 4, device="cuda")
        bd = bbuf[bias_off:bias_off + N]
        bd.copy_(b)
    rd = None
    if res is not None or mask:
        rd = torch.full((r.shape[0], max(ldr, N)), SENT, device="cuda")
        rd[:, :N] = r.cuda()
    y = torch.full((M, ldy), SENT, dtype=ydt, device="cuda")
    y2d = torch.full((M, N + 8), SENT, dtype=wdt, device="cuda") if y2 else None
    st = torch.full((M, N // 32, 2), SENT, device="cuda") if stats else None
    lens, keep_len = _row_keep(M)
    lens_d = lens.cuda() if row_len else None
    step_d = torch.tensor([drop], dtype=torch.int64, device="cuda") if drop else None
    code = lambda d: H.DT_F32 if d == F32 else H.DT_BF16
    lib, P, S = H.lib(), H.ptr, H.stream_ptr()
    head = (P(xd), code(xdt), K, P(wd), code(wdt))
    out = (P(y), code(ydt), ldy, M, N, K)
    acc = x.double() @ w.double().t()
    listed = None
    if mask:
        rc = lib.bofi_linear_masked(*head, P(rd), ldr, 2.0, *out, S)
        ref = torch.where(r > 0, acc * 2.0, torch.zeros(()).double())
    else:
        v = acc
        stats_d = colsum_d = None
        if ln:
            mean, rstd = x32.double().mean(1, keepdim=True), 1.0 / (x32.double().std(1, keepdim=True) + 1e-6)
            colsum = w.double().sum(1)
            v = rstd * (acc - mean * colsum)
            stats_d, colsum_d = _row_stats(x32, ln).cuda(), colsum.float().cuda()
        if b is not None:
            v = v + b.double()
        if relu:
            v = torch.relu(v)
        if row_len:
            v = v * keep_len[:, None]
        if drop is not None:
            keep = torch.from_numpy(cs.keep_mask(4711, drop, 0.5, cs.linear_ids(M, N)))
            assert 0.3 < float(keep.float().mean()) < 0.7 or M * N < 64
            v = torch.where(keep, v * 2.0, torch.zeros(()).double())
        ref = v + r.double() if res is not None else v
        if rows is not None:
            order = torch.randperm(M, generator=g)[:rows].to(torch.int32)
            idx = torch.zeros(M, dtype=torch.int32)
            idx[:rows] = order
            idx_d, cnt = idx.cuda(), torch.tensor([rows], dtype=torch.int32, device="cuda")
            listed = torch.zeros(M, dtype=torch.bool)
            listed[order.long()] = True
            rc = lib.bofi_linear_rows(*head, P(bd), P(rd), ldr, *out, relu, P(idx_d), P(cnt), S)
        elif ln or stats:
            assert dt == "bf16"
            rc = lib.bofi_linear_fused(P(xd), K, P(wd), P(bd), P(rd), ldr, P(y), code(ydt), ldy, P(y2d), N + 8, P(stats_d), P(colsum_d),
                                       0 if ln == K // 32 else ln, P(st), M, N, K, relu, S)
        elif drop is not None or y2 or ex:
            rc = lib.bofi_linear_ex(*head, P(bd), P(rd), ldr, *out, relu, P(lens_d), RPG, 0.5 if drop is not None else 0.0, 4711, P(step_d),
                                    P(y2d), N + 8, S)
        else:
            rc = lib.bofi_linear(*head, P(bd), P(rd), ldr, *out, relu, P(lens_d), RPG, S)
    torch.cuda.synchronize()
    return dict(rc=rc, y=y, y2=y2d, st=st, ref=ref, listed=listed, M=M, N=N, K=K, dt=dt, ln=ln, exact=exact)


def _check(o, what=""):
    """The call was accepted; outputs meet the reference (exactly, or within the operator's bar); the sentinel outside [M, N] is intact."""
    assert o["rc"] == 0, f"{what}: status {o['rc']}"
    M, N, K, ref = o["M"], o["N"], o["K"], o["ref"]
    live = o["listed"] if o["listed"] is not None else torch.ones(M, dtype=torch.bool)
    scale = max(1.0, float(ref.abs().max()))
    for name in ("y", "y2"):
        t = o[name]
        if t is None:
            continue
        got = t.cpu()
        assert bool((got[:, N:].float() == SENT).all()), f"{what}: {name} written beyond column N"
        assert bool((got[~live].float() == SENT).all()), f"{what}: {name} written at a row that is not listed"
        val = got[live][:, :N].double()
        assert bool(torch.isfinite(val).all()), f"{what}: {name} not finite"
        if o["exact"]:
            if t.dtype == BF:
                assert float(ref.abs().max()) <= 256, "the probe's reference is not exact in bf16"
            assert float(ref.abs().max()) < 2 ** 24 and torch.equal(ref, ref.round())
            bad = (val != ref[live]).nonzero()
            assert bad.numel() == 0, f"{what}: {name} differs from the exact product at {bad.shape[0]} elements, first (row, col) {bad[0].tolist()}"
        else:
            err = float((val - ref[live]).abs().max())
            if t.dtype == BF:
                bar = 1e-2 * scale
            elif o["ln"]:
                bar = 2e-5 * 8 * scale
            else:
                bar = (2e-5 if o["dt"] == "f32" else 1e-4) * math.sqrt(K)
            print(f"{what} {name}: max err {err:.3e} (bar {bar:.3e})")
            assert err <= bar, f"{what}: {name} err {err:.3e} > {bar:.3e}"
    if o["st"] is not None:
        st = o["st"].cpu()
        if o["exact"]:
            assert torch.equal(st[live].double(), _row_stats(ref, N // 32)[live]), f"{what}: row statistics differ from the exact sums"
        else:
            assert o["y"].dtype == F32
            assert torch.allclose(st[live], _row_stats(o["y"].cpu()[:, :N].contiguous(), N // 32)[live], rtol=1e-4, atol=1e-3), f"{what}: row statistics"
        assert bool((st[~live] == SENT).all())


def _equal_outputs(a, b, what):
    for name in ("y", "y2", "st"):
        if a[name] is not None:
            assert _same_bits(a[name], b[name]), f"{what}: {name} is not bit-equal"


# ================================================================================================ (a) one tile per workgroup: tiles and edges
# launch_glds_t:  M <= 64 -> 64x32x4;  bf16, K <= 512 and a specialised feature set -> 64x32x9, or 64x16x9 when the vector epilogue runs,
#                 N % 16 == 0 and there are no statistics / y2.   M > 64 -> 64x64x2 below 200 tiles of 128x64 (64x64x4: bf16, K >= 1024,
#                 feature sets 0, 1, 2, 6), 128x64x2 from 200 tiles on.
# vector epilogue: N % 4 == 0, ldy % 4 == 0, ldr % 4 == 0, y / bias / residual 16-byte aligned; anything else: one float per lane.
TILE_CASES = [
    # ---- 64x32x4 (4 waves)
    ("64x32x4 f32 M=1 N=33: scalar, lanes 32-63 idle, last column tile of 1", dict(M=1, N=33, K=32, dt="f32")),
    ("64x32x4 f32 M=63 N=60: vector, last column tile BN-4, pitch > N", dict(M=63, N=60, K=96, dt="f32", ldy_pad=4, relu=1)),
    ("64x32x4 f32 M=64 N=64: scalar by ldy % 4 != 0", dict(M=64, N=64, K=32, dt="f32", ldy_pad=1)),
    ("64x32x4 f32 M=50: scalar by a bias pointer off by one float", dict(M=50, N=40, K=64, dt="f32", bias_off=1, relu=1, row_len=True)),
    ("64x32x4 f32 M=33: scalar by ldr % 4 != 0, dropout", dict(M=33, N=36, K=32, dt="f32", ldr_pad=3, drop=0)),
    ("64x32x4 f32 M=64: vector, broadcast residual (ldr = 0)", dict(M=64, N=96, K=64, dt="f32", res="bcast")),
    ("64x32x4 bf16 K=576 > 512: vector, bf16 out, pitch > N", dict(M=64, N=96, K=576, ydt=BF, ldy_pad=8)),
    ("64x32x4 bf16 K=1024 N=34: scalar + relu + row_len + dropout", dict(M=37, N=34, K=1024, relu=1, row_len=True, drop=3)),
    ("64x32x4 bf16 K=2048 M=1: 32 slabs through a 4-slot ring", dict(M=1, N=32, K=2048, res=None)),
    # ---- 64x32x9 (bf16, K <= 512, specialised feature sets; statistics / y2, N % 16 != 0, or the scalar epilogue)
    ("64x32x9 feat 2 M=64 N=64 K=512: residual + statistics + bf16 copy", dict(M=64, N=64, K=512, stats=True, y2=True)),
    ("64x32x9 feat 2 M=1 N=32 K=64: one slab in nine slots", dict(M=1, N=32, K=64, stats=True, y2=True, ydt=BF, res=None)),
    ("64x32x9 feat 0 M=63 N=60 K=64: vector, N % 16 != 0, last tile BN-4", dict(M=63, N=60, K=64, ldy_pad=4)),
    ("64x32x9 feat 0 M=64 N=33 K=512: scalar, bf16 out, relu", dict(M=64, N=33, K=512, ydt=BF, relu=1, ldy_pad=2)),
    ("64x32x9 feat 0 N=48: N % 16 == 0 but ldy % 4 != 0 -> scalar", dict(M=40, N=48, K=128, ldy_pad=3)),
    ("64x32x9 feat 0 N=48: bias off by one float, broadcast residual", dict(M=64, N=48, K=192, bias_off=1, res="bcast")),
    ("64x32x9 feat 8 N=40: dropout, vector", dict(M=64, N=40, K=128, drop=0, relu=1)),
    ("64x32x9 feat 8 N=33: dropout + relu, scalar, ldr % 4 != 0", dict(M=63, N=33, K=64, drop=2, relu=1, ldr_pad=1)),
    ("64x32x9 feat 10 M=17 N=32: dropout + bf16 copy", dict(M=17, N=32, K=128, drop=0, y2=True)),
    ("64x32x9 feat 32 N=20: masked", dict(M=64, N=20, K=64, mask=True, ydt=BF)),
    # ---- 64x16x9 (2 waves: vector epilogue, N % 16 == 0, no statistics)
    ("64x16x9 M=1 N=16 K=64: one slab, one tile", dict(M=1, N=16, K=64)),
    ("64x16x9 M=64 N=48 K=512: eight slabs, bf16 out, pitch > N", dict(M=64, N=48, K=512, ydt=BF, ldy_pad=8, relu=1)),
    ("64x16x9 M=63 N=80 K=256: broadcast residual", dict(M=63, N=80, K=256, res="bcast")),
    ("64x16x9 feat 8 N=32: dropout with a device step word", dict(M=33, N=32, K=128, drop=5)),
    ("64x16x9 feat 32 N=32: masked", dict(M=64, N=32, K=512, mask=True)),
    # ---- 64x64x2 (8 waves)
    ("64x64x2 f32 M=65 N=65: scalar, ragged last row tile of 1, last column tile of 1", dict(M=65, N=65, K=32, dt="f32")),
    ("64x64x2 bf16 M=130 N=124: vector, last tile BN-4, bf16 out, pitch > N", dict(M=130, N=124, K=128, ydt=BF, ldy_pad=4)),
    ("64x64x2 f32 M=100 N=70: scalar by ldy % 4, relu + row_len + dropout", dict(M=100, N=70, K=64, dt="f32", ldy_pad=1, relu=1, row_len=True, drop=0)),
    ("64x64x2 bf16 M=65: scalar by bias off by one float, ldr % 4 != 0", dict(M=65, N=64, K=512, bias_off=1, ldr_pad=2)),
    ("64x64x2 bf16 M=129: broadcast residual, relu", dict(M=129, N=128, K=64, res="bcast", relu=1)),
    ("64x64x2 feat 2 M=65 N=96: statistics + bf16 copy", dict(M=65, N=96, K=256, stats=True, y2=True)),
    ("64x64x2 feat 4 bf16 M=65: row_len (generic kernel)", dict(M=65, N=64, K=128, row_len=True, relu=1)),
    ("64x64x2 feat 8 M=70 N=68: dropout, vector", dict(M=70, N=68, K=64, drop=1)),
    ("64x64x2 feat 10 M=70 N=64: dropout + bf16 copy", dict(M=70, N=64, K=128, drop=0, y2=True, relu=1)),
    ("64x64x2 feat 12 M=65: dropout + row_len (generic kernel)", dict(M=65, N=96, K=64, drop=0, row_len=True)),
    ("64x64x2 feat 32 M=65 N=68: masked, bf16 out", dict(M=65, N=68, K=128, mask=True, ydt=BF, ldy_pad=4)),
    # ---- 64x64x4 (bf16, K >= 1024)
    ("64x64x4 feat 0 M=65 N=124 K=1024: vector", dict(M=65, N=124, K=1024, ldy_pad=4)),
    ("64x64x4 feat 0 M=129 N=65 K=1088: scalar, 17 slabs", dict(M=129, N=65, K=1088, relu=1, ydt=BF)),
    ("64x64x4 feat 2 M=70 N=64 K=1024: statistics + bf16 copy", dict(M=70, N=64, K=1024, stats=True, y2=True)),
    ("64x64x4 feat 6 M=70 N=64 K=1024: row_len + bf16 copy (generic kernel)", dict(M=70, N=64, K=1024, row_len=True, y2=True)),
    # ---- 128x64x2: at least 200 tiles of 128x64 (10 x 20); M = 1275 leaves a last row tile of 123
    ("128x64x2 f32 M=1275 N=1276 K=32: vector, last column tile BN-4", dict(M=1275, N=1276, K=32, dt="f32", ldy_pad=4)),
    ("128x64x2 bf16 M=1275 N=1217 K=64: scalar, last column tile of 1, bf16 out", dict(M=1275, N=1217, K=64, ydt=BF, relu=1, ldy_pad=1)),
    ("128x64x2 bf16 M=1275 N=1280 K=64: row_len (generic kernel), broadcast residual", dict(M=1275, N=1280, K=64, row_len=True, res="bcast")),
    ("128x64x2 feat 2 M=1275 N=1280 K=64: statistics + bf16 copy", dict(M=1275, N=1280, K=64, stats=True, y2=True)),
    ("128x64x2 feat 8 f32 M=1153 N=1280 K=32: dropout, last row tile of 1", dict(M=1153, N=1280, K=32, dt="f32", drop=0)),
    ("128x64x2 feat 10 M=1275 N=1280 K=64: dropout + bf16 copy", dict(M=1275, N=1280, K=64, drop=2, y2=True)),
    ("128x64x2 feat 32 M=1275 N=1280 K=64: masked, bf16 out", dict(M=1275, N=1280, K=64, mask=True, ydt=BF)),
    # ---- float32 operands on the feature sets the bf16 cases above leave to them
    ("64x32x4 f32 feat 32 M=64 N=36: masked", dict(M=64, N=36, K=32, dt="f32", mask=True)),
    ("64x32x4 f32 feat 10 M=50 N=32: dropout + float32 copy", dict(M=50, N=32, K=64, dt="f32", drop=0, y2=True)),
    ("64x64x2 f32 feat 10 M=70 N=64: dropout + float32 copy", dict(M=70, N=64, K=32, dt="f32", drop=1, y2=True, relu=1)),
    ("64x64x2 f32 feat 32 M=65 N=68: masked", dict(M=65, N=68, K=64, dt="f32", mask=True, ldy_pad=4)),
    ("128x64x2 f32 feat 32 M=1275 N=1280 K=32: masked", dict(M=1275, N=1280, K=32, dt="f32", mask=True)),
]


@pytest.mark.parametrize("what,kw", TILE_CASES, ids=[f"{i:02d} " + c[0].split(":")[0] for i, c in enumerate(TILE_CASES)])
def test_one_tile_kernel_exact_on_every_tile_and_edge(H, what, kw):
    _check(_linear(H, **kw), what)


# rows (feature set 64): the grid is sized for the capacity, the count is read on the device; unlisted rows keep the sentinel
ROW_LIST_CASES = [
    ("64x32x4 f32 capacity 60, 37 rows, scalar", dict(M=60, N=33, K=32, dt="f32", rows=37)),
    ("64x64x2 bf16 capacity 200, 70 rows: two of four row tiles run", dict(M=200, N=124, K=128, rows=70, ldy_pad=4, relu=1)),
    ("64x64x2 bf16 capacity 65, no rows", dict(M=65, N=64, K=64, rows=0)),
    ("64x64x2 f32 capacity 130, all rows, bf16-free", dict(M=130, N=70, K=64, dt="f32", rows=130)),
    ("128x64x2 bf16 capacity 1275, 300 rows", dict(M=1275, N=1280, K=64, rows=300, ydt=BF)),
]


@pytest.mark.parametrize("what,kw", ROW_LIST_CASES, ids=[c[0] for c in ROW_LIST_CASES])
def test_one_tile_kernel_over_a_row_list(H, what, kw):
    _check(_linear(H, **kw), what)


# The folded LayerNorm (feature sets 1 and 3): 16 statistic groups take the tree sum, any other count the loop (gemm_glds.hip, the two
# branches on np4); random values, the fold's bar.  K = 512 with 16 groups = 32-column groups of d_model, with 32 groups 16-column groups.
LN_CASES = [
    ("64x16x9 feat 1 M=64 N=64 K=512, 16 groups", dict(M=64, N=64, K=512, ln=16, ydt=BF, relu=1)),
    ("64x16x9 feat 1 M=37 N=64 K=512, 32 groups", dict(M=37, N=64, K=512, ln=32, res="full")),
    ("64x32x9 feat 1 M=63 N=36 K=256, 8 groups: N % 16 != 0", dict(M=63, N=36, K=256, ln=8, res=None)),
    ("64x32x4 feat 3 M=64 N=64 K=512, 16 groups: LayerNorm in, statistics out (refused before)", dict(M=64, N=64, K=512, ln=16, stats=True, y2=True)),
    ("64x64x2 feat 3 M=65 N=64 K=512, 32 groups", dict(M=65, N=64, K=512, ln=32, stats=True, y2=True)),
    ("64x64x2 feat 1 M=130 N=124 K=512, 16 groups", dict(M=130, N=124, K=512, ln=16, res=None, relu=1, ldy_pad=4)),
    ("64x64x4 feat 1 M=70 N=64 K=1024, 32 groups", dict(M=70, N=64, K=1024, ln=32, res=None)),
    ("64x64x4 feat 1 M=70 N=64 K=1024, 16 groups", dict(M=70, N=64, K=1024, ln=16, ydt=BF, res=None)),
    ("128x64x2 feat 1 M=1275 N=1280 K=64, 16 groups of 4 columns", dict(M=1275, N=1280, K=64, ln=16, res=None)),
]


@pytest.mark.parametrize("what,kw", LN_CASES, ids=[c[0].split(":")[0] for c in LN_CASES])
def test_one_tile_kernel_folded_layernorm(H, knobs, what, kw):
    knobs(BOFI_GEMM_PERS=0)                                     # (M = 1275 x N = 1280 is 50 tiles of 256 x 128: not persistent anyway)
    _check(_linear(H, exact=False, **kw), what)


RANDOM_CASES = [
    ("64x32x4 f32", dict(M=63, N=33, K=96, dt="f32", relu=1)),
    ("64x16x9 bf16", dict(M=64, N=48, K=512)),
    ("64x32x9 bf16, bf16 out", dict(M=50, N=36, K=256, ydt=BF, relu=1, res=None)),
    ("64x64x2 f32", dict(M=130, N=124, K=160, dt="f32")),
    ("64x64x4 bf16", dict(M=129, N=65, K=1088)),
    ("128x64x2 bf16, bf16 out", dict(M=1275, N=1217, K=64, ydt=BF, res=None)),
]


@pytest.mark.parametrize("what,kw", RANDOM_CASES, ids=[c[0] for c in RANDOM_CASES])
def test_one_tile_kernel_random_values(H, what, kw):
    _check(_linear(H, exact=False, **kw), what)


# ---- the calls launch_glds_t used to refuse: bf16, M <= 64, K <= 512 and a feature set without a 9-deep tile.  They stay on 64x32x4.
FIX_CASES = [
    ("feat 4: bofi_linear with row_len, 50 x 96 x 128", dict(N=96, K=128, row_len=True), 50),
    ("feat 4: bofi_linear with row_len, N = 512, K = 512", dict(N=512, K=512, row_len=True, relu=1), 64),
    ("feat 64: bofi_linear_rows, capacity", dict(N=64, K=512, rows=33), 60),
    ("feat 12: bofi_linear_ex with dropout and row_len", dict(N=96, K=512, drop=0, row_len=True), 64),
    ("feat 6: bofi_linear_ex with row_len and a bf16 copy", dict(N=64, K=256, row_len=True, y2=True), 64),
    ("feat 4, scalar epilogue", dict(N=33, K=64, row_len=True, ldy_pad=1), 63),
]


@pytest.mark.parametrize("over", [False, True], ids=["M<=64", "M=65"])
@pytest.mark.parametrize("what,kw,M", FIX_CASES, ids=[c[0].split(":")[0] + f" #{i}" for i, c in enumerate(FIX_CASES)])
def test_small_m_calls_without_a_deep_tile_are_served(H, what, kw, M, over):
    """include/boficap_hip.h documents these calls as valid at any M; up to 64 rows they returned BOFI_ERR_ARG.  Status and values,
    and the same call one tile size up (M = 65)."""
    o = _linear(H, M=65 if over else M, **kw)
    assert o["rc"] == 0, f"{what}: refused with status {o['rc']}"
    _check(o, what)


def test_small_m_layernorm_in_statistics_out_is_served(H):
    """feature set 3 (bofi_linear_fused with ln_stats and stats_out) at M = 64 and M = 65: accepted, within the fold's bar."""
    for M in (64, 65):
        o = _linear(H, M=M, N=512, K=512, ln=16, stats=True, y2=True, exact=False)
        assert o["rc"] == 0, f"M = {M}: refused with status {o['rc']}"
        _check(o, f"feat 3 M={M}")


# ---- developer knobs that pick another tile or order for the same MFMA K order: BIT-equal to the default
DEEP_CASES = [dict(M=64, N=48, K=512, relu=1), dict(M=63, N=60, K=64, ldy_pad=4), dict(M=64, N=33, K=512, ydt=BF), dict(M=64, N=64, K=512, stats=True, y2=True),
              dict(M=33, N=32, K=128, drop=5), dict(M=17, N=32, K=128, drop=0, y2=True), dict(M=64, N=32, K=512, mask=True)]


@pytest.mark.parametrize("kw", DEEP_CASES, ids=lambda k: "-".join(f"{a}{b}" for a, b in k.items() if a not in "MNK") or "plain")
def test_whole_k_ring_equals_the_four_slot_ring(H, knobs, kw):
    """BOFI_GEMM_DEEP=0 (64x32x4 for every M <= 64) against the default (64x32x9 / 64x16x9) on specialised feature sets."""
    a = _linear(H, **kw)
    knobs(BOFI_GEMM_DEEP=0)
    b = _linear(H, **kw)
    _check(a, "default"); _check(b, "BOFI_GEMM_DEEP=0")
    _equal_outputs(a, b, "BOFI_GEMM_DEEP=0")


@pytest.mark.parametrize("groups", [16, 32])
def test_whole_k_ring_equals_the_four_slot_ring_with_the_layernorm_fold(H, knobs, groups):
    a = _linear(H, M=64, N=64, K=512, ln=groups, exact=False)
    knobs(BOFI_GEMM_DEEP=0)
    b = _linear(H, M=64, N=64, K=512, ln=groups, exact=False)
    _check(b, "BOFI_GEMM_DEEP=0")
    _equal_outputs(a, b, f"BOFI_GEMM_DEEP=0, LayerNorm fold over {groups} groups")


@pytest.mark.parametrize("kw", [dict(M=65, N=124, K=1024, ldy_pad=4), dict(M=129, N=65, K=1088, ydt=BF), dict(M=70, N=64, K=1024, stats=True, y2=True),
                                dict(M=70, N=64, K=1024, row_len=True, y2=True)], ids=["feat0-vector", "feat0-scalar", "feat2", "feat6"])
def test_long_k_ring_equals_the_two_slot_ring(H, knobs, kw):
    """BOFI_GEMM_HEUR2=0 (64x64x2) against the default (64x64x4) at K >= 1024."""
    a = _linear(H, **kw)
    knobs(BOFI_GEMM_HEUR2=0)
    b = _linear(H, **kw)
    _check(a, "default"); _check(b, "BOFI_GEMM_HEUR2=0")
    _equal_outputs(a, b, "BOFI_GEMM_HEUR2=0")


def test_long_k_ring_equals_the_two_slot_ring_with_the_layernorm_fold(H, knobs):
    a = _linear(H, M=70, N=64, K=1024, ln=32, exact=False)
    knobs(BOFI_GEMM_HEUR2=0)
    b = _linear(H, M=70, N=64, K=1024, ln=32, exact=False)
    _check(b, "BOFI_GEMM_HEUR2=0")
    _equal_outputs(a, b, "BOFI_GEMM_HEUR2=0, LayerNorm fold")


PLAIN_ORDER_CASES = [
    ("16 on 64x16x9", dict(M=64, N=48, K=512)), ("16 on 64x32x9", dict(M=63, N=33, K=64)), ("16 on 64x64x2", dict(M=200, N=190, K=64)),
    ("18 on 64x32x9", dict(M=64, N=64, K=512, stats=True, y2=True)), ("18 on 64x64x4", dict(M=200, N=192, K=1024, stats=True, y2=True)),
    ("80 on 64x32x4 (capacity 60)", dict(M=60, N=64, K=512, rows=33)), ("80 on 64x64x2", dict(M=200, N=124, K=128, rows=70)),
    ("16 on 128x64x2", dict(M=1275, N=1344, K=64)),
    ("18 on 64x64x2", dict(M=200, N=192, K=128, stats=True, y2=True)), ("18 on 128x64x2", dict(M=1275, N=1280, K=64, stats=True, y2=True)),
    ("16 on 64x32x4 (K > 512)", dict(M=64, N=96, K=576)),
]


@pytest.mark.parametrize("what,kw", PLAIN_ORDER_CASES, ids=[c[0] for c in PLAIN_ORDER_CASES])
def test_plain_tile_order_equals_the_xcd_order(H, knobs, what, kw):
    """BOFI_GEMM_DBG=16 (plain tile order, valid results; feature sets 16 / 18 / 80) against the default order."""
    a = _linear(H, **kw)
    knobs(BOFI_GEMM_DBG=16)
    b = _linear(H, **kw)
    _check(a, "default"); _check(b, what)
    _equal_outputs(a, b, what)


@pytest.mark.parametrize("M,N,K,groups", [(64, 64, 512, 16), (63, 36, 256, 8), (130, 124, 512, 32), (70, 64, 1024, 32), (1275, 1280, 64, 16)])
def test_plain_tile_order_with_the_layernorm_fold(H, knobs, M, N, K, groups):
    """feature set 17"""
    a = _linear(H, M=M, N=N, K=K, ln=groups, exact=False, res=None)
    knobs(BOFI_GEMM_DBG=16)
    b = _linear(H, M=M, N=N, K=K, ln=groups, exact=False, res=None)
    _check(b, "feat 17")
    _equal_outputs(a, b, "feat 17")


# ================================================================================================ (b) XCD tile order
# gemm_glds.hip, the mapping at the head of the kernel: workgroup -> (XCD, index) -> a linear order that walks row_bands bands of
# row tiles.  Claimed bijective for any tile count: a tile visited twice or never leaves a sentinel or is caught by nothing else.
BAND_CASES = [
    ("64x64: 5 x 3 tiles, 15 % 8 != 0; 4 bands leave a last band of 1", dict(M=320 - 7, N=192 - 4, K=64)),
    ("64x64: 2 x 3 tiles, fewer than 8", dict(M=128, N=129, K=64)),
    ("64x64: 3 x 4 tiles, more bands than row tiles", dict(M=190, N=256, K=128, ydt=BF)),
    ("64x64: 7 x 1 tiles", dict(M=400, N=60, K=64, dt="f32")),
    ("128x64: 10 x 21 tiles, 210 % 8 = 2; 4 bands leave a last band of 1", dict(M=1275, N=1344 - 4, K=64)),
]


@pytest.mark.parametrize("what,kw", BAND_CASES, ids=[c[0].split(":")[0] + f" #{i}" for i, c in enumerate(BAND_CASES)])
def test_xcd_tile_order_is_a_bijection_for_every_band_count(H, knobs, what, kw):
    base = _linear(H, **kw)
    _check(base, what + " (default)")
    for bands in (1, 2, 4, 8):
        knobs(BOFI_GEMM_BANDS=bands)
        o = _linear(H, **kw)
        _check(o, f"{what} (BOFI_GEMM_BANDS={bands})")
        _equal_outputs(base, o, f"BOFI_GEMM_BANDS={bands}")


# ================================================================================================ (c) persistent kernel
# launch_gemm_pers: feature sets 0-3, each with and without residual (the eight switch cases); FAST = bf16 out, no residual, no
# statistics; the staged epilogue otherwise (float32 out, or BOFI_GEMM_PERS_FAST=0).  BOFI_GEMM_PERS_MIN=1 brings small shapes to it on
# 128-row tiles, BOFI_GEMM_PERS_BM128=0 on 256-row tiles.  N % 128 == 0, K >= 192, LayerNorm over 16 groups.
PERS_FEATS = [
    ("case 0: feat 0, FAST", dict(ydt=BF, res=None), {}),
    ("case 0: feat 0, staged by knob", dict(ydt=BF, res=None), dict(BOFI_GEMM_PERS_FAST=0)),
    ("case 0: feat 0, staged by float32 out", dict(res=None, relu=1), {}),
    ("case 1: feat 0 + residual", dict(ydt=BF), {}),
    ("case 2: feat 1, FAST", dict(ln=16, ydt=BF, res=None, relu=1), {}),
    ("case 2: feat 1, staged by knob", dict(ln=16, ydt=BF, res=None), dict(BOFI_GEMM_PERS_FAST=0)),
    ("case 3: feat 1 + residual", dict(ln=16), {}),
    ("case 4: feat 2", dict(stats=True, y2=True, res=None), {}),
    ("case 5: feat 2 + residual", dict(stats=True, y2=True), {}),
    ("case 6: feat 3", dict(ln=16, stats=True, y2=True, res=None), {}),
    ("case 7: feat 3 + residual", dict(ln=16, stats=True, y2=True), {}),
]


@pytest.mark.parametrize("rows256", [False, True], ids=["128-row", "256-row"])
@pytest.mark.parametrize("what,kw,extra", PERS_FEATS, ids=[c[0] for c in PERS_FEATS])
def test_persistent_kernel_every_switch_case_on_both_tile_heights(H, knobs, what, kw, extra, rows256):
    """M = 300 (a ragged last row tile on either height), N = 256 (two column tiles), K = 512; M = 513, N = 128, K = 192 (the shortest K,
    a last row tile of 1) without the fold.  Bit-equal to the one-tile kernel, and the exact probe / the operator's bar."""
    shapes = [(300, 256, 512)] + ([] if kw.get("ln") else [(513, 128, 192)])
    for M, N, K in shapes:
        exact = not kw.get("ln")
        knobs(BOFI_GEMM_PERS=1, BOFI_GEMM_PERS_MIN=1, BOFI_GEMM_PERS_BM128=0 if rows256 else None, **extra)
        a = _linear(H, M=M, N=N, K=K, exact=exact, **kw)
        knobs(BOFI_GEMM_PERS=0)
        b = _linear(H, M=M, N=N, K=K, exact=exact, **kw)
        _check(a, f"{what} persistent {M}x{N}x{K}"); _check(b, f"{what} one tile {M}x{N}x{K}")
        _equal_outputs(a, b, f"{what} {M}x{N}x{K}")


# ================================================================================================ (d) register-staged kernel (gemm.hip)
# float32 x with bf16 w.  launch_tiles: M > 64 and >= 224 tiles of 128x128 -> 128x128; M > 64 or N >= 2048 -> 64x64; else 64x32.
STAGED_CASES = [
    ("128x128 M=1787 N=2048 K=64: 14 x 16 tiles, ragged M, row_len, relu", dict(M=1792 - 5, N=2048, K=64, row_len=True, relu=1, ldy_pad=4)),
    ("128x128 M=1787 N=2046 K=64: N % 4 != 0, bf16 out", dict(M=1792 - 5, N=2046, K=64, ydt=BF, relu=1, ldy_pad=1)),
    ("64x64 M=70 N=101 K=128: M > 64, N % 4 != 0, row_len, relu", dict(M=70, N=101, K=128, row_len=True, relu=1, ldy_pad=3)),
    ("64x64 M=130 N=64 K=64: bf16 out, broadcast residual", dict(M=130, N=64, K=64, ydt=BF, res="bcast")),
    ("64x64 M=30 N=2050 K=64: M <= 64 and N >= 2048, N % 4 != 0", dict(M=30, N=2050, K=64, row_len=True, relu=1)),
    ("64x64 M=64 N=2048 K=128: bf16 out", dict(M=64, N=2048, K=128, ydt=BF, relu=1)),
    ("64x32 M=63 N=33 K=192: N % 4 != 0, row_len, relu", dict(M=63, N=33, K=192, row_len=True, relu=1, ldy_pad=2)),
    ("64x32 M=1 N=96 K=64: bf16 out", dict(M=1, N=96, K=64, ydt=BF)),
    ("64x32 M=64 N=2044 K=64: just below the 64x64 threshold", dict(M=64, N=2044, K=64)),
]


@pytest.mark.parametrize("what,kw", STAGED_CASES, ids=[c[0].split(":")[0] for c in STAGED_CASES])
def test_register_staged_kernel_exact_on_every_tile(H, what, kw):
    _check(_linear(H, dt="mixed", **kw), what)


@pytest.mark.parametrize("M,N,K,ydt", [(70, 101, 128, F32), (63, 33, 192, BF), (300, 256, 64, F32)])
def test_register_staged_kernel_random_values(H, M, N, K, ydt):
    _check(_linear(H, M=M, N=N, K=K, dt="mixed", ydt=ydt, exact=False, relu=1), f"staged {M}x{N}x{K}")


# ================================================================================================ (e) weight-gradient GEMM (gemm_tn.hip)
def _tn_problem(g, M, NI, NJ, *, a_extra=8, b_extra=0, pitch=16, colsum=True):
    """c [NI, NJ] (+ 3 columns of pitch) += a^T b with a [M, NI], b [M, NJ] in {-1, 0, 1}; a_cols > NI holds zeros (the header's contract),
    the pitch behind a_cols / b_cols NaN: a kernel that reads it poisons the result.  c and colsum start from integers."""
    up8 = lambda v: (v + 7) // 8 * 8
    a_cols, b_cols = up8(NI) + a_extra, up8(NJ) + b_extra
    a = torch.full((max(M, 1), a_cols + pitch), float("nan"))
    b = torch.full((max(M, 1), b_cols + pitch), float("nan"))
    a[:, :a_cols] = 0; b[:, :b_cols] = 0
    a[:M, :NI] = _tern(g, M, NI); b[:M, :NJ] = _tern(g, M, NJ)
    c0 = torch.full((NI, NJ + 3), SENT)
    c0[:, :NJ] = torch.randint(-9, 10, (NI, NJ), generator=g).float()
    s0 = torch.randint(-9, 10, (NI,), generator=g).float()
    return dict(a=a.to(BF).cuda(), b=b.to(BF).cuda(), a_cols=a_cols, b_cols=b_cols, c=c0.cuda(), cs=s0.cuda() if colsum else None, M=M, NI=NI, NJ=NJ,
                c_ref=c0[:, :NJ].double() + a[:M, :NI].double().t() @ b[:M, :NJ].double(), cs_ref=s0.double() + a[:M, :NI].double().sum(0))


def _tn_check(p, what):
    got = p["c"].cpu()
    assert bool((got[:, p["NJ"]:] == SENT).all()), f"{what}: c written beyond column NJ"
    bad = (got[:, :p["NJ"]].double() != p["c_ref"]).nonzero()
    assert bad.numel() == 0, f"{what}: c differs at {bad.shape[0]} elements, first {bad[0].tolist()}"
    if p["cs"] is not None:
        assert torch.equal(p["cs"].cpu().double(), p["cs_ref"]), f"{what}: column sums"


TN_SHAPES = [(37, 20, 24), (1, 64, 64), (64, 64, 64), (200, 70, 130), (300, 128, 65), (129, 200, 136), (1000, 64, 192)]


@pytest.mark.parametrize("colsum", [True, False], ids=["colsum", "no-colsum"])
@pytest.mark.parametrize("M,NI,NJ", TN_SHAPES)
def test_weight_gradient_gemm_exact(H, M, NI, NJ, colsum):
    """bofi_gemm_tn_acc (64 x 64 tiles, rows split over workgroups): M below one row block, M % 64 != 0, several splits (M = 300, 1000),
    ragged output tiles, accumulation into a non-zero c."""
    p = _tn_problem(torch.Generator().manual_seed(M + NI + NJ), M, NI, NJ, colsum=colsum)
    rc = H.lib().bofi_gemm_tn_acc(H.ptr(p["a"]), p["a"].shape[1], p["a_cols"], H.ptr(p["b"]), p["b"].shape[1], p["b_cols"], H.ptr(p["c"]), p["NJ"] + 3,
                                  M, NI, NJ, H.ptr(p["cs"]), H.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    _tn_check(p, f"tn_acc {M}x{NI}x{NJ}")


def _tn_grouped(H, probs):
    n = len(probs)
    vp, ia = C.c_void_p * n, C.c_int * n
    ints = lambda f: ia(*[int(f(p)) for p in probs])
    ptrs = lambda k: vp(*[None if p[k] is None else p[k].data_ptr() for p in probs])
    rc = H.lib().bofi_gemm_tn_grouped(n, ptrs("a"), ints(lambda p: p["a"].shape[1]), ints(lambda p: p["a_cols"]), ptrs("b"), ints(lambda p: p["b"].shape[1]),
                                      ints(lambda p: p["b_cols"]), ptrs("c"), ints(lambda p: p["NJ"] + 3), ints(lambda p: p["M"]), ints(lambda p: p["NI"]),
                                      ints(lambda p: p["NJ"]), ptrs("cs"), H.stream_ptr())
    torch.cuda.synchronize()
    return rc


# (M, NI, NJ): both tile classes (NI, NJ >= 128 -> 128 x 128 tiles, else 64 x 64), a mixed NI < 128 <= NJ problem, M = 0 inside the group
TN_GROUP = [(200, 128, 128), (37, 20, 24), (0, 64, 64), (129, 100, 136), (300, 200, 130), (64, 64, 64), (1, 130, 129), (0, 128, 128), (257, 136, 264), (70, 8, 8)]


@pytest.mark.parametrize("wt", [0, 2, 4], ids=["default", "BOFI_TN_WT=2", "BOFI_TN_WT=4"])
def test_grouped_weight_gradient_gemms_exact(H, knobs, wt):
    """bofi_gemm_tn_grouped on both tile classes, column sums given and NULL entry by entry; one tile class forced for everything
    (BOFI_TN_WT) gives the same integers."""
    if wt:
        knobs(BOFI_TN_WT=wt)
    g = torch.Generator().manual_seed(99)
    probs = [_tn_problem(g, M, NI, NJ, colsum=e % 3 != 1, a_extra=8 * (e % 2)) for e, (M, NI, NJ) in enumerate(TN_GROUP)]
    assert _tn_grouped(H, probs) == 0
    for e, p in enumerate(probs):
        _tn_check(p, f"grouped problem {e} {TN_GROUP[e]}")


@pytest.mark.parametrize("M,NI,NJ", [(70, 20, 24), (64, 128, 128)], ids=["64x64 class", "128x128 class"])
def test_grouped_weight_gradient_gemms_second_launch(H, M, NI, NJ):
    """45 problems of one class: the kernel arguments hold 40, so a second launch takes the last five (one of them empty)."""
    g = torch.Generator().manual_seed(NI)
    probs = [_tn_problem(g, 0 if e == 42 else M + e, NI, NJ, colsum=e % 2 == 0) for e in range(45)]
    assert _tn_grouped(H, probs) == 0
    for e, p in enumerate(probs):
        _tn_check(p, f"problem {e} of 45")
