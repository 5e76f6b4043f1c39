"""The decoder layers' cross K|V projected BESIDE the bounding loop (bound_loop_kernel<5, true> of boficap_amd/csrc/bound_loop.hip, bofi_engine_set_bound_kv_beside):
extra workgroups of the loop kernel's launch run rb_gemm_kernel<false, 6>'s body (csrc/bofi_rowblock.h) over the columns [1024, N) of the stacked K|V, with the row
sums taken in the order of the feed-forward kernel's projection tail; the encoder's last feed-forward launch projects the bounding layer's 1 024 columns only.

What must hold, all of it bit for bit (the form moves work, it changes no arithmetic):
  * every column of the engine's stacked K|V is the OTHER FORM's (setter 0: all 7 168 columns in the tail of the encoder's last feed-forward launch);
  * hence every output of the decode -- what the loop writes, the captions, their log-probabilities -- equals the other form's;
  * the form is taken exactly where the engine says so, and nowhere else does a decode change;
  * launches in flight do not disturb each other.
The full-width model with seeded weights (the loop kernel has no narrow form); the row-block family and its 96-row blocks forced at these small sizes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

R0 = 36
BOUND_COLS = 1024                 # the bounding layer's K|V columns: what the loop reads
KEYS = ("seq", "phrase_num", "phrase_length", "phrase_syn", "bound_iters")


@pytest.fixture(scope="module")
def env():
    """Row-block kernels from 0 rows on, 96-row projection blocks from 0 rows on -- for every decode of this module, whatever its form."""
    import os
    from boficap_amd import hip as H
    keep = {k: os.environ.get(k) for k in ("BOFI_RB_MIN_ROWS", "BOFI_RB_GEMM_MT8_ROWS", "BOFI_RB_FFN_PROJ_MAXN")}
    os.environ["BOFI_RB_MIN_ROWS"] = "0"
    os.environ["BOFI_RB_GEMM_MT8_ROWS"] = "0"
    os.environ.pop("BOFI_RB_FFN_PROJ_MAXN", None)
    H.lib().bofi_reload_env()
    yield H
    for k, v in keep.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    H.lib().bofi_reload_env()


@pytest.fixture(scope="module")
def base(env, weight_cache):
    """One engine for the module (150 images, 48 regions); larger or concurrent launches run on forks of it."""
    from boficap_amd.engine import BofiEngine
    cfg, sd = weight_cache("FULL", 0, 1.0)
    eng = BofiEngine(cfg, torch.bfloat16, max_batch=150, max_regions=48)
    eng.load_state_dict(sd)
    eng.set_decodes_in_flight(2)
    return cfg, eng


def _inputs(cfg, B, R, seed, ragged):
    from boficap_amd import weights as W
    att_np = W.synthetic_att_feats(B, R, cfg.att_feat_size, seed=seed)
    att_len = None
    if ragged:
        lens = np.random.default_rng(seed).integers(R // 3, R + 1, B).astype(np.int32)
        lens[0] = R
        lens[3] = 0                                   # an image without regions: NaN through the cross-attentions
        for b in range(B):
            att_np[b, lens[b]:] = 0
        att_len = torch.from_numpy(lens).cuda()
    return torch.from_numpy(att_np).cuda().to(torch.bfloat16), att_len


def _read(H, eng, name, shape, dtype):
    t = torch.empty(shape, dtype=dtype, device="cuda")
    H.check(H.lib().bofi_engine_debug_copy(eng._h, name.encode(), H.ptr(t), t.numel() * t.element_size(), H.stream_ptr()), name)
    return t


def _kv(H, eng, cfg, M):
    N = 2 * cfg.d_model * (1 + cfg.N_dec)
    return _read(H, eng, "kv", (M, N), torch.int16)


def _same(a, b, keys=KEYS, logprob=True):
    for k in keys:
        assert torch.equal(a[k], b[k]), k
    if logprob:
        assert torch.equal(a["seq_logprob"].isnan(), b["seq_logprob"].isnan())
        assert torch.equal(a["seq_logprob"].nan_to_num().view(torch.int32), b["seq_logprob"].nan_to_num().view(torch.int32))


# 17 images: two loop groups (the second ragged), 612 rows = 7 row blocks of 96 (the last ragged), one workgroup per row block; 150: ten groups, 57 row blocks, two workgroups per
# row block; 150 under a hint of 8 launches in flight: the projection's share of the chip is 12 workgroups, which WALK the 57 row blocks (five for most, four for the last three)
CASES = [(17, 2), (150, 2), (150, 8)]


@pytest.fixture
def hinted(base):
    """base's engine under another decodes-in-flight hint for one test."""
    cfg, eng = base

    def set_hint(n):
        eng.set_decodes_in_flight(n)
        return cfg, eng
    yield set_hint
    eng.set_decodes_in_flight(2)


@pytest.mark.parametrize("B,hint", CASES)
def test_kv_columns_are_the_other_forms_bits(B, hint, env, hinted):
    H = env
    cfg, eng = hinted(hint)
    d, M = cfg.d_model, B * R0
    N = 2 * d * (1 + cfg.N_dec)
    att, _ = _inputs(cfg, B, R0, 100 + B + 1000 * hint, False)         # (inputs of this case alone: the engine's K|V buffer holds another decode's values)
    assert eng.bound_kv_beside_active(B, R0)
    out = eng.decode_naic(att, None, strict_q1=False)
    kv_new = _kv(H, eng, cfg, M)
    x_new = _read(H, eng, "x_enc", (M, d), torch.float32)
    assert int((kv_new[:, BOUND_COLS:] != 0).sum()) > 0.9 * M * (N - BOUND_COLS)          # (really written)
    eng.set_bound_kv_beside(0)
    try:
        assert not eng.bound_kv_beside_active(B, R0)
        old = eng.decode_naic(att, None, strict_q1=False)
        kv_old = _kv(H, eng, cfg, M)
        x_old = _read(H, eng, "x_enc", (M, d), torch.float32)
    finally:
        eng.set_bound_kv_beside(1)
    assert torch.equal(x_new.view(torch.int32), x_old.view(torch.int32))           # the same encoder output ...
    assert torch.equal(kv_new[:, :BOUND_COLS], kv_old[:, :BOUND_COLS])             # ... the tail's 1 024 columns as among 7 168 ...
    assert torch.equal(kv_new[:, BOUND_COLS:], kv_old[:, BOUND_COLS:])             # ... and the projection role's 6 144 as the tail's
    _same(out, old)
    if B == 150:                                                    # pairs really form (diagnostic counter 5: groups whose loop ran as a pair)
        eng.decode_naic(att, None, strict_q1=False)
        assert int(_read(H, eng, "counters", (8,), torch.int32)[5]) >= 1


@pytest.mark.parametrize("B,hint", CASES)
def test_whole_decode_equals_the_other_form(B, hint, env, hinted):
    H = env
    cfg, eng = hinted(hint)
    att, att_len = _inputs(cfg, B, R0, 200 + B + 1000 * hint, True)
    assert eng.bound_kv_beside_active(B, R0)
    new = eng.decode_naic(att, att_len, strict_q1=False)
    g = eng.decode_naic(att, att_len, strict_q1=False, graph=True)
    g = eng.decode_naic(att, att_len, strict_q1=False, graph=True, out=g)
    g1 = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in g.items()}
    g = eng.decode_naic(att, att_len, strict_q1=False, graph=True, out=g)            # a second replay
    eng.set_bound_kv_beside(0)
    try:
        old = eng.decode_naic(att, att_len, strict_q1=False)
    finally:
        eng.set_bound_kv_beside(1)
    torch.cuda.synchronize()
    assert int(new["phrase_num"].max()) >= 4 and int(new["bound_iters"]) >= 5           # the loop really ran
    assert int(new["phrase_num"][3]) == 0                                              # the empty image ended at once
    for o in (new, g1, g):
        _same(o, old)                                     # what the loop writes, the captions and their log-probabilities: the other form's


def _pair(eng, att, att_len, **kw):
    """The same decode under setter 1 (the default) and setter 0."""
    a = eng.decode_naic(att, att_len, strict_q1=False, **kw)
    eng.set_bound_kv_beside(0)
    try:
        b = eng.decode_naic(att, att_len, strict_q1=False, **kw)
    finally:
        eng.set_bound_kv_beside(1)
    return a, b


def test_the_form_is_taken_where_the_engine_says_and_nowhere_else(env, base):
    cfg, eng = base
    B = 150
    att, att_len = _inputs(cfg, B, R0, 301, True)
    assert eng.bound_kv_beside_active(B, R0)                      # 150 images, hint 2
    # a decode that runs alone
    eng.set_decodes_in_flight(1)
    try:
        assert not eng.bound_kv_beside_active(B, R0)
        _same(*_pair(eng, att, att_len))
    finally:
        eng.set_decodes_in_flight(2)
    # the five-launch bounding iterations
    eng.set_bound_loop(0)
    try:
        assert not eng.bound_kv_beside_active(B, R0)
        _same(*_pair(eng, att, att_len))
    finally:
        eng.set_bound_loop(-1)
    # a launch above the pair's size
    big = eng.fork(max_batch=400)
    big.set_decodes_in_flight(2)
    att4, len4 = _inputs(cfg, 400, R0, 302, True)
    assert not big.bound_kv_beside_active(400, R0) and big.bound_kv_beside_active(384, R0)
    _same(*_pair(big, att4, len4))
    del big
    # the phased call: ENCODE promises the whole stacked K|V
    assert not eng.bound_kv_beside_active(B, R0, "e") and not eng.bound_kv_beside_active(B, R0, "b") and not eng.bound_kv_beside_active(B, R0, "ebf")

    def phased(out=None):
        for ph in "ebf":
            out = eng.decode_naic(att, att_len, strict_q1=False, phases=ph, out=out)
        return out
    a = phased()
    eng.set_bound_kv_beside(0)
    try:
        b = phased()
        whole = eng.decode_naic(att, att_len, strict_q1=False)
    finally:
        eng.set_bound_kv_beside(1)
    _same(a, b)
    _same(a, whole)
    # more than 36 regions
    att48, len48 = _inputs(cfg, B, 48, 303, True)
    assert not eng.bound_kv_beside_active(B, 48)
    _same(*_pair(eng, att48, len48))
    # the setter itself, and what a fork starts from
    eng.set_bound_kv_beside(0)
    try:
        assert not eng.bound_kv_beside_active(B, R0)
        f0 = eng.fork()
    finally:
        eng.set_bound_kv_beside(1)
    f1 = eng.fork()
    assert not f0.bound_kv_beside_active(B, R0) and f1.bound_kv_beside_active(B, R0)          # each fork with the mode its parent had when it was made (and no hint: throughput forms)
    a, b = f0.decode_naic(att, att_len, strict_q1=False), f1.decode_naic(att, att_len, strict_q1=False)
    _same(a, b)
    f0.set_bound_kv_beside(1)
    assert f0.bound_kv_beside_active(B, R0)
    _same(f0.decode_naic(att, att_len, strict_q1=False), b)
    # pairs forced by the environment (the setting of the pair's own tests): nothing else moves
    import os
    os.environ["BOFI_BL_PAIR"] = "2"
    env.lib().bofi_reload_env()
    try:
        assert not eng.bound_kv_beside_active(B, R0)
        _same(*_pair(eng, att, att_len))
    finally:
        os.environ.pop("BOFI_BL_PAIR")
        env.lib().bofi_reload_env()
    assert eng.bound_kv_beside_active(B, R0)
    with pytest.raises(env.BofiHipError):
        eng.set_bound_kv_beside(2)
    torch.cuda.synchronize()


def test_launches_in_flight_equal_the_same_launches_alone(env, base):
    """Three forks of 150 images on their own streams, three launches each: every launch's outputs equal the same launch run with nothing beside it, and every fork's
    K|V is its own last launch's (a projection workgroup writes its own engine's buffer only)."""
    H = env
    cfg, eng = base
    B, M, NF, NL = 150, 150 * R0, 3, 3
    forks = [eng.fork() for _ in range(NF)]
    for f in forks:
        f.set_decodes_in_flight(NF)
        assert f.bound_kv_beside_active(B, R0)
    inputs = [[_inputs(cfg, B, R0, 400 + 10 * i + j, True) for j in range(NL)] for i in range(NF)]
    streams = [f.stream() for f in forks]
    torch.cuda.synchronize()
    flight = [[None] * NL for _ in range(NF)]
    for j in range(NL):
        for i, f in enumerate(forks):
            with torch.cuda.stream(streams[i]):
                flight[i][j] = f.decode_naic(*inputs[i][j], strict_q1=False)
    torch.cuda.synchronize()
    kv_flight = [_kv(H, f, cfg, M) for f in forks]
    torch.cuda.synchronize()
    for i, f in enumerate(forks):
        for j in range(NL):
            alone = f.decode_naic(*inputs[i][j], strict_q1=False)
            torch.cuda.synchronize()
            _same(flight[i][j], alone)
        assert torch.equal(kv_flight[i], _kv(H, f, cfg, M))


def test_the_benchmarks_launch_shape_equals_the_other_form(env, base):
    """320 images under a hint of four launches in flight (the shape of `bench.py --steps 20`): 120 row blocks walked by 24 projection workgroups, five each."""
    H = env
    cfg, eng = base
    B, M = 320, 320 * R0
    f = eng.fork(max_batch=B)
    f.set_decodes_in_flight(4)
    att, att_len = _inputs(cfg, B, R0, 500, True)
    assert f.bound_kv_beside_active(B, R0)
    new = f.decode_naic(att, att_len, strict_q1=False)
    kv_new = _kv(H, f, cfg, M)
    f.set_bound_kv_beside(0)
    old = f.decode_naic(att, att_len, strict_q1=False)
    kv_old = _kv(H, f, cfg, M)
    torch.cuda.synchronize()
    assert torch.equal(kv_new, kv_old)
    _same(new, old)
