"""The constrained pick on the MI355X: the kernel against the numpy restatement (exact), the float32 engine against the restated decode
(tests/test_constrained_pick.py), the bf16 engine held without a tolerance to ``pick_np`` on its OWN returned log-probs (plain, graph replay, fork, phased form,
grouped batches), "off is today's decode", the refusals, and the interface above the engine (decode_many, mode='sample', eval_split)."""
import functools

import numpy as np
import pytest
import torch

import boficap_oracle as O
from conftest import record_parity
from test_constrained_pick import NAN, VARIANTS, pick_np, plain_of, restate

pytestmark = pytest.mark.gpu

LAYOUT = ("phrase_num", "phrase_length", "phrase_syn")
KEEP = 123.0                                   # what stands in row_chosen before a launch: positions past n_b must keep it


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b, keys):
    return all(torch.equal(_bits(a[k]) if a[k].is_floating_point() else a[k], _bits(b[k]) if b[k].is_floating_point() else b[k]) for k in keys)


def _clone(r):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in r.items()}


# ----------------------------------------------------------------------------- 1. the kernel
def _rows(rng, B, S, V, ldx):
    """x [B * S, ldx] float32: values from a small set (exact ties abound, +0.0 and -0.0 among them) under Gaussian rows, NaNs and infinities sprinkled in, whole rows
    of -inf / NaN / one value, leaders that repeat along a caption (chains of the same best id, of the same best two), and poison past column V."""
    vals = np.array([-0.125, -0.5, -0.5, -1.0, -2.0, -3.5, -0.0, 0.0], np.float32)
    x = rng.standard_normal((B, S, ldx)).astype(np.float32) - 4.0
    tie = rng.random((B, S, ldx)) < 0.3
    x[tie] = vals[rng.integers(0, len(vals), int(tie.sum()))]
    x[rng.random((B, S, ldx)) < 0.01] = -np.inf
    for b, s in zip(*np.nonzero(rng.random((B, S)) < 0.15)):    # a NaN or three in one row of seven; +inf likewise (twice: a tie at the top)
        x[b, s, rng.integers(0, V, int(rng.integers(1, 4)))] = NAN
    for b, s in zip(*np.nonzero(rng.random((B, S)) < 0.15)):
        x[b, s, rng.integers(0, V, int(rng.integers(1, 3)))] = np.inf
    for b in range(B):                                          # chains: one word id >= 7 leads a run of positions, a second one is the runner-up for part of it
        a, c = (int(v) for v in rng.choice(np.arange(7, V), 2, replace=False))
        s0 = int(rng.integers(0, max(1, S - 4)))
        x[b, s0:s0 + 5, a] = 5.0
        x[b, s0 + 1:s0 + 3, c] = 4.0
        low = int(rng.integers(0, 7))                           # ... and an id below repeat_min_id leads another run: it may repeat
        x[b, max(0, s0 - 3):s0, low] = 6.0
    if B * S >= 8:
        flat = x.reshape(B * S, ldx)
        flat[3] = -np.inf
        flat[5] = NAN
        flat[6] = -0.75
        flat[7, :] = -np.inf; flat[7, V - 1] = -1.0             # the last id alone
    x[:, :, V:] = np.inf                                        # a padded pitch: never read
    if ldx > V + 1:
        x[:, :, V + 1] = NAN
    return x


CASES = [(1, 20, 64, 64), (5, 20, 9491, 9491), (3, 64, 9491, 9600), (130, 20, 257, 257)]


@pytest.mark.parametrize("B,S,V,ldx", CASES)
def test_kernel_equals_pick_np(B, S, V, ldx):
    """seq, row_chosen and changed bit for bit, on every variant of the optional arguments; ntok holds 0, 1, S and values outside 0 .. S (clamped), read with a bias; the
    tensor starts 1, 2, 3 floats off a 16-byte boundary as well (with V = 9 491 the rows then walk through every misalignment)."""
    from boficap_amd import hip
    rng = np.random.default_rng(7000 + 100 * B + S + V)
    x = _rows(rng, B, S, V, ldx)
    n = rng.integers(0, S + 1, B)
    n[:min(B, 3)] = [S, 0, 1][:min(B, 3)]
    ntok = (n + 1).astype(np.int32)                             # the engine's form: `last` with a bias of -1
    if B > 8:
        ntok[5], ntok[6], n[5], n[6] = -4, S + 9, 0, S
    order = np.argsort(-np.nan_to_num(x[:, :, :V].reshape(B * S, V), nan=np.inf), axis=1, kind="stable")
    ban = set(rng.choice(V, V // 8, replace=False).tolist()) | set(order[::3, 0].tolist()) | set(order[::7, 1].tolist())      # banned leaders, banned best two
    ban = sorted(ban)[:V - 2] if len(ban) > V - 2 else sorted(ban)
    old = rng.integers(0, V, (B, S)).astype(np.int64)
    old[::2] = order[:, 0].reshape(B, S)[::2]                   # half of the images enter with the plain argmax standing in seq
    d_ntok, d_ban = torch.from_numpy(ntok).cuda(), hip.ban_bits(ban, V, "cuda")
    runs = [(v, rep, min_id) for v in ("all", "no_ntok", "no_ban", "no_outputs") for rep, min_id in (((True, 7), (False, 7), (True, 0)) if v == "all" else ((True, 7),))]
    wants = {(v, rep, min_id): pick_np(x[:, :, :V], np.full(B, S) if v == "no_ntok" else n, () if v == "no_ban" else ban, rep, min_id, pad=2, old=old)
             for v, rep, min_id in runs}                       # (computed once: the restatement does not depend on where the tensor starts)
    for off in ((0, 1, 2, 3) if B <= 5 else (0,)):
        buf = torch.full((B * S * ldx + 8,), 7.0, dtype=torch.float32, device="cuda")
        dx = buf[off:off + B * S * ldx].view(B * S, ldx)
        dx.copy_(torch.from_numpy(x.reshape(B * S, ldx)))
        assert (dx.data_ptr() // 4) % 4 == (buf.data_ptr() // 4 + off) % 4
        for variant, rep, min_id in runs:
            nn = np.full(B, S) if variant == "no_ntok" else n
            want = wants[(variant, rep, min_id)]
            seq = torch.from_numpy(old.copy()).cuda().view(-1)
            chosen = torch.full((B * S,), KEEP, dtype=torch.float32, device="cuda") if variant != "no_outputs" else None
            changed = torch.full((B,), -1, dtype=torch.int32, device="cuda") if variant != "no_outputs" else None
            hip.vocab_constrain(dx, V, S, seq, ntok=None if variant == "no_ntok" else d_ntok, ntok_bias=0 if variant == "no_ntok" else -1, pad_idx=2,
                                ban=None if variant == "no_ban" else d_ban, no_repeat=rep, repeat_min_id=min_id, row_chosen=chosen, changed=changed)
            torch.cuda.synchronize()
            what = (B, S, V, ldx, off, variant, rep, min_id)
            assert np.array_equal(seq.cpu().numpy().reshape(B, S), want["seq"]), what
            if variant != "no_outputs":
                live = np.arange(S)[None, :] < np.clip(nn, 0, S)[:, None]
                expect = np.where(live, want["chosen"], np.float32(KEEP)).astype(np.float32)
                assert np.array_equal(chosen.cpu().numpy().reshape(B, S).view(np.int32), expect.view(np.int32)), what
                assert np.array_equal(changed.cpu().numpy(), want["changed"]), what
        assert np.array_equal(dx.cpu().numpy().view(np.int32), x.reshape(B * S, ldx).view(np.int32))      # (x is read only)


def _plain_rows(rng, B, S, V):
    """x [B, S, V] float32 for a V below _rows' nine: Gaussian rows, an exact tie at the top of every third row, one NaN and one -inf."""
    x = rng.standard_normal((B, S, V)).astype(np.float32)
    flat = x.reshape(B * S, V)
    for r in range(0, B * S, 3):
        flat[r, rng.choice(V, 2, replace=False)] = flat[r].max()
    flat[1, int(rng.integers(0, V))] = NAN
    flat[B * S - 2, int(rng.integers(0, V))] = -np.inf
    return x


def _short_case(V, B=2, S=8):
    """(x, n, ntok, ban, old) of the short-row tests here and in test_gpu_trigram_pick: ntok in the engine's form (bias -1), image 1 shorter than S; at most V - 2 ids
    banned, the best id of row 0 among them."""
    rng = np.random.default_rng(7700 + V)
    x = _plain_rows(rng, B, S, V)
    n = np.array([S, S - 3])
    best = int(np.argsort(-np.nan_to_num(x[0, 0], nan=np.inf), kind="stable")[0])
    ban = sorted(([best] + [int(i) for i in rng.permutation(V) if int(i) != best])[:min(V - 2, 2)])
    old = rng.integers(0, V, (B, S)).astype(np.int64)
    return x, n, (n + 1).astype(np.int32), ban, old


def _at_offset(x2d, off):
    """x2d [rows, ldx] on the device, its first element ``off`` floats behind a 16-byte boundary."""
    buf = torch.full((x2d.size + 8,), 7.0, dtype=torch.float32, device="cuda")
    dx = buf[off:off + x2d.size].view(x2d.shape)
    dx.copy_(torch.from_numpy(x2d))
    assert (dx.data_ptr() // 4) % 4 == (buf.data_ptr() // 4 + off) % 4
    return dx


@pytest.mark.parametrize("V", [2, 3, 5, 6])
def test_kernel_on_rows_shorter_than_a_wavefronts_loads(V):
    """ldx = V below 8 floats, the tensor 0, 1, 2, 3 floats off a 16-byte boundary: the rows walk through every alignment, so the row stream meets a peel cut short by V,
    rows without one 16-byte group, peel-only and tail-only rows.  seq, row_chosen and changed bit for bit against pick_np, with the table (an empty one at V = 2) and without."""
    from boficap_amd import hip
    B, S = 2, 8
    x, n, ntok, ban, old = _short_case(V, B, S)
    d_ntok, d_ban = torch.from_numpy(ntok).cuda(), hip.ban_bits(ban, V, "cuda")
    runs = [(use_ban, rep, min_id) for use_ban in (True, False) for rep, min_id in ((True, 0), (False, 7))]
    wants = {r: pick_np(x, n, ban if r[0] else (), r[1], r[2], pad=2, old=old) for r in runs}
    live = np.arange(S)[None, :] < n[:, None]
    for off in (0, 1, 2, 3):
        dx = _at_offset(x.reshape(B * S, V), off)
        for use_ban, rep, min_id in runs:
            want, what = wants[(use_ban, rep, min_id)], (V, off, use_ban, rep, min_id)
            seq = torch.from_numpy(old.copy()).cuda().view(-1)
            chosen = torch.full((B * S,), KEEP, dtype=torch.float32, device="cuda")
            changed = torch.full((B,), -1, dtype=torch.int32, device="cuda")
            hip.vocab_constrain(dx, V, S, seq, ntok=d_ntok, ntok_bias=-1, pad_idx=2, ban=d_ban if use_ban else None, no_repeat=rep, repeat_min_id=min_id,
                                row_chosen=chosen, changed=changed)
            torch.cuda.synchronize()
            assert np.array_equal(seq.cpu().numpy().reshape(B, S), want["seq"]), what
            expect = np.where(live, want["chosen"], np.float32(KEEP)).astype(np.float32)
            assert np.array_equal(chosen.cpu().numpy().reshape(B, S).view(np.int32), expect.view(np.int32)), what
            assert np.array_equal(changed.cpu().numpy(), want["changed"]), what


BIG_V = 262177                                 # (V + 31) / 32 = 8 194 words: more than the 8 192 the candidate kernels stage in LDS


@functools.lru_cache(maxsize=None)
def _big_ban_case():
    """(x [1, 2, BIG_V], ban, old): Gaussian rows; a few thousand ids banned, each row's best id among them."""
    rng = np.random.default_rng(7800)
    x = rng.standard_normal((1, 2, BIG_V)).astype(np.float32)
    ban = sorted(set(rng.choice(BIG_V, 3000, replace=False).tolist()) | {int(x[0, 0].argmax()), int(x[0, 1].argmax())})
    return x, ban, rng.integers(0, BIG_V, (1, 2)).astype(np.int64)


def test_kernel_reads_a_long_ban_table_through_the_cache():
    """A ban table of 8 194 words is not staged: the candidates launch looks the bits up in global memory.  Bit for bit against pick_np."""
    from boficap_amd import hip
    x, ban, old = _big_ban_case()
    assert (BIG_V + 31) // 32 > 8192
    want = pick_np(x, [2], ban, True, 7, pad=2, old=old)
    assert not set(want["seq"].ravel().tolist()) & set(ban) and (want["seq"] != x.argmax(2)).all()
    dx = torch.from_numpy(x.reshape(2, BIG_V)).cuda()
    seq = torch.from_numpy(old.copy()).cuda().view(-1)
    chosen = torch.full((2,), KEEP, dtype=torch.float32, device="cuda")
    changed = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    hip.vocab_constrain(dx, BIG_V, 2, seq, pad_idx=2, ban=hip.ban_bits(ban, BIG_V, "cuda"), no_repeat=True, repeat_min_id=7, row_chosen=chosen, changed=changed)
    torch.cuda.synchronize()
    assert np.array_equal(seq.cpu().numpy().reshape(1, 2), want["seq"])
    assert np.array_equal(chosen.cpu().numpy().reshape(1, 2).view(np.int32), want["chosen"].view(np.int32))
    assert np.array_equal(changed.cpu().numpy(), want["changed"])


# ----------------------------------------------------------------------------- 2. the float32 engine against the restated decode
@pytest.fixture(scope="module")
def f32_engines():
    from boficap_amd.engine import BofiEngine
    cache = {}

    def get(name):
        base = plain_of(name)
        key = id(base["sd"])
        if key not in cache:
            e = BofiEngine(base["cfg"], torch.float32, max_batch=64, max_regions=36)
            e.load_state_dict(base["sd"])
            cache[key] = e
        return cache[key]
    return get


@pytest.mark.parametrize("T", [0, 1])
@pytest.mark.parametrize("name", ["tiny_saic_multi", "full_b8"])
def test_f32_engine_equals_the_restated_decode(name, T, f32_engines):
    """Strict Q1, all three variants (ban the plain decode's most frequent id / no_repeat / both), T feed-back rounds with the constrained ids fed back.  The layout is the
    plain decode's; on every SAFE image (every decision of its scan, all passes, has a margin above 1e-3 in the restatement's own run) seq and the counts are equal
    and row_chosen is within the float32 log-prob bar of the mask-predict and refinement tests."""
    BAR = 1e-3
    base = plain_of(name)
    eng = f32_engines(name)
    att = base["att"].cuda()
    att_len = None if base["masks"] is None else base["masks"].sum(1).to(torch.int32).cuda()
    plain = _clone(eng.decode_naic(att, att_len, refine_rounds=T, row_stats=True))
    worst = 0.0
    for variant, (ban_on, rep_on) in VARIANTS.items():
        ref = restate(name, variant)[T]
        r = eng.decode_naic(att, att_len, refine_rounds=T, row_stats=True, ban_ids=[base["top_id"]] if ban_on else None, no_repeat=rep_on)
        torch.cuda.synchronize()
        for k in LAYOUT:
            assert torch.equal(r[k].cpu(), base[k]) and torch.equal(r[k], plain[k]), (variant, k)
        safe = ref["safe"]
        assert (T == 0 and safe.all()) or int((~safe).sum()) <= 1
        assert np.array_equal(r["seq"].cpu().numpy()[safe], ref["seq"][safe]), variant
        assert np.array_equal(r["constrained"].cpu().numpy()[safe], ref["changed"][safe]), variant
        live = (np.arange(base["cfg"].seq_length)[None, :] < base["n"][:, None]) & safe[:, None]
        err = float(np.abs(np.nan_to_num(r["row_chosen"].cpu().numpy() - ref["chosen"]))[live].max())
        lp_err = float((r["seq_logprob"].cpu() - torch.from_numpy(ref["lp"])).nan_to_num().abs()[torch.from_numpy(safe)].max())
        print(f"constrained pick {name} {variant} T={T}: |row_chosen - restatement| max {err:.3e}, |seq_logprob - restatement| max {lp_err:.3e}; safe images {int(safe.sum())} of "
              f"{len(safe)}; {int(ref['changed'].sum())} positions changed")
        worst = max(worst, err)
        assert err < BAR and lp_err < BAR, variant
        assert torch.equal(_bits(r["row_plogp"].nan_to_num()), _bits(plain["row_plogp"].nan_to_num())) or T > 0      # (a figure of the distribution: the epilogue's, untouched)
        assert not torch.equal(r["seq"], plain["seq"])
    record_parity(f"constrained_pick_f32_row_chosen_{name}_T{T}", worst, BAR, "float32 engine, row_chosen of a constrained decode, against the restatement on the oracle")


# ----------------------------------------------------------------------------- 3. the bf16 engine, without a tolerance
@pytest.fixture(scope="module")
def bf16_full(weight_cache, manifest):
    """The full-size bf16 engine on full_b8's weights and 16 synthetic images."""
    from boficap_amd import weights as W
    from boficap_amd.engine import BofiEngine
    m = manifest["full_b8"]
    cfg, sd = weight_cache(m["config"], m["seed"], m["gen_scale"], m["digest"], m.get("patch"))
    eng = BofiEngine(cfg, torch.bfloat16, max_batch=64, max_regions=36)
    eng.load_state_dict(sd)
    att = torch.from_numpy(W.synthetic_att_feats(16, 36, cfg.att_feat_size, seed=77)).cuda().to(torch.bfloat16)
    plain = _clone(eng.decode_naic(att, row_stats=True))        # (before any constrained call on this engine)
    torch.cuda.synchronize()
    live = plain["seq"][plain["seq"] >= 7]
    ids, counts = torch.unique(live, return_counts=True)
    return cfg, eng, att, plain, int(ids[counts.argmax()])


def _holds_the_rule(cfg, r, ban, rep, min_id=7):
    """seq, row_chosen and constrained of ``r`` equal pick_np on r's own seq_logprob, bit for bit."""
    S = cfg.seq_length
    lp = r["seq_logprob"].cpu().numpy()
    n = r["phrase_length"].sum(1).cpu().numpy()
    want = pick_np(lp, n, ban, rep, min_id, pad=cfg.pad_idx, old=pick_np(lp, n, pad=cfg.pad_idx)["seq"])
    assert np.array_equal(r["seq"].cpu().numpy(), want["seq"])
    live = np.arange(S)[None, :] < n[:, None]
    assert np.array_equal(r["row_chosen"].cpu().numpy().view(np.int32)[live], want["chosen"].view(np.int32)[live])
    assert np.array_equal(r["constrained"].cpu().numpy(), want["changed"])
    return want


def test_bf16_engine_holds_the_rule_graph_fork_phases_groups(bf16_full):
    cfg, eng, att, plain, top = bf16_full
    kw = dict(row_stats=True, ban_ids=[top], no_repeat=True)
    keys = ("seq", "row_plogp", "row_chosen", "seq_logprob", "constrained") + LAYOUT
    r = _clone(eng.decode_naic(att, **kw))
    torch.cuda.synchronize()
    want = _holds_the_rule(cfg, r, [top], True)
    assert torch.equal(_bits(r["seq_logprob"]), _bits(plain["seq_logprob"]))          # T = 0: the distribution is the plain decode's, bit for bit
    assert torch.equal(_bits(r["row_plogp"]), _bits(plain["row_plogp"])) and _same_bits(r, plain, LAYOUT)
    n = r["phrase_length"].sum(1)
    assert int(want["changed"].sum()) > 0 and not (r["seq"] == top).any()
    inside = torch.arange(1, cfg.seq_length, device="cuda")[None, :] < n[:, None]
    assert not ((r["seq"][:, 1:] == r["seq"][:, :-1]) & (r["seq"][:, 1:] >= 7) & inside).any()
    assert ((plain["seq"][:, 1:] == plain["seq"][:, :-1]) & (plain["seq"][:, 1:] >= 7) & inside).any() and (plain["seq"] == top).any()
    # each rule alone, another floor for the repeats, and one feed-back round (every pass constrained; the last one checked on its own tensor)
    for ban, rep, min_id, T in (([top], False, 7, 0), (None, True, 7, 0), (None, True, 0, 0), ([top], True, 7, 1)):
        q = eng.decode_naic(att, row_stats=True, ban_ids=ban, no_repeat=rep, repeat_min_id=min_id, refine_rounds=T)
        torch.cuda.synchronize()
        _holds_the_rule(cfg, q, ban or (), rep, min_id)
        if T:
            assert not torch.equal(_bits(q["seq_logprob"]), _bits(eng.decode_naic(att, refine_rounds=T)["seq_logprob"]))      # (the constrained ids were fed back)
    # graph: captured, then replayed
    g = eng.decode_naic(att, graph=True, **kw)
    g = eng.decode_naic(att, graph=True, out=g, **kw)
    torch.cuda.synchronize()
    assert _same_bits(g, r, keys)
    # a fork on its own stream (its own workspace and bit table)
    f = eng.fork()
    st = f.stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        fo = f.decode_naic(att, **kw)
    st.synchronize()
    assert _same_bits(fo, r, keys)
    # the phased form: the filling phase owns the launch
    ph = eng.decode_naic(att, phases="e", **kw)
    ph = eng.decode_naic(att, phases="b", out=ph, **kw)
    ph = eng.decode_naic(att, phases="f", out=ph, **kw)
    torch.cuda.synchronize()
    assert _same_bits(ph, r, keys)
    # two batches of 8 in one call: the rule on the call's own tensor
    q1 = eng.decode_naic(att, q1_group=8, **kw)
    torch.cuda.synchronize()
    _holds_the_rule(cfg, q1, [top], True)
    # the filling pass alone on the decode's own layout
    ext, last = O.layout_of(cfg, r)
    eng.encode(att)
    fr = eng.fill_naic(ext.to(torch.int32).cuda(), torch.from_numpy(last).to(torch.int32).cuda(), att.size(1), ban_ids=[top], no_repeat=True)
    torch.cuda.synchronize()
    assert len(fr) == 3 and torch.equal(fr[0], r["seq"]) and torch.equal(fr[2]["constrained"], r["constrained"]) and torch.equal(_bits(fr[1]), _bits(r["seq_logprob"]))
    assert len(eng.fill_naic(ext.to(torch.int32).cuda(), torch.from_numpy(last).to(torch.int32).cuda(), att.size(1))) == 2
    # raw logits: the pick is over logits
    raw = eng.decode_naic(att, raw_logits=True, ban_ids=[top], no_repeat=True)
    torch.cuda.synchronize()
    lg, nn = raw["seq_logprob"].cpu().numpy(), raw["phrase_length"].sum(1).cpu().numpy()
    assert np.array_equal(raw["seq"].cpu().numpy(), pick_np(lg, nn, [top], True, 7, pad=cfg.pad_idx)["seq"])


def test_off_is_todays_decode(bf16_full):
    """No options, an empty ban list and a zero record each give the decode made before any constrained call on this engine, bit for bit, and carry no counts."""
    from boficap_amd import hip
    cfg, eng, att, plain, top = bf16_full
    keys = ("seq", "seq_logprob", "row_plogp", "row_chosen") + LAYOUT
    eng.decode_naic(att, ban_ids=[top], no_repeat=True)         # (a constrained call in between)
    for kw in ({}, {"ban_ids": []}, {"ban_ids": None, "no_repeat": False, "repeat_min_id": 0}):
        r = eng.decode_naic(att, row_stats=True, **kw)
        torch.cuda.synchronize()
        assert _same_bits(r, plain, keys) and "constrained" not in r, kw
    o = eng.decode_naic(att)
    rec = hip.BofiCallOpts()                                    # zero-filled
    rc = hip.lib().bofi_engine_decode_naic(eng._h, hip.ptr(att), hip.dtype_code(att), None, att.size(0), 36, hip.FLAG_STRICT_Q1, hip.ptr(o["seq"]), hip.ptr(o["seq_logprob"]),
                                           hip.ptr(o["phrase_num"]), hip.ptr(o["phrase_length"]), hip.ptr(o["phrase_syn"]), None, hip.ptr(o["bound_iters"]), rec, hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and _same_bits(o, plain, ("seq", "seq_logprob") + LAYOUT)


def test_engine_refuses_what_the_constrained_pick_excludes(bf16_full):
    from boficap_amd import hip
    cfg, eng, att, plain, top = bf16_full
    a = att[:4].contiguous()
    with pytest.raises(hip.BofiHipError, match="ids_only"):
        eng.decode_naic(a, ids_only=True, no_repeat=True)
    with pytest.raises(hip.BofiHipError, match="mask_predict"):
        eng.decode_naic(a, refine_rounds=2, refine_method="mask_predict", ban_ids=[top])
    with pytest.raises(hip.BofiHipError, match="0.."):
        eng.decode_naic(a, ban_ids=[cfg.tgt_vocab])
    with pytest.raises(hip.BofiHipError, match="at least two"):
        eng.decode_naic(a, ban_ids=range(1, cfg.tgt_vocab))
    with pytest.raises(hip.BofiHipError, match="repeat_min_id"):
        eng.decode_naic(a, no_repeat=True, repeat_min_id=-1)
    # the library's own checks, before anything is enqueued
    o = eng.decode_naic(a)
    lib = hip.lib()
    table = hip.ban_bits([top], cfg.tgt_vocab, "cuda")

    def args(flags, rec, lp=True):
        return (eng._h, hip.ptr(a), hip.dtype_code(a), None, 4, 36, flags, hip.ptr(o["seq"]), hip.ptr(o["seq_logprob"]) if lp else None, hip.ptr(o["phrase_num"]),
                hip.ptr(o["phrase_length"]), hip.ptr(o["phrase_syn"]), None, hip.ptr(o["bound_iters"]), rec, hip.stream_ptr())
    on = lambda **kw: hip.BofiCallOpts(**dict(dict(pick_ban=table.data_ptr(), pick_no_repeat=1, pick_repeat_min_id=7), **kw))
    assert lib.bofi_engine_decode_naic(*args(hip.FLAG_IDS_ONLY, on(), lp=False)) == 1 and b"IDS_ONLY" in lib.bofi_last_error()
    assert lib.bofi_engine_decode_naic(*args(hip.FLAG_IDS_ONLY, on(pick_ban=None), lp=False)) == 1
    assert lib.bofi_engine_decode_naic(*args(hip.FLAG_MASK_PREDICT | (2 << 8), on())) == 1 and b"MASK_PREDICT" in lib.bofi_last_error()
    assert lib.bofi_engine_decode_naic(*args(0, on(pick_no_repeat=2))) == 1 and b"pick_no_repeat" in lib.bofi_last_error()
    assert lib.bofi_engine_decode_naic(*args(0, on(pick_repeat_min_id=-1))) == 1 and b"pick_repeat_min_id" in lib.bofi_last_error()
    sa = args(0, on())
    assert lib.bofi_engine_decode_saic(*(sa[:12] + sa[13:])) == 3 and b"semi-autoregressive" in lib.bofi_last_error()
    f = eng.fork(ids_only=True)                                  # a fork without vocabulary buffers never sees the pick: its own refusals come first
    fa = (f._h,) + args(0, on())[1:]
    assert lib.bofi_engine_decode_naic(*fa) == 3
    torch.cuda.synchronize()
    again = eng.decode_naic(a)                                   # nothing was enqueued: the engine decodes as before
    torch.cuda.synchronize()
    assert _same_bits(again, o, ("seq", "seq_logprob"))


# ----------------------------------------------------------------------------- 4. above the engine
def test_interface_gives_the_engine_level_result(weight_cache, monkeypatch):
    """decode_many (a ragged tail batch) and mode='sample' with the reference's option names against BofiEngine.decode_naic on the same batches, same
    kernel family and hint."""
    import captioning.models as models
    from boficap_amd import hip as H, weights as W
    from boficap_amd.engine import BofiEngine
    monkeypatch.setenv("BOFI_RB_MIN_ROWS", "0")                 # one kernel family whatever the launch size (a row's result then does not depend on the launch)
    monkeypatch.setenv("BOFI_BOUND_LOOP", "2")
    H.lib().bofi_reload_env()
    try:
        cfg, sd = weight_cache("FULL", 0, 1.0)
        opt = cfg.to_opt()
        opt.bofi_compute_dtype, opt.bofi_max_batch, opt.bofi_max_regions = torch.bfloat16, 16, 36
        model = models.setup(opt)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        model.cuda().eval()
        feats = torch.from_numpy(W.synthetic_att_feats(16 * 2 + 5, 36, cfg.att_feat_size, seed=79)).to(torch.bfloat16)
        batches = [feats[i:i + 16] for i in range(0, feats.size(0), 16)]       # two batches of 16 and a tail of 5 ...
        tail_masks = torch.ones(5, 36)
        tail_masks[1, 9:] = 0; tail_masks[4, 30:] = 0                           # ... which is ragged
        ref = BofiEngine(cfg, torch.bfloat16, max_batch=16, max_regions=36)
        ref.load_state_dict(sd)
        ref.set_decodes_in_flight(2)
        lens = lambda i: tail_masks.sum(1).to(torch.int32).cuda() if i == 2 else None
        plain = [ref.decode_naic(b.cuda(), lens(i))["seq"].cpu() for i, b in enumerate(batches)]
        live = torch.cat(plain)
        ids, counts = torch.unique(live[live >= 7], return_counts=True)
        top = int(ids[counts.argmax()])
        want = []
        for i, b in enumerate(batches):
            r = ref.decode_naic(b.cuda(), lens(i), row_stats=True, ban_ids=[top], no_repeat=True)
            ent, ppl = ref.entropy_perplexity(r)
            want.append(dict({k: v.cpu() for k, v in r.items() if torch.is_tensor(v)}, entropy=ent.cpu(), perplexity=ppl.cpu()))
        # decode_many
        items = [b.pin_memory() for b in batches[:2]] + [(batches[2].pin_memory(), tail_masks)]
        got = list(model.decode_many(items, batches_per_launch=2, in_flight=2, ban_ids=[top], no_repeat=True))
        assert len(got) == 3
        for i, (g, w) in enumerate(zip(got, want)):
            for k in ("seq", "constrained") + LAYOUT:
                assert torch.equal(g[k], w[k]), (i, k)
            assert g["constrained"].dtype == torch.int32 and torch.equal(g["perplexity"].nan_to_num(), w["perplexity"].nan_to_num()), i
        assert all(not torch.equal(g["seq"], p) for g, p in zip(got, plain)) and sum(int(g["constrained"].sum()) for g in got) > 0
        again = list(model.decode_many(items, batches_per_launch=2, in_flight=2))               # the defaults stay today's decode
        assert all(torch.equal(g["seq"], p) and "constrained" not in g for g, p in zip(again, plain))
        with pytest.raises(H.BofiHipError, match="fused_vocab"):
            list(model.decode_many(items, fused_vocab=True, no_repeat=True))
        # mode='sample' with the reference's names: a vocabulary that maps one id to 'UNK'
        model.vocab = dict(model.vocab)
        model.vocab.update({k: "x" for k, v in model.vocab.items() if v == "UNK"})
        model.vocab[str(top)] = "UNK"
        fc = torch.zeros(5, 0, device="cuda")
        out = model(fc, batches[2].cuda(), tail_masks.cuda(), opt={"train_mode": "NAIC", "suppress_UNK": 1, "decoding_constraint": 1}, mode="sample")
        assert len(out) == 6
        counts_ = model.last_constrained.clone()
        e = model.engine().decode_naic(batches[2].cuda(), lens(2), ban_ids=[top], no_repeat=True)
        torch.cuda.synchronize()
        assert torch.equal(out[0], e["seq"]) and torch.equal(counts_, e["constrained"]) and torch.equal(out[3], e["phrase_length"])
        assert torch.equal(_bits(out[1].nan_to_num()), _bits(e["seq_logprob"].nan_to_num()))
        assert int(counts_.sum()) > 0 and not (out[0] == top).any()
        p6 = model(fc, batches[2].cuda(), tail_masks.cuda(), opt={"train_mode": "NAIC"}, mode="sample")
        assert model.last_constrained is None                    # (a plain call clears it; the reference's defaults, 0 and 0, are the plain decode)
        assert (p6[0] == top).any()
        model.vocab[str(top)] = "x"                              # no UNK in the vocabulary: nothing banned, nothing launched
        model(fc, batches[2].cuda(), tail_masks.cuda(), opt={"train_mode": "NAIC", "suppress_UNK": 1}, mode="sample")
        assert model.last_constrained is None
        for bad in ({"train_mode": "NAIC", "decoding_constraint": 1, "sample_method": "sample"},
                    {"train_mode": "NAIC", "ban_ids": [top], "refine_rounds": 2, "refine_method": "mask_predict"}, {"train_mode": "SAIC", "ban_ids": [top]}):
            with pytest.raises(H.BofiHipError):
                model(fc, batches[2].cuda(), tail_masks.cuda(), opt=bad, mode="sample")
    finally:
        monkeypatch.undo()
        H.lib().bofi_reload_env()


def test_eval_split_reports_constrained_rate():
    from boficap_amd import eval_utils
    from boficap_amd.config import TINY
    from test_gpu_lang_eval import tiny_model
    labels = eval_utils.SyntheticLabels(TINY, 8, 5, seed=3)
    model = tiny_model()
    base = {"batch_size": 4, "language_eval": 1, "verbose_loss": 0}
    _, preds0, stats0 = eval_utils.eval_split(model, labels.feats, labels, dict(base))
    _, preds, stats = eval_utils.eval_split(model, labels.feats, labels, dict(base, decoding_constraint=1))
    assert "constrained_rate" not in stats0 and list(stats)[:-1] == list(stats0) and list(stats)[-1] == "constrained_rate"
    host = torch.from_numpy(labels.feats)
    got = list(model.decode_many([host[i:i + 4] for i in range(0, 8, 4)], no_repeat=True))
    changed, emitted = sum(int(g["constrained"].sum()) for g in got), sum(int(g["phrase_length"].sum()) for g in got)
    assert 0 < changed <= emitted and stats["constrained_rate"] == changed / emitted
    assert [p["seq"] for p in preds] == [[int(v) for v in row.tolist()[:next((q for q, v in enumerate(row.tolist()) if v <= 0), len(row))]] for g in got for row in g["seq"]]
    assert preds != preds0
    for g in got:
        seq, n = g["seq"], g["phrase_length"].sum(1)
        inside = torch.arange(1, seq.size(1))[None, :] < n[:, None]
        assert not ((seq[:, 1:] == seq[:, :-1]) & (seq[:, 1:] >= 7) & inside).any()
    with pytest.raises(ValueError, match="NAIC"):
        eval_utils.eval_split(model, labels.feats, labels, dict(base, inference_mode="SAIC", suppress_UNK=1))
