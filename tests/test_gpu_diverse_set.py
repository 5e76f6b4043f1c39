"""The Hamming-diverse caption set on the MI355X: bofi_vocab_diverse against the numpy restatement (tests/test_diverse_set.py; ids equal, the float64 totals and
augmented values compared as bits), its refusals with live buffers, the float32 and the bf16 engine each held without a tolerance to ``diverse_np`` on the log-probs
the SAME call returned, "off is the decode as it was", the engine's refusals, and the interface above the engine (mode='sample', fill_naic, eval_split)."""
import numpy as np
import pytest
import torch

import boficap_oracle as O
from test_constrained_pick import order_np
from test_diverse_set import diverse_np
from test_gpu_constrained_pick import LAYOUT, _bits, _clone, _same_bits
from test_nbest_no_repeat import is_valid

pytestmark = pytest.mark.gpu

MIN_ID = 7
VP_CUT = 0x7ffffffe                            # in the candidates workspace: the row's order is not known from this entry on
WINDOW8 = [1.0, 1.75, 1.625, 1.5, 1.875, 1.375, 1.25, 1.125]      # a row's eight best values in eight consecutive columns (test_gpu_nbest.py has the argument)
DV_KEYS = ("diverse_seq", "diverse_logp", "diverse_aug", "diverse_count")


# ----------------------------------------------------------------------------- 1. the kernel
def _case(rng, B, S, V, ldx):
    """x [B, S, ldx]: even images on the four-value tie grid {0, -1/8, -2/8, -3/8}, odd images on a grid of eighths in [-8, 0] with every second row a copy of the
    row before it (neighbours share their leaders: the repeat rule bites); poison past column V.  n_b mixes S, 0, S - 1, 1 and random lengths, ntok is read with a bias
    of -1 and clamped from both sides.  Row min(5, S - 1) of image 0 holds its eight best values in eight consecutive columns: the candidates launch cannot settle
    its order and the kernel streams the row again.  With B >= 13: images led by a NaN, by two +inf and by a row of -inf alone (degenerate; S >= 3 there), a row of two finite
    values (-inf at the ranks behind them: fewer candidates than K), an image whose first two rows have one candidate each, the same word (no valid caption under the
    repeat rule), a NaN in a row past n_b (never read)."""
    x = np.empty((B, S, ldx), np.float32)
    for b in range(B):
        x[b] = -rng.integers(0, 4 if b % 2 == 0 else 65, (S, ldx)) / 8.0
        if b % 2:
            for s in range(1, S):
                if s % 2:
                    x[b, s] = x[b, s - 1]
    n = rng.integers(0, S + 1, B)
    n[:4] = [S, 0, max(S - 1, 1), 1][:min(B, 4)]
    ntok = (n + 1).astype(np.int32)
    w0 = 1000 if V > 1008 else 8
    x[0, min(5, S - 1), w0:w0 + 8] = WINDOW8
    if B >= 13:
        ntok[5], n[5] = S + 9, S                                # clamped from above ...
        ntok[6], n[6] = -4, 0                                   # ... and from below
        for b in range(7, 13):
            n[b] = min(S, 3)
            ntok[b] = n[b] + 1
        x[7, 0, V - 2] = np.nan
        x[8, 0, [3, 9]] = np.inf
        x[9, 0, :] = -np.inf
        x[10, 0, :] = -np.inf
        x[10, 0, [V // 3, V // 2]] = -1.5, -0.75
        x[11, :2, :] = -np.inf
        x[11, :2, 8] = -1.0
        n[12], ntok[12] = 1, 2
        x[12, 2, 3] = np.nan                                    # (past n_b: not read)
    x[:, :, V:] = np.inf                                        # a padded pitch: never read
    if ldx > V + 1:
        x[:, :, V + 1] = np.nan
    light = sorted({int(order_np(x[0, 0, :V])[0])} | {int(v) for v in rng.choice(V, 3, replace=False)} - {8})
    heavy = sorted(set(range(V)) - {8, 11, int(order_np(x[0, 0, :V])[1])})      # three ids left: fewer than K
    return x, n, ntok, {"none": (), "light": light, "heavy": heavy}


KERNEL_CASES = [(1, 1, 37, 41, 1, (0.5,)), (3, 5, 37, 41, 2, (0.0, 1e6)), (67, 5, 37, 41, 8, (0.5,)), (67, 20, 37, 41, 2, (0.5,)), (3, 20, 37, 41, 6, (0.5, 1e6)),
                (3, 64, 37, 41, 8, (0.5,)), (3, 20, 9491, 9491, 8, (0.5,))]


@pytest.mark.parametrize("B,S,V,ldx,N,lams", KERNEL_CASES)
def test_kernel_equals_diverse_np(B, S, V, ldx, N, lams):
    """seq_n, total, aug (as bits: NaN and -inf included) and count against ``diverse_np``: both variants (the repeat rule with min(N, 6) groups), without a ban table,
    with one and with one that leaves three ids; ntok read with a bias and clamped; the tensor one float off a 16-byte boundary; x is read only; two calls give the
    same bytes.  With K = 8 the workspace shows that the candidates launch left image 0's window row unsettled inside its first K entries."""
    from boficap_amd import hip
    rng = np.random.default_rng(9300 + 100 * B + S + V + N)
    x, n, ntok, bans = _case(rng, B, S, V, ldx)
    d_ntok = torch.from_numpy(ntok).cuda()
    pad = 3
    buf = torch.full((B * S * ldx + 8,), 7.0, dtype=torch.float32, device="cuda")
    dx = buf[1:1 + B * S * ldx].view(B * S, ldx)                # 4 bytes off the allocation's alignment
    dx.copy_(torch.from_numpy(x.reshape(B * S, ldx)))
    assert dx.data_ptr() % 16 == 4
    seen = dict(degenerate=0, empty=0, differ=0)
    for nr in (False, True):
        Ng = min(N, 6) if nr else N
        K = Ng + 2 if nr else Ng
        for lam in lams:
            for name, ban in bans.items():
                if name != "none" and lam != lams[0]:
                    continue
                what = (B, S, V, ldx, Ng, nr, lam, name)
                want = diverse_np(x[:, :, :V], n, Ng, lam, ban, nr, MIN_ID, pad=pad)
                outs = []
                for _ in range(2):
                    seq_n = torch.full((B, Ng, S), -7, dtype=torch.int64, device="cuda")
                    total = torch.full((B, Ng), 123.0, dtype=torch.float64, device="cuda")
                    aug = torch.full((B, Ng), 321.0, dtype=torch.float64, device="cuda")
                    count = torch.full((B,), -7, dtype=torch.int32, device="cuda")
                    work = torch.full((B * S * 8,), -1, dtype=torch.int32, device="cuda")
                    hip.vocab_diverse(dx, V, S, Ng, lam=lam, no_repeat=nr, repeat_min_id=MIN_ID, ntok=d_ntok, ntok_bias=-1, pad_idx=pad,
                                      ban=hip.ban_bits(ban, V, "cuda") if ban else None, seq_n=seq_n, total=total, aug=aug, count=count, work=work)
                    torch.cuda.synchronize()
                    outs.append((seq_n.cpu().numpy(), total.cpu().numpy().view(np.int64), aug.cpu().numpy().view(np.int64), count.cpu().numpy()))
                got = outs[0]
                assert all(np.array_equal(u, v) for u, v in zip(outs[0], outs[1])), what
                assert np.array_equal(got[3], want["count"]), (what, got[3], want["count"])
                assert np.array_equal(got[0], want["seq"]), what
                assert np.array_equal(got[1], want["total"].view(np.int64)), what
                assert np.array_equal(got[2], want["aug"].view(np.int64)), what
                if K == 8 and name == "none":
                    assert (work.view(B * S, 8)[min(5, S - 1)] == VP_CUT).any(), what      # the kernel re-read that row
                seen["degenerate"] += int(want["degenerate"].sum())
                seen["empty"] += int((want["count"] == 0).sum())
                seen["differ"] += int(sum((want["seq"][b, 1:] != want["seq"][b, :1]).any() for b in range(B)))
                for b in range(B):
                    for g in range(int(want["count"][b])):
                        if nr and not want["degenerate"][b]:
                            assert is_valid(want["seq"][b, g, :n[b]].tolist(), ban, MIN_ID), (what, b, g)
    assert np.array_equal(dx.cpu().numpy().view(np.int32), x.reshape(B * S, ldx).view(np.int32))      # (x is read only)
    print(f"diverse kernel {(B, S, V, ldx, N, lams)}: over the variants {seen['degenerate']} degenerate images, {seen['empty']} without a valid caption, "
          f"{seen['differ']} sets with more than one caption")
    if B >= 13:
        assert seen["degenerate"] and seen["empty"]
    if N > 1 and max(lams) > 0:
        assert seen["differ"]
    # ntok, ban and the buffers left out: every position is live
    for nr in (False, True):
        Ng = min(N, 6) if nr else N
        seq_n, total, aug, count = hip.vocab_diverse(dx, V, S, Ng, lam=lams[0], no_repeat=nr, repeat_min_id=0, pad_idx=pad)
        torch.cuda.synchronize()
        full = diverse_np(x[:, :, :V], np.full(B, S), Ng, lams[0], (), nr, 0, pad=pad)
        assert np.array_equal(seq_n.cpu().numpy(), full["seq"]) and np.array_equal(count.cpu().numpy(), full["count"])
        assert np.array_equal(total.cpu().numpy().view(np.int64), full["total"].view(np.int64)) and np.array_equal(aug.cpu().numpy().view(np.int64), full["aug"].view(np.int64))


def test_entry_point_refuses_with_live_buffers_and_launches_nothing():
    """Every refusal returns BOFI_ERR_ARG with a message "vocab_diverse: ..."; the outputs keep their fill."""
    from boficap_amd import hip
    lib = hip.lib()
    S, V, B, N = 5, 37, 3, 4
    x = torch.zeros(B * S, V, device="cuda")
    seq_n = torch.full((B, 8, S), -7, dtype=torch.int64, device="cuda")
    total = torch.full((B, 8), 123.0, dtype=torch.float64, device="cuda")
    aug = torch.full((B, 8), 321.0, dtype=torch.float64, device="cuda")
    count = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    work = torch.full((B * S * 8,), -1, dtype=torch.int32, device="cuda")
    good = dict(rows=B * S, V=V, ldx=V, S=S, N=N, lam=0.5, nr=0, lo=7, aug=hip.ptr(aug), work=hip.ptr(work), wb=work.numel() * 4)

    def call(**kw):
        a = dict(good, **kw)
        return lib.bofi_vocab_diverse(hip.ptr(x), a["ldx"], a["rows"], a["V"], a["S"], None, 0, 0, None, a["N"], a["lam"], a["nr"], a["lo"], hip.ptr(seq_n), hip.ptr(total),
                                      a["aug"], hip.ptr(count), a["work"], a["wb"], hip.stream_ptr())

    for kw, word in ((dict(N=0), b"N in 1..8"), (dict(N=9), b"N in 1..8"), (dict(N=7, nr=1), b"N in 1..6"), (dict(lam=-0.5), b"lambda"), (dict(lam=float("nan")), b"lambda"),
                     (dict(lam=float("inf")), b"lambda"), (dict(nr=2), b"no_repeat"), (dict(lo=-1), b"repeat_min_id"), (dict(aug=None), b"aug"),
                     (dict(work=None), b"workspace"), (dict(wb=work.numel() * 4 - 1), b"workspace"), (dict(rows=B * S + 1), b"rows"), (dict(S=65, rows=65), b"S in 1..64"),
                     (dict(ldx=V - 1), b"pitch"), (dict(V=1), b"V >= 2")):
        assert call(**kw) == 1, kw
        msg = lib.bofi_last_error()
        assert msg.startswith(b"vocab_diverse: ") and word in msg, (kw, msg)
    torch.cuda.synchronize()
    assert (seq_n == -7).all() and (total == 123.0).all() and (aug == 321.0).all() and (count == -7).all() and (work == -1).all()
    with pytest.raises(hip.BofiHipError, match="float32"):
        hip.vocab_diverse(x.double(), V, S, 3)
    with pytest.raises(hip.BofiHipError, match=r"1\.\.6"):
        hip.vocab_diverse(x, V, S, 7, no_repeat=True)
    with pytest.raises(hip.BofiHipError, match="lambda"):
        hip.vocab_diverse(x, V, S, 3, lam=-1.0)
    assert call() == 0
    torch.cuda.synchronize()
    assert (count == N).all()


# ----------------------------------------------------------------------------- 2. the engines, without a tolerance
@pytest.fixture(scope="module", params=[torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def tiny_engine(request):
    """The TINY engine in float32 / bf16 on 16 synthetic images, with the plain decodes made BEFORE any call with the option on this engine."""
    from boficap_amd import weights as W
    from boficap_amd.config import TINY
    from boficap_amd.engine import BofiEngine
    eng = BofiEngine(TINY, request.param, max_batch=64, max_regions=36)
    eng.load_state_dict(W.make_state_dict(TINY, seed=0, gen_scale=6.0))
    att = torch.from_numpy(W.synthetic_att_feats(16, 36, TINY.att_feat_size, seed=77)).cuda().to(request.param)
    plain = _clone(eng.decode_naic(att, row_stats=True))
    torch.cuda.synchronize()
    live = plain["seq"][plain["seq"] >= 7]
    ids, counts = torch.unique(live, return_counts=True)
    top = int(ids[counts.argmax()])
    before = {"ban": _clone(eng.decode_naic(att, row_stats=True, ban_ids=[top])), "T1": _clone(eng.decode_naic(att, row_stats=True, refine_rounds=1))}
    torch.cuda.synchronize()
    return TINY, eng, att, plain, top, before


def _holds_the_rule(cfg, r, N, lam=0.5, nr=False, ban=(), min_id=MIN_ID):
    """``r`` (a decode with diverse = N): the four outputs equal diverse_np on the log-probs ``r`` itself carries (the float64 values as bits)."""
    lp = r["seq_logprob"].cpu().numpy()
    n = r["phrase_length"].sum(1).cpu().numpy()
    want = diverse_np(lp, n, N, lam, ban, nr, min_id, pad=cfg.pad_idx)
    assert not np.isnan(lp).any() and not want["degenerate"].any()
    assert np.array_equal(r["diverse_count"].cpu().numpy(), want["count"])
    assert np.array_equal(r["diverse_seq"].cpu().numpy(), want["seq"])
    assert np.array_equal(r["diverse_logp"].cpu().numpy().view(np.int64), want["total"].view(np.int64))
    assert np.array_equal(r["diverse_aug"].cpu().numpy().view(np.int64), want["aug"].view(np.int64))
    assert r["diverse_seq"].shape == (lp.shape[0], N, cfg.seq_length) and r["diverse_logp"].dtype == torch.float64 and r["diverse_count"].dtype == torch.int32
    return want


def test_engine_holds_the_rule_and_leaves_the_decode_alone(tiny_engine):
    cfg, eng, att, plain, top, before = tiny_engine
    keys = ("seq", "seq_logprob", "row_plogp", "row_chosen") + LAYOUT
    r = _clone(eng.decode_naic(att, row_stats=True, diverse=4))
    torch.cuda.synchronize()
    want = _holds_the_rule(cfg, r, 4)
    assert _same_bits(r, plain, keys)                           # the decode itself is the plain one ...
    assert torch.equal(r["diverse_seq"][:, 0], r["seq"]) and (r["diverse_count"] == 4).all()      # ... and group 0 is its caption
    assert torch.equal(_bits(r["diverse_aug"][:, 0].contiguous()), _bits(r["diverse_logp"][:, 0].contiguous()))
    differ = int((r["diverse_seq"][:, 1:] != r["diverse_seq"][:, :1]).any(2).any(1).sum())
    print(f"diverse engine {att.dtype}: {differ} of 16 sets hold more than one caption; mean log-prob per group {want['total'].mean(0).tolist()}")
    assert differ
    # the repeat rule, another lambda, N at its limits
    q = eng.decode_naic(att, diverse=6, diversity_lambda=2.0, diverse_no_repeat=True)
    torch.cuda.synchronize()
    w = _holds_the_rule(cfg, q, 6, 2.0, True)
    n = q["phrase_length"].sum(1).cpu().numpy()
    assert all(is_valid(w["seq"][b, g, :n[b]].tolist(), (), MIN_ID) for b in range(16) for g in range(w["count"][b])) and torch.equal(q["seq"], plain["seq"])
    q = eng.decode_naic(att, diverse=8, diversity_lambda=0.0)
    torch.cuda.synchronize()
    _holds_the_rule(cfg, q, 8, 0.0)
    assert (q["diverse_seq"] == q["seq"][:, None]).all()
    q = eng.decode_naic(att, diverse=3, diverse_no_repeat=True, repeat_min_id=0)
    torch.cuda.synchronize()
    _holds_the_rule(cfg, q, 3, 0.5, True, min_id=0)
    # a ban list: the set is made under the call's table; the decode is the constrained one of before
    q = eng.decode_naic(att, row_stats=True, ban_ids=[top], diverse=4)
    torch.cuda.synchronize()
    _holds_the_rule(cfg, q, 4, ban=(top,))
    assert _same_bits(q, before["ban"], keys) and torch.equal(q["constrained"], before["ban"]["constrained"]) and not (q["diverse_seq"] == top).any()
    # one feed-back round: the final pass's rows
    q = eng.decode_naic(att, row_stats=True, refine_rounds=1, diverse=4)
    torch.cuda.synchronize()
    _holds_the_rule(cfg, q, 4)
    assert _same_bits(q, before["T1"], keys)
    # no log-prob tensor asked for: the engine's own workspace is read
    nl = eng.decode_naic(att, want_logprob=False, diverse=4)
    torch.cuda.synchronize()
    assert nl["seq_logprob"] is None and _same_bits(nl, r, DV_KEYS + ("seq",))
    # the filling pass alone on the decode's own layout
    ext, last = O.layout_of(cfg, plain)
    eng.encode(att)
    fr = eng.fill_naic(ext.to(torch.int32).cuda(), torch.from_numpy(last).to(torch.int32).cuda(), att.size(1), diverse=4)
    torch.cuda.synchronize()
    assert len(fr) == 3 and torch.equal(fr[0], r["seq"]) and torch.equal(_bits(fr[1]), _bits(r["seq_logprob"]))
    assert all(torch.equal(fr[2][k], r[k]) if r[k].dtype != torch.float64 else torch.equal(_bits(fr[2][k]), _bits(r[k])) for k in DV_KEYS)


def test_off_is_the_decode_as_it_was(tiny_engine):
    """Without the option no key is added -- also into a reused dict of a call that had it -- and the decode is the one made before any call with the option."""
    cfg, eng, att, plain, top, before = tiny_engine
    keys = ("seq", "seq_logprob", "row_plogp", "row_chosen") + LAYOUT
    used = eng.decode_naic(att, row_stats=True, diverse=3, diverse_no_repeat=True)
    assert all(k in used for k in DV_KEYS)
    for off in (None, 0, False):
        r = eng.decode_naic(att, row_stats=True, diverse=off)
        torch.cuda.synchronize()
        assert _same_bits(r, plain, keys) and not any(k in r for k in DV_KEYS)
    r = eng.decode_naic(att, row_stats=True, out=used)
    torch.cuda.synchronize()
    assert _same_bits(r, plain, keys) and not any(k in r for k in DV_KEYS) and "constrained" not in r and "nbest_seq" not in r


def test_engine_refuses_what_the_option_excludes(tiny_engine):
    from boficap_amd import hip
    cfg, eng, att, plain, top, before = tiny_engine
    a = att[:4].contiguous()
    for kw, word in ((dict(ids_only=True), "ids_only"), (dict(refine_rounds=2, refine_method="mask_predict"), "mask_predict"), (dict(no_repeat=True), "no_repeat"),
                     (dict(block_trigrams=True), "block_trigrams"), (dict(require_ids=[9]), "require_ids"), (dict(require_phrases=[[9, 10]]), "require_"),
                     (dict(require_any=[[[9], [10]]]), "require_"), (dict(nbest=3), "nbest"), (dict(diverse=9), r"1\.\.8"), (dict(diverse=7, diverse_no_repeat=True), r"1\.\.6"),
                     (dict(diversity_lambda=-1.0), "lambda"), (dict(diversity_lambda=float("nan")), "lambda"), (dict(diversity_lambda=float("inf")), "lambda"),
                     (dict(diverse_no_repeat=True, repeat_min_id=-1), "repeat_min_id")):
        with pytest.raises(hip.BofiHipError, match=word) as e:
            eng.decode_naic(a, **dict(dict(diverse=3), **kw))
        assert "diverse" in str(e.value), kw
    with pytest.raises(hip.BofiHipError, match="needs diverse"):
        eng.decode_naic(a, diverse_no_repeat=True)
    with pytest.raises(hip.BofiHipError, match="decode_saic") as e:
        eng.decode_saic(a, diverse=3)
    assert "diverse" in str(e.value)
    with pytest.raises(hip.BofiHipError, match="diverse"):     # an ids-only fork keeps no rows
        eng.fork(ids_only=True).decode_naic(a, want_logprob=False, diverse=3)
    z = torch.zeros(4, cfg.bound_len, dtype=torch.int32, device="cuda")
    one = torch.ones(4, dtype=torch.int32, device="cuda")
    with pytest.raises(hip.BofiHipError, match="needs diverse"):
        eng.fill_naic(z, one, 36, diverse_no_repeat=True)
    with pytest.raises(hip.BofiHipError, match=r"1\.\.6"):
        eng.fill_naic(z, one, 36, diverse=7, diverse_no_repeat=True)
    with pytest.raises(hip.BofiHipError, match="nbest"):
        eng.fill_naic(z, one, 36, diverse=3, nbest=3)
    torch.cuda.synchronize()
    r = eng.decode_naic(att, row_stats=True)                    # nothing was enqueued: the engine decodes as before
    torch.cuda.synchronize()
    assert _same_bits(r, plain, ("seq", "seq_logprob", "row_chosen") + LAYOUT)


# ----------------------------------------------------------------------------- 3. above the engine
def test_sample_mode_gives_the_engine_level_set():
    from boficap_amd import hip as H, weights as W
    from boficap_amd.config import TINY
    from test_gpu_lang_eval import tiny_model
    model = tiny_model().eval()
    att = torch.from_numpy(W.synthetic_att_feats(6, 36, TINY.att_feat_size, seed=81)).cuda()
    masks = torch.ones(6, 36, device="cuda")
    masks[1, 9:] = 0; masks[4, 30:] = 0
    fc = torch.zeros(6, 0, device="cuda")
    plain = model(fc, att, masks, opt={"train_mode": "NAIC"}, mode="sample")
    assert model.last_diverse is None
    out = model(fc, att, masks, opt={"train_mode": "NAIC", "diverse": 4, "diversity_lambda": 0.3, "diverse_no_repeat": 1}, mode="sample")
    assert len(out) == 6 and sorted(model.last_diverse) == ["aug", "count", "logp", "seq"] and model.last_nbest is None
    last = {k: v.clone() for k, v in model.last_diverse.items()}
    e = model.engine().decode_naic(att, masks.sum(1).to(torch.int32), diverse=4, diversity_lambda=0.3, diverse_no_repeat=True)
    torch.cuda.synchronize()
    assert torch.equal(out[0], e["seq"]) and torch.equal(out[0], plain[0]) and torch.equal(_bits(out[1]), _bits(plain[1]))
    assert torch.equal(last["seq"], e["diverse_seq"]) and torch.equal(last["count"], e["diverse_count"])
    assert torch.equal(_bits(last["logp"]), _bits(e["diverse_logp"])) and torch.equal(_bits(last["aug"]), _bits(e["diverse_aug"]))
    assert last["seq"].shape == (6, 4, TINY.seq_length)
    _holds_the_rule(TINY, e, 4, 0.3, True)
    model(fc, att, masks, opt={"train_mode": "NAIC", "diverse": 3}, mode="sample")      # the reference's default lambda
    d = model.engine().decode_naic(att, masks.sum(1).to(torch.int32), diverse=3, diversity_lambda=0.5)
    torch.cuda.synchronize()
    assert torch.equal(model.last_diverse["seq"], d["diverse_seq"]) and torch.equal(_bits(model.last_diverse["aug"]), _bits(d["diverse_aug"]))
    for bad, word in (({"diverse": 0}, "needs"), ({"diverse": 7}, r"1\.\.6"), ({"decoding_constraint": 1}, "decoding_constraint"), ({"block_trigrams": 1}, "block_trigrams"),
                      ({"sample_method": "sample"}, "sample_method"), ({"nbest": 3}, "nbest"), ({"diversity_lambda": -2}, "lambda"), ({"train_mode": "SAIC"}, "NAIC"),
                      ({"refine_rounds": 1, "refine_method": "mask_predict"}, "mask_predict"), ({"require_ids": [9]}, "require_ids"), ({"group_size": 2}, "beam")):
        with pytest.raises((H.BofiHipError, NotImplementedError), match=word):
            model(fc, att, masks, opt=dict({"train_mode": "NAIC", "diverse": 3, "diverse_no_repeat": 1}, **bad), mode="sample")
    again = model(fc, att, masks, opt={"train_mode": "NAIC"}, mode="sample")
    assert model.last_diverse is None and torch.equal(again[0], plain[0]) and torch.equal(_bits(again[1]), _bits(plain[1]))


def test_eval_split_takes_the_set_for_its_n_captions(tmp_path):
    from boficap_amd import eval_utils
    from boficap_amd.config import TINY
    from boficap_amd.diversity import KEYS as DIV_KEYS, DiversityEval
    from test_cider import synthetic_corpus, write_df_pickle
    from test_gpu_lang_eval import tiny_model
    path = str(tmp_path / "tiny-idxs.p")
    write_df_pickle(path, synthetic_corpus(200, seed=4, vocab=64, lengths=(3, 20)))
    labels = eval_utils.SyntheticLabels(TINY, 8, 5, seed=3)
    model = tiny_model()
    base = {"batch_size": 4, "language_eval": 1, "cached_tokens": path, "verbose_loss": 0, "eval_oracle": 1}
    kw = dict(base, sample_n=3, sample_n_method="diverse", diversity_lambda=1e6)
    _, predictions, stats = eval_utils.eval_split(model, labels.feats, labels, kw)
    preds_n = kw["preds_n"]
    assert len(preds_n) == 24 and [p["image_id"] for p in preds_n] == [j // 3 for j in range(24)]
    assert all(set(p) == {"image_id", "seq", "logp"} for p in preds_n)
    assert all(k in stats for k in DIV_KEYS) and any(k.startswith("oracle_") for k in stats)
    assert stats["diverse_short"] == kw["diverse_short"] == sum(1 for i in range(8) if preds_n[3 * i + 2]["logp"] == -np.inf)      # (an image without a live position has one caption)
    # the set is the engine's on the same images; caption 0 of every image is the greedy prediction
    e = model.engine().decode_naic(torch.from_numpy(labels.feats[:4]).cuda(), diverse=3, diversity_lambda=1e6)
    torch.cuda.synchronize()
    assert [p["logp"] for p in preds_n[:12]] == e["diverse_logp"].reshape(-1).cpu().tolist()
    rows_e = e["diverse_seq"].reshape(12, -1).cpu().numpy()
    for j in range(12):
        row = rows_e[j].tolist()
        stop = next((i for i, v in enumerate(row) if v <= 0), len(row))
        assert preds_n[j]["seq"] == row[:stop]
    assert [preds_n[3 * i]["seq"] for i in range(8)] == [p["seq"] for p in predictions]
    # the statistics are those of exactly these rows
    rows = np.zeros((24, TINY.seq_length), dtype=np.int64)
    for j, p in enumerate(preds_n):
        rows[j, :len(p["seq"])] = p["seq"]
    div = DiversityEval(path, torch.device("cuda")).evaluate(torch.from_numpy(rows).cuda(), 3)
    assert all(div[k] == stats[k] for k in DIV_KEYS)
    # with a lambda above any spread of a row every position differs between the groups: Div-1 is not below the N-best list's on the same images
    kw_n = dict(base, sample_n=3, sample_n_method="nbest")
    _, predictions_n, stats_n = eval_utils.eval_split(model, labels.feats, labels, kw_n)
    print(f"eval_split: Div-1 {stats['Div-1']:.4f} (diverse, lambda 1e6) against {stats_n['Div-1']:.4f} (nbest); Div-2 {stats['Div-2']:.4f} against {stats_n['Div-2']:.4f}")
    assert stats["Div-1"] >= stats_n["Div-1"] and [p["seq"] for p in predictions] == [p["seq"] for p in predictions_n]
    # the repeat rule and the refusals
    kw_r = dict(base, sample_n=3, sample_n_method="diverse", diverse_no_repeat=1)
    eval_utils.eval_split(model, labels.feats, labels, kw_r)
    assert all(is_valid(p["seq"], (), MIN_ID) for p in kw_r["preds_n"])
    for bad, word in ((dict(sample_n=9), "at most 8"), (dict(sample_n=7, diverse_no_repeat=1), "at most 6"), (dict(decoding_constraint=1), "decoding_constraint"),
                      (dict(inference_mode="SAIC"), "NAIC"), (dict(diversity_lambda=-1), "diversity_lambda"), (dict(require_words="dog"), "require_words")):
        with pytest.raises(ValueError, match=word):
            eval_utils.eval_split(model, labels.feats, labels, dict(kw, **bad))
    with pytest.raises(ValueError, match="diverse_no_repeat"):
        eval_utils.eval_split(model, labels.feats, labels, dict(base, sample_n=3, diverse_no_repeat=1))
