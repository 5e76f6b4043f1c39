"""The N most probable captions of the filling pass on the MI355X: bofi_vocab_nbest against the numpy restatement (tests/test_nbest.py; bit for bit, the float64 totals
compared as bits), the prefix property on the device, the float32 and the bf16 engine each held without a tolerance to ``nbest_np`` on the log-probs the SAME call
returned (ban list, feed-back round, filling pass alone, fork, graph replay, raw logits, no log-prob tensor), "off is today's decode", the refusals, and the interface
above the engine (mode='sample', eval_split)."""
import numpy as np
import pytest
import torch

import boficap_oracle as O
from test_constrained_pick import NAN, order_np
from test_gpu_constrained_pick import LAYOUT, _bits, _clone, _same_bits
from test_nbest import nbest_np

pytestmark = pytest.mark.gpu

VP_CUT = 0x7ffffffe                            # in the candidates workspace: the row's order is not known from this entry on
WINDOW = 1000                                  # the first of the eight consecutive columns of the re-read case


# ----------------------------------------------------------------------------- 1. the kernel
def _kernel_case(rng, B, S, V, ldx, N):
    """x [B, S, ldx]: a floor on a grid of eighths in [-8, -4], a dozen leaders per row on a coarse grid in [-0.5, 0] (ties among a row's best, so ties among the
    totals), -inf sprinkled in, poison past column V.  With B >= 5: images of 0 and of 1 live positions, ntok clamped from above and from below, an image whose one live
    row has two finite values (count < N), images led by a NaN or a +inf (degenerate), NaNs in rows past n_b (never read).  With V > WINDOW + 8: row 5 of image 0 has its
    eight best values in columns WINDOW .. WINDOW + 7 (the re-read)."""
    x = (-4.0 - rng.integers(0, 33, (B, S, ldx)) / 8.0).astype(np.float32)
    lead = np.array([0.0, -0.0, -0.125, -0.25, -0.25, -0.5], np.float32)
    for b in range(B):
        for s in range(S):
            cols = rng.choice(V, min(V, 12), replace=False)
            x[b, s, cols] = lead[rng.integers(0, len(lead), len(cols))]
    x[rng.random((B, S, ldx)) < 0.01] = -np.inf
    n = rng.integers(2, S + 1, B)
    n[0] = S
    ntok = (n + 1).astype(np.int32)                             # the engine's form: `last` with a bias of -1
    if B >= 5:
        n[1], ntok[1] = 0, 1
        n[2], ntok[2] = 1, 2
        n[3], ntok[3] = S, S + 9                                # clamped from above ...
        n[4], ntok[4] = 0, -4                                   # ... and from below
        x[2, 0, :] = -np.inf
        x[2, 0, [V // 3, V // 2]] = -1.5, -0.75                 # two candidates: count = min(N, 2)
        x[2, 5, 3] = NAN                                        # (past n_b: not read)
        x[1, 0, 0] = NAN
        x[3, 7, V - 2] = NAN                                    # a NaN leads a live row: degenerate
        for b in range(5, B, 10):
            x[b, 1, int(rng.integers(0, V))] = np.inf           # a +inf leads a live row: degenerate
        for b in range(7, B, 10):                               # one live row of two finite values, tied
            n[b], ntok[b] = 1, 2
            x[b, 0, :] = -np.inf
            x[b, 0, [1, V - 1]] = -0.25
    if V > WINDOW + 8:                                          # the 8th best in the window's first column, the 7th in its last: whichever quad a lane holds whole,
        x[0, 5, WINDOW:WINDOW + 8] = [1.0, 1.75, 1.625, 1.5, 1.875, 1.375, 1.25, 1.125]      # its fourth entry stands in front of the row's eighth
    x[:, :, V:] = np.inf                                        # a padded pitch: never read
    if ldx > V + 1:
        x[:, :, V + 1] = NAN
    ban = sorted({int(order_np(x[0, 0, :V])[0])} | {int(v) for v in rng.choice(min(V, 900), 3, replace=False)})
    return x, n, ntok, ban


KERNEL_CASES = [(1, 20, 64, 64, 1), (5, 20, 9491, 9491, 5), (3, 64, 9491, 9600, 8), (130, 20, 257, 257, 3)]


@pytest.mark.parametrize("B,S,V,ldx,N", KERNEL_CASES)
def test_kernel_equals_nbest_np(B, S, V, ldx, N):
    """seq_n, total (as bits: NaN and -inf included) and count against ``nbest_np``, with and without a ban table; ntok read with a bias and clamped; for the small-B
    shapes the tensor 0..3 floats off a 16-byte boundary; x is read only; ntok and ban left out.

    The re-read (the case V = 9 491, N = 8): row 5 of image 0 holds its eight best values in columns 1000..1007.  ``vk_stream`` peels a row to its first 16-byte
    boundary and then gives every lane whole aligned groups of four consecutive floats; eight consecutive columns contain at least one whole such group whatever the
    row's alignment (0..3 floats off: the groups 1000-1003 and 1004-1007, or 1001-1004, 1002-1005, 1003-1006).  That lane's list of VP_L = 4 is full of the row's
    best eight, so its fourth entry carries the mark "this lane may hold more", and the candidates launch writes VP_CUT behind that entry's place in the merged
    order.  The values are laid out so that the whole group never ends in the row's eighth best (the 8th stands in column 1000, the 7th in 1007): the cut falls
    inside the first 8 entries, which the test reads back from the workspace, and the merge kernel must stream the row again (``vk_row_behind``) to be right."""
    from boficap_amd import hip
    rng = np.random.default_rng(9000 + 100 * B + S + V + N)
    x, n, ntok, ban = _kernel_case(rng, B, S, V, ldx, N)
    d_ntok, d_ban = torch.from_numpy(ntok).cuda(), hip.ban_bits(ban, V, "cuda")
    pad = 3
    wants = {use_ban: nbest_np(x[:, :, :V], n, N, ban if use_ban else (), pad) for use_ban in (False, True)}
    w = wants[False]
    short = (w["count"] < N) & ~w["degenerate"]
    print(f"n-best kernel {(B, S, V, ldx, N)}: {int(w['tie'].sum())} of {B} images with tied totals, {int(w['degenerate'].sum())} degenerate, {int(short.sum())} with "
          f"count < N; {int((wants[True]['seq'] != w['seq']).sum())} ids differ under the ban")
    if B >= 5:
        assert w["tie"].any() and w["degenerate"].any() and short.any()
        assert (wants[True]["seq"] != w["seq"]).any()
    reread = V > WINDOW + 8 and N == 8
    for off in ((0, 1, 2, 3) if B <= 5 else (0,)):
        buf = torch.full((B * S * ldx + 8,), 7.0, dtype=torch.float32, device="cuda")
        dx = buf[off:off + B * S * ldx].view(B * S, ldx)
        dx.copy_(torch.from_numpy(x.reshape(B * S, ldx)))
        for use_ban, want in wants.items():
            what = (B, S, V, ldx, N, off, use_ban)
            seq_n = torch.full((B, N, S), -7, dtype=torch.int64, device="cuda")
            total = torch.full((B, N), 123.0, dtype=torch.float64, device="cuda")
            count = torch.full((B,), -7, dtype=torch.int32, device="cuda")
            work = torch.full((B * S * 8,), -1, dtype=torch.int32, device="cuda")
            hip.vocab_nbest(dx, V, S, N, ntok=d_ntok, ntok_bias=-1, pad_idx=pad, ban=d_ban if use_ban else None, seq_n=seq_n, total=total, count=count, work=work)
            torch.cuda.synchronize()
            assert np.array_equal(count.cpu().numpy(), want["count"]), what
            assert np.array_equal(seq_n.cpu().numpy(), want["seq"]), what
            assert np.array_equal(total.cpu().numpy().view(np.int64), want["total"].view(np.int64)), what
            if reread:
                assert (work.view(B * S, 8)[5] == VP_CUT).any(), what      # the candidates launch could not settle that row's first 8: the merge re-read it
        assert np.array_equal(dx.cpu().numpy().view(np.int32), x.reshape(B * S, ldx).view(np.int32))      # (x is read only)
    # ntok, ban and the buffers left out: every position is live
    seq_n, total, count = hip.vocab_nbest(dx, V, S, N, pad_idx=pad)
    torch.cuda.synchronize()
    full = nbest_np(x[:, :, :V], np.full(B, S), N, (), pad)
    assert np.array_equal(seq_n.cpu().numpy(), full["seq"]) and np.array_equal(count.cpu().numpy(), full["count"])
    assert np.array_equal(total.cpu().numpy().view(np.int64), full["total"].view(np.int64))


def test_first_entries_of_the_8_list_are_the_3_list_on_the_device():
    from boficap_amd import hip
    B, S, V, ldx = 8, 20, 9491, 9491
    rng = np.random.default_rng(77)
    x, n, ntok, ban = _kernel_case(rng, B, S, V, ldx, 8)
    x[:, :, :V] += (rng.random((B, S, V)) * 1e-3).astype(np.float32)      # off the grid: every float64 add of the totals rounds
    dx, d_ntok = torch.from_numpy(x.reshape(B * S, ldx)).cuda(), torch.from_numpy(ntok).cuda()
    s8, t8, c8 = hip.vocab_nbest(dx, V, S, 8, ntok=d_ntok, ntok_bias=-1)
    s3, t3, c3 = hip.vocab_nbest(dx, V, S, 3, ntok=d_ntok, ntok_bias=-1)
    torch.cuda.synchronize()
    assert torch.equal(s8[:, :3], s3) and torch.equal(t8[:, :3].contiguous().view(torch.int64), t3.view(torch.int64)) and torch.equal(c8.clamp(max=3), c3)
    assert int((c8 == 8).sum()) >= 2


# ----------------------------------------------------------------------------- 2. the engines, without a tolerance
@pytest.fixture(scope="module", params=[torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def tiny_engine(request):
    """The TINY engine in float32 / bf16 on 16 synthetic images, with the plain decodes made BEFORE any call with nbest on this engine."""
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


def _holds_the_rule(cfg, r, N, ban=(), lp=None):
    """``r`` (a decode with nbest = N): nbest_seq, nbest_logp (as bits) and nbest_count equal nbest_np on the log-probs ``r`` itself carries; entry 0 is r's own seq."""
    lp = (r["seq_logprob"] if lp is None else lp).cpu().numpy()
    n = r["phrase_length"].sum(1).cpu().numpy()
    want = nbest_np(lp, n, N, ban, cfg.pad_idx)
    assert not np.isnan(lp).any() and not want["degenerate"].any()
    assert np.array_equal(r["nbest_count"].cpu().numpy(), want["count"])
    assert np.array_equal(r["nbest_seq"].cpu().numpy(), want["seq"])
    assert np.array_equal(r["nbest_logp"].cpu().numpy().view(np.int64), want["total"].view(np.int64))
    assert r["nbest_seq"].shape == (lp.shape[0], N, cfg.seq_length) and r["nbest_logp"].dtype == torch.float64 and r["nbest_count"].dtype == torch.int32
    assert torch.equal(r["nbest_seq"][:, 0], r["seq"])
    return want


NB_KEYS = ("nbest_seq", "nbest_logp", "nbest_count")


def test_engine_holds_the_rule_ban_feedback_fill_fork_graph_raw(tiny_engine):
    cfg, eng, att, plain, top, before = tiny_engine
    keys = ("seq", "seq_logprob", "row_plogp", "row_chosen") + LAYOUT
    r = _clone(eng.decode_naic(att, row_stats=True, nbest=5))
    torch.cuda.synchronize()
    want = _holds_the_rule(cfg, r, 5)
    assert _same_bits(r, plain, keys)                           # the decode itself is the plain one
    print(f"n-best engine {att.dtype}: counts {want['count'].tolist()}, {int(want['tie'].sum())} of 16 images with tied totals")
    assert (want["count"][r["phrase_length"].sum(1).cpu().numpy() >= 2] == 5).all()
    r8 = eng.decode_naic(att, nbest=8)
    torch.cuda.synchronize()
    _holds_the_rule(cfg, r8, 8)
    assert torch.equal(r8["nbest_seq"][:, :5], r["nbest_seq"]) and torch.equal(_bits(r8["nbest_logp"][:, :5].contiguous()), _bits(r["nbest_logp"]))
    # a ban list: the list is made under the call's table, and entry 0 is the constrained caption
    q = eng.decode_naic(att, row_stats=True, ban_ids=[top], nbest=5)
    torch.cuda.synchronize()
    _holds_the_rule(cfg, q, 5, (top,))
    assert _same_bits(q, before["ban"], keys) and torch.equal(q["constrained"], before["ban"]["constrained"]) and not (q["nbest_seq"] == top).any()
    # one feed-back round: the final pass's rows
    q = eng.decode_naic(att, row_stats=True, refine_rounds=1, nbest=5)
    torch.cuda.synchronize()
    _holds_the_rule(cfg, q, 5)
    assert _same_bits(q, before["T1"], keys)
    # graph: captured, then replayed; the two launches stay outside the graph, and the reused dict's buffers are written again
    g = eng.decode_naic(att, row_stats=True, graph=True, nbest=5)
    g["nbest_seq"].fill_(-1)
    g = eng.decode_naic(att, row_stats=True, graph=True, out=g, nbest=5)
    torch.cuda.synchronize()
    assert _same_bits(g, r, keys + NB_KEYS)
    # a fork on its own stream
    f = eng.fork()
    st = f.stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        fo = f.decode_naic(att, row_stats=True, nbest=5)
    st.synchronize()
    assert _same_bits(fo, r, keys + NB_KEYS)
    # no log-prob tensor asked for: the engine's own workspace is read
    nl = eng.decode_naic(att, want_logprob=False, nbest=5)
    torch.cuda.synchronize()
    assert nl["seq_logprob"] is None and _same_bits(nl, r, NB_KEYS + ("seq",))
    # the phased form: the filling phase owns the launches
    ph = eng.decode_naic(att, phases="e", nbest=5)
    assert "nbest_seq" not in ph
    ph = eng.decode_naic(att, phases="b", out=ph, nbest=5)
    ph = eng.decode_naic(att, phases="f", out=ph, nbest=5)
    torch.cuda.synchronize()
    assert _same_bits(ph, r, NB_KEYS + ("seq",))
    # the filling pass alone on the decode's own layout
    ext, last = O.layout_of(cfg, plain)
    eng.encode(att)
    fr = eng.fill_naic(ext.to(torch.int32).cuda(), torch.from_numpy(last).to(torch.int32).cuda(), att.size(1), nbest=5)
    torch.cuda.synchronize()
    assert len(fr) == 3 and torch.equal(fr[0], r["seq"]) and torch.equal(_bits(fr[1]), _bits(r["seq_logprob"]))
    assert all(torch.equal(fr[2][k], r[k]) if k != "nbest_logp" else torch.equal(_bits(fr[2][k]), _bits(r[k])) for k in NB_KEYS)
    # raw logits: the totals are sums of logits
    raw = eng.decode_naic(att, raw_logits=True, nbest=4)
    torch.cuda.synchronize()
    _holds_the_rule(cfg, raw, 4)
    assert torch.equal(raw["nbest_seq"][:, 0], r["seq"])


def test_off_is_the_decode_as_it_was(tiny_engine):
    """nbest None and 0 add no keys and give the outputs of the decodes made before any n-best call on this engine, bit for bit -- also into a reused dict."""
    cfg, eng, att, plain, top, before = tiny_engine
    keys = ("seq", "seq_logprob", "row_plogp", "row_chosen") + LAYOUT
    used = eng.decode_naic(att, row_stats=True, nbest=3)       # (a call with the option in between, and its dict reused below)
    assert "nbest_seq" in used
    for off in (None, 0):
        r = eng.decode_naic(att, row_stats=True, nbest=off)
        torch.cuda.synchronize()
        assert _same_bits(r, plain, keys) and not any(k in r for k in NB_KEYS) and "constrained" not in r
    r = eng.decode_naic(att, row_stats=True, out=used)
    torch.cuda.synchronize()
    assert _same_bits(r, plain, keys) and not any(k in r for k in NB_KEYS)
    r = eng.decode_naic(att, row_stats=True, ban_ids=[top])
    torch.cuda.synchronize()
    assert _same_bits(r, before["ban"], keys) and torch.equal(r["constrained"], before["ban"]["constrained"]) and "nbest_seq" not in r


def test_engine_refuses_what_the_list_excludes(tiny_engine):
    from boficap_amd import hip
    cfg, eng, att, plain, top, before = tiny_engine
    a = att[:4].contiguous()
    for kw, word in ((dict(ids_only=True), "ids_only"), (dict(refine_rounds=2, refine_method="mask_predict"), "mask_predict"), (dict(no_repeat=True), "no_repeat"),
                     (dict(block_trigrams=True), "block_trigrams"), (dict(require_ids=[9]), "require_ids")):
        with pytest.raises(hip.BofiHipError, match=word) as e:
            eng.decode_naic(a, nbest=3, **kw)
        assert "nbest" in str(e.value)
    for bad in (9, -2):
        with pytest.raises(hip.BofiHipError, match="1..8"):
            eng.decode_naic(a, nbest=bad)
    with pytest.raises(hip.BofiHipError, match="decode_saic"):
        eng.decode_saic(a, nbest=3)
    with pytest.raises(hip.BofiHipError, match="ids-only fork"):
        eng.fork(ids_only=True).decode_naic(a, want_logprob=False, nbest=3)
    z = torch.zeros(4, cfg.bound_len, dtype=torch.int32, device="cuda")
    for kw, word in ((dict(refine_rounds=2, refine_method="mask_predict"), "mask_predict"), (dict(no_repeat=True), "no_repeat"), (dict(require_ids=[9]), "require_ids")):
        with pytest.raises(hip.BofiHipError, match=word):
            eng.fill_naic(z, torch.ones(4, dtype=torch.int32, device="cuda"), 36, nbest=3, **kw)
    with pytest.raises(hip.BofiHipError, match="float32"):
        hip.vocab_nbest(torch.zeros(20, 61, dtype=torch.float64, device="cuda"), 61, 20, 3)
    with pytest.raises(hip.BofiHipError, match="1..8"):
        hip.vocab_nbest(torch.zeros(20, 61, device="cuda"), 61, 20, 9)
    torch.cuda.synchronize()
    r = eng.decode_naic(att, row_stats=True)                    # nothing was enqueued: the engine decodes as before
    torch.cuda.synchronize()
    assert _same_bits(r, plain, ("seq", "seq_logprob", "row_chosen") + LAYOUT)


# ----------------------------------------------------------------------------- 3. above the engine
def test_sample_mode_gives_the_engine_level_list():
    from boficap_amd import hip as H, weights as W
    from boficap_amd.config import TINY
    from test_gpu_lang_eval import tiny_model
    model = tiny_model().eval()
    att = torch.from_numpy(W.synthetic_att_feats(6, 36, TINY.att_feat_size, seed=81)).cuda()
    masks = torch.ones(6, 36, device="cuda")
    masks[1, 9:] = 0; masks[4, 30:] = 0
    fc = torch.zeros(6, 0, device="cuda")
    plain = model(fc, att, masks, opt={"train_mode": "NAIC"}, mode="sample")
    assert model.last_nbest is None
    out = model(fc, att, masks, opt={"train_mode": "NAIC", "nbest": 4, "ban_ids": [11]}, mode="sample")
    assert len(out) == 6 and sorted(model.last_nbest) == ["count", "logp", "seq"]
    last = {k: v.clone() for k, v in model.last_nbest.items()}
    e = model.engine().decode_naic(att, masks.sum(1).to(torch.int32), ban_ids=[11], nbest=4)
    torch.cuda.synchronize()
    assert torch.equal(out[0], e["seq"]) and torch.equal(last["seq"], e["nbest_seq"]) and torch.equal(last["count"], e["nbest_count"])
    assert torch.equal(_bits(last["logp"]), _bits(e["nbest_logp"])) and torch.equal(last["seq"][:, 0], out[0]) and last["seq"].shape == (6, 4, TINY.seq_length)
    again = model(fc, att, masks, opt={"train_mode": "NAIC", "nbest": 0}, mode="sample")
    assert model.last_nbest is None and torch.equal(again[0], plain[0]) and torch.equal(_bits(again[1]), _bits(plain[1]))
    for bad, word in (({"sample_method": "sample"}, "sample_method"), ({"refine_rounds": 2, "refine_method": "mask_predict"}, "mask_predict"),
                      ({"decoding_constraint": 1}, "decoding_constraint"), ({"block_trigrams": 1}, "block_trigrams"), ({"require_ids": [12]}, "require_ids"),
                      ({"nbest": 9}, "1..8")):
        with pytest.raises(H.BofiHipError, match=word) as err:
            model(fc, att, masks, opt=dict({"train_mode": "NAIC", "nbest": 3}, **bad), mode="sample")
        assert "nbest" in str(err.value)
    with pytest.raises(H.BofiHipError, match="NAIC"):
        model(fc, att, masks, opt={"train_mode": "SAIC", "nbest": 3}, mode="sample")
    assert torch.equal(model(fc, att, masks, opt={"train_mode": "NAIC"}, mode="sample")[0], plain[0])


def test_eval_split_takes_the_list_for_its_n_captions(tmp_path):
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
    kw = dict(base, sample_n=3, sample_n_method="nbest")
    _, predictions, stats = eval_utils.eval_split(model, labels.feats, labels, kw)
    preds_n = kw["preds_n"]
    assert len(preds_n) == 24 and [p["image_id"] for p in preds_n] == [j // 3 for j in range(24)]
    assert all(set(p) == {"image_id", "seq", "logp"} for p in preds_n)
    for i in range(8):
        lp = [preds_n[3 * i + j]["logp"] for j in range(3)]
        assert lp[0] >= lp[1] >= lp[2] and lp[0] > -np.inf
    assert stats["nbest_short"] == kw["nbest_short"] == sum(1 for i in range(8) if preds_n[3 * i + 2]["logp"] == -np.inf)
    # the list is the engine's on the same images
    e = model.engine().decode_naic(torch.from_numpy(labels.feats[:4]).cuda(), nbest=3)
    torch.cuda.synchronize()
    assert [p["logp"] for p in preds_n[:12]] == e["nbest_logp"].reshape(-1).cpu().tolist()
    # diversity and oracle scores are those of exactly these rows
    rows = np.zeros((24, TINY.seq_length), dtype=np.int64)
    for j, p in enumerate(preds_n):
        rows[j, :len(p["seq"])] = p["seq"]
    again = kw["lang_eval"].evaluate_n(rows, 3)
    assert all(again[k] == stats[k] for k in again if k != "per_image") and any(k.startswith("oracle_") for k in again)
    div = DiversityEval(path, torch.device("cuda")).evaluate(torch.from_numpy(rows).cuda(), 3)
    assert all(div[k] == stats[k] for k in DIV_KEYS)
    # 'sample' behaves as without the key: two fresh models draw the same captions
    kw_a, kw_b = dict(base, sample_n=3, sample_n_method="sample"), dict(base, sample_n=3)
    stats_a = eval_utils.eval_split(tiny_model(), labels.feats, labels, kw_a)[2]
    stats_b = eval_utils.eval_split(tiny_model(), labels.feats, labels, kw_b)[2]
    assert kw_a["preds_n"] == kw_b["preds_n"] and stats_a == stats_b and "nbest_short" not in stats_a and "logp" not in kw_a["preds_n"][0]
    assert [k for k in stats if k != "nbest_short"] == list(stats_a)
    # suppress_UNK / ban_words go with the list; the refusals
    vocab = {str(i): f"w{i}" for i in range(TINY.tgt_vocab)}
    j0 = next(j for j, p in enumerate(preds_n) if p["seq"])
    word = preds_n[j0]["seq"][0]
    kw_c = dict(base, sample_n=3, sample_n_method="nbest", ban_words=f"w{word}", vocab=vocab)
    eval_utils.eval_split(model, labels.feats, labels, kw_c)
    assert all(word not in p["seq"] for p in kw_c["preds_n"]) and kw_c["preds_n"][j0]["seq"] != preds_n[j0]["seq"] and len(kw_c["preds_n"]) == 24
    for bad, word in ((dict(inference_mode="SAIC"), "NAIC"), (dict(decoding_constraint=1), "decoding_constraint"), (dict(sample_n_method="bs"), "'nbest'"),
                      (dict(sample_n=9), "at most 8")):
        with pytest.raises(ValueError, match=word):
            eval_utils.eval_split(model, labels.feats, labels, dict(kw, **bad))
