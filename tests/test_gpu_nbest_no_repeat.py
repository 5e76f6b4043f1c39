"""The N best captions with no adjacent repeated word on the MI355X: bofi_vocab_nbest_norepeat against the numpy restatement (tests/test_nbest_no_repeat.py; bit for
bit, the float64 totals compared as bits), the float32 and the bf16 engine each held without a tolerance to ``nbest_nr_np`` on the log-probs the SAME call returned (ban
list, feed-back round, filling pass alone, fork, graph replay, raw logits, no log-prob tensor), "off is the decode as it was", the refusals, and the interface above the
engine (mode='sample', eval_split)."""
import numpy as np
import pytest
import torch

import boficap_oracle as O
from test_constrained_pick import order_np
from test_gpu_constrained_pick import LAYOUT, _bits, _clone, _same_bits
from test_gpu_nbest import VP_CUT, WINDOW, _kernel_case
from test_nbest_no_repeat import is_valid, nbest_nr_np, sandwich

pytestmark = pytest.mark.gpu

MIN_ID = 7
POOL = np.arange(3, 13)                        # the columns the rows' shared leaders are drawn from: they straddle repeat_min_id = 7


# ----------------------------------------------------------------------------- 1. the kernel
def _case(rng, B, S, V, ldx, N):
    """``test_gpu_nbest._kernel_case`` (its special images: n = 0, n = 1, clamped ntok, NaN and +inf leaders, a two-candidate row, the re-read row) with, on top, four
    leaders per row drawn from the ten columns of POOL -- neighbours share leaders, some of them below repeat_min_id --, and two images appended: the sandwich
    (every listed caption uses ranks 2..7 of its middle row) and an image without any valid caption (count = 0)."""
    x, n, ntok, ban = _kernel_case(rng, B, S, V, ldx, N)
    lead = np.array([0.0, -0.0, -0.125, -0.25, -0.25, -0.5], np.float32)
    for b in range(B):
        for s in range(S):
            if (b == 2 and s == 0 and B >= 5) or (B >= 5 and b >= 7 and (b - 7) % 10 == 0 and s == 0):
                continue                                        # (the rows of two finite values stay)
            cols = rng.choice(POOL, 4, replace=False)
            x[b, s, cols] = lead[rng.integers(0, len(lead), 4)]
    extra = np.full((2, S, ldx), -np.inf, np.float32)
    extra[0, :3, :12] = sandwich()[0][0]
    extra[1, 0, 8] = extra[1, 1, 8] = -1.0                      # two adjacent rows with one candidate each, the same word
    extra[1, 2, :V] = -np.arange(V, dtype=np.float32) / 8.0
    extra[:, :, V:] = x[:1, :1, V:]
    x = np.concatenate([x, extra])
    n = np.concatenate([n, [3, 3]])
    ntok = np.concatenate([ntok, [4, 4]]).astype(np.int32)
    ban = sorted((set(ban) | {int(order_np(x[0, 0, :V])[0])}) - {8, 9, 10})      # (the two appended images keep their words)
    return x, n, ntok, ban


KERNEL_CASES = [(1, 20, 64, 64, 1), (5, 20, 9491, 9491, 5), (3, 64, 9491, 9600, 6), (130, 20, 257, 257, 3)]


@pytest.mark.parametrize("B,S,V,ldx,N", KERNEL_CASES)
def test_kernel_equals_nbest_nr_np(B, S, V, ldx, N):
    """seq_n, total (as bits: NaN and -inf included) and count against ``nbest_nr_np``, with and without a ban table; ntok read with a bias and clamped; for the
    small-B shapes the tensor 0..3 floats off a 16-byte boundary; x is read only.  The rule bites: in some image entry 0 of the plain list (hip.vocab_nbest) repeats a
    word, and no caption of the new list does.  The re-read (V = 9 491, N = 6): row 5 of image 0 holds its eight best values in eight consecutive columns, so the
    candidates launch cuts its order inside the first N + 2 = 8 entries (test_gpu_nbest.py has the argument) and the kernel must stream the row again."""
    from boficap_amd import hip
    rng = np.random.default_rng(9100 + 100 * B + S + V + N)
    x, n, ntok, ban = _case(rng, B, S, V, ldx, N)
    B2 = B + 2
    d_ntok, d_ban = torch.from_numpy(ntok).cuda(), hip.ban_bits(ban, V, "cuda")
    pad = 3
    wants = {use_ban: nbest_nr_np(x[:, :, :V], n, N, ban if use_ban else (), pad, MIN_ID) for use_ban in (False, True)}
    w = wants[False]
    short = (w["count"] < N) & ~w["degenerate"]
    print(f"no-repeat n-best kernel {(B, S, V, ldx, N)}: {int(w['tie'].sum())} of {B2} images with tied totals, {int(w['degenerate'].sum())} degenerate, "
          f"{int(short.sum())} with count < N, {int((w['count'] == 0).sum())} with count 0; {int((wants[True]['seq'] != w['seq']).sum())} ids differ under the ban")
    assert w["count"][B + 1] == 0 and (wants[True]["seq"] != w["seq"]).any()
    if N == 6:
        assert w["seq"][B, :, :3].tolist() == sandwich()[1]
    if B >= 5:
        assert w["tie"].any() and w["degenerate"].any() and short.any()
    reread = V > WINDOW + 8 and N == 6
    for off in ((0, 1, 2, 3) if B <= 5 else (0,)):
        buf = torch.full((B2 * S * ldx + 8,), 7.0, dtype=torch.float32, device="cuda")
        dx = buf[off:off + B2 * S * ldx].view(B2 * S, ldx)
        dx.copy_(torch.from_numpy(x.reshape(B2 * S, ldx)))
        for use_ban, want in wants.items():
            what = (B, S, V, ldx, N, off, use_ban)
            seq_n = torch.full((B2, N, S), -7, dtype=torch.int64, device="cuda")
            total = torch.full((B2, N), 123.0, dtype=torch.float64, device="cuda")
            count = torch.full((B2,), -7, dtype=torch.int32, device="cuda")
            work = torch.full((B2 * S * 8,), -1, dtype=torch.int32, device="cuda")
            hip.vocab_nbest_norepeat(dx, V, S, N, ntok=d_ntok, ntok_bias=-1, pad_idx=pad, ban=d_ban if use_ban else None, repeat_min_id=MIN_ID, seq_n=seq_n, total=total,
                                     count=count, work=work)
            torch.cuda.synchronize()
            assert np.array_equal(count.cpu().numpy(), want["count"]), what
            assert np.array_equal(seq_n.cpu().numpy(), want["seq"]), what
            assert np.array_equal(total.cpu().numpy().view(np.int64), want["total"].view(np.int64)), what
            if reread:
                assert (work.view(B2 * S, 8)[5, :N + 2] == VP_CUT).any(), what      # the candidates launch could not settle that row's first 8: the kernel re-read it
        assert np.array_equal(dx.cpu().numpy().view(np.int32), x.reshape(B2 * S, ldx).view(np.int32))      # (x is read only)
    # the rule bites: the plain list's best caption repeats a word somewhere; no caption of the new list does, and none holds a banned id
    p_seq, _, p_cnt = hip.vocab_nbest(dx, V, S, N, ntok=d_ntok, ntok_bias=-1, pad_idx=pad)
    torch.cuda.synchronize()
    p_seq = p_seq.cpu().numpy()
    repeats = [b for b in range(B2) if not w["degenerate"][b] and not is_valid(p_seq[b, 0, :n[b]].tolist(), (), MIN_ID)]
    print(f"  the plain list's entry 0 repeats a word in {len(repeats)} of {B2} images")
    assert repeats
    for use_ban, want in wants.items():
        for b in range(B2):
            if not want["degenerate"][b]:
                assert all(is_valid(want["seq"][b, j, :n[b]].tolist(), ban if use_ban else (), MIN_ID) for j in range(want["count"][b])), (b, use_ban)
    # ntok, ban and the buffers left out: every position is live; repeat_min_id = 0: every id is a word
    seq_n, total, count = hip.vocab_nbest_norepeat(dx, V, S, N, pad_idx=pad, repeat_min_id=0)
    torch.cuda.synchronize()
    full = nbest_nr_np(x[:, :, :V], np.full(B2, S), N, (), pad, 0)
    assert np.array_equal(seq_n.cpu().numpy(), full["seq"]) and np.array_equal(count.cpu().numpy(), full["count"])
    assert np.array_equal(total.cpu().numpy().view(np.int64), full["total"].view(np.int64))


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
    before = {"ban": _clone(eng.decode_naic(att, row_stats=True, ban_ids=[top])), "T1": _clone(eng.decode_naic(att, row_stats=True, refine_rounds=1)),
              "nbest5": _clone(eng.decode_naic(att, row_stats=True, nbest=5))}
    torch.cuda.synchronize()
    return TINY, eng, att, plain, top, before


def _holds_the_rule(cfg, r, N, ban=(), lp=None, min_id=MIN_ID):
    """``r`` (a decode with nbest = N, nbest_no_repeat): nbest_seq, nbest_logp (as bits) and nbest_count equal nbest_nr_np on the log-probs ``r`` itself carries."""
    lp = (r["seq_logprob"] if lp is None else lp).cpu().numpy()
    n = r["phrase_length"].sum(1).cpu().numpy()
    want = nbest_nr_np(lp, n, N, ban, cfg.pad_idx, min_id)
    assert not np.isnan(lp).any() and not want["degenerate"].any()
    assert np.array_equal(r["nbest_count"].cpu().numpy(), want["count"])
    assert np.array_equal(r["nbest_seq"].cpu().numpy(), want["seq"])
    assert np.array_equal(r["nbest_logp"].cpu().numpy().view(np.int64), want["total"].view(np.int64))
    assert r["nbest_seq"].shape == (lp.shape[0], N, cfg.seq_length) and r["nbest_logp"].dtype == torch.float64 and r["nbest_count"].dtype == torch.int32
    for b in range(lp.shape[0]):
        assert all(is_valid(want["seq"][b, j, :n[b]].tolist(), ban, min_id) for j in range(want["count"][b]))
    return want


NB_KEYS = ("nbest_seq", "nbest_logp", "nbest_count")


def test_engine_holds_the_rule_ban_feedback_fill_fork_graph_raw(tiny_engine):
    cfg, eng, att, plain, top, before = tiny_engine
    keys = ("seq", "seq_logprob", "row_plogp", "row_chosen") + LAYOUT
    r = _clone(eng.decode_naic(att, row_stats=True, nbest=5, nbest_no_repeat=True))
    torch.cuda.synchronize()
    want = _holds_the_rule(cfg, r, 5)
    assert _same_bits(r, plain, keys)                           # the decode itself is the plain one
    n = r["phrase_length"].sum(1).cpu().numpy()
    rep = sum(not is_valid(plain["seq"][b, :n[b]].tolist(), (), MIN_ID) for b in range(16))
    differ = int((r["nbest_seq"] != before["nbest5"]["nbest_seq"]).any(2).any(1).sum())
    print(f"no-repeat n-best engine {att.dtype}: counts {want['count'].tolist()}, {int(want['tie'].sum())} of 16 images with tied totals; the plain caption repeats a "
          f"word in {rep} images, the list differs from the plain list in {differ}")
    r6 = eng.decode_naic(att, nbest=6, nbest_no_repeat=True, repeat_min_id=0)
    torch.cuda.synchronize()
    _holds_the_rule(cfg, r6, 6, min_id=0)
    # a ban list: the list is made under the call's table; the decode is the constrained one of before
    q = eng.decode_naic(att, row_stats=True, ban_ids=[top], nbest=5, nbest_no_repeat=True)
    torch.cuda.synchronize()
    _holds_the_rule(cfg, q, 5, (top,))
    assert _same_bits(q, before["ban"], keys) and torch.equal(q["constrained"], before["ban"]["constrained"]) and not (q["nbest_seq"] == top).any()
    # one feed-back round: the final pass's rows
    q = eng.decode_naic(att, row_stats=True, refine_rounds=1, nbest=5, nbest_no_repeat=True)
    torch.cuda.synchronize()
    _holds_the_rule(cfg, q, 5)
    assert _same_bits(q, before["T1"], keys)
    # graph: captured, then replayed; the two launches stay outside the graph, and the reused dict's buffers are written again
    g = eng.decode_naic(att, row_stats=True, graph=True, nbest=5, nbest_no_repeat=True)
    g["nbest_seq"].fill_(-1)
    g = eng.decode_naic(att, row_stats=True, graph=True, out=g, nbest=5, nbest_no_repeat=True)
    torch.cuda.synchronize()
    assert _same_bits(g, r, keys + NB_KEYS)
    # a fork on its own stream
    f = eng.fork()
    st = f.stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        fo = f.decode_naic(att, row_stats=True, nbest=5, nbest_no_repeat=True)
    st.synchronize()
    assert _same_bits(fo, r, keys + NB_KEYS)
    # no log-prob tensor asked for: the engine's own workspace is read
    nl = eng.decode_naic(att, want_logprob=False, nbest=5, nbest_no_repeat=True)
    torch.cuda.synchronize()
    assert nl["seq_logprob"] is None and _same_bits(nl, r, NB_KEYS + ("seq",))
    # the phased form: the filling phase owns the launches
    ph = eng.decode_naic(att, phases="e", nbest=5, nbest_no_repeat=True)
    assert "nbest_seq" not in ph
    ph = eng.decode_naic(att, phases="b", out=ph, nbest=5, nbest_no_repeat=True)
    ph = eng.decode_naic(att, phases="f", out=ph, nbest=5, nbest_no_repeat=True)
    torch.cuda.synchronize()
    assert _same_bits(ph, r, NB_KEYS + ("seq",))
    # the filling pass alone on the decode's own layout
    ext, last = O.layout_of(cfg, plain)
    eng.encode(att)
    fr = eng.fill_naic(ext.to(torch.int32).cuda(), torch.from_numpy(last).to(torch.int32).cuda(), att.size(1), nbest=5, nbest_no_repeat=True)
    torch.cuda.synchronize()
    assert len(fr) == 3 and torch.equal(fr[0], r["seq"]) and torch.equal(_bits(fr[1]), _bits(r["seq_logprob"]))
    assert all(torch.equal(fr[2][k], r[k]) if k != "nbest_logp" else torch.equal(_bits(fr[2][k]), _bits(r[k])) for k in NB_KEYS)
    # raw logits: the totals are sums of logits
    raw = eng.decode_naic(att, raw_logits=True, nbest=4, nbest_no_repeat=True)
    torch.cuda.synchronize()
    _holds_the_rule(cfg, raw, 4)
    assert torch.equal(raw["seq"], r["seq"])


def test_off_is_the_decode_as_it_was(tiny_engine):
    """nbest_no_repeat False with nbest = 5 is the nbest = 5 result made before any call with the option, bit for bit; without nbest no key is added -- also into a
    reused dict of a call that had the option."""
    cfg, eng, att, plain, top, before = tiny_engine
    keys = ("seq", "seq_logprob", "row_plogp", "row_chosen") + LAYOUT
    used = eng.decode_naic(att, row_stats=True, nbest=3, nbest_no_repeat=True)      # (a call with the option in between, and its dict reused below)
    assert "nbest_seq" in used
    for off in (False, 0, None):
        r = eng.decode_naic(att, row_stats=True, nbest=5, nbest_no_repeat=off)
        torch.cuda.synchronize()
        assert _same_bits(r, before["nbest5"], keys + NB_KEYS)
    r = eng.decode_naic(att, row_stats=True, nbest=5, out=used)
    torch.cuda.synchronize()
    assert _same_bits(r, before["nbest5"], keys + NB_KEYS)
    r = eng.decode_naic(att, row_stats=True, out=r)
    torch.cuda.synchronize()
    assert _same_bits(r, plain, keys) and not any(k in r for k in NB_KEYS) and "constrained" not in r


def test_engine_refuses_what_the_option_excludes(tiny_engine):
    from boficap_amd import hip
    cfg, eng, att, plain, top, before = tiny_engine
    a = att[:4].contiguous()
    with pytest.raises(hip.BofiHipError, match="needs nbest"):
        eng.decode_naic(a, nbest_no_repeat=True)
    for bad in (7, 8):
        with pytest.raises(hip.BofiHipError, match=r"1\.\.6"):
            eng.decode_naic(a, nbest=bad, nbest_no_repeat=True)
    with pytest.raises(hip.BofiHipError, match=r"1\.\.8"):
        eng.decode_naic(a, nbest=9, nbest_no_repeat=True)
    with pytest.raises(hip.BofiHipError, match="repeat_min_id"):
        eng.decode_naic(a, nbest=3, nbest_no_repeat=True, repeat_min_id=-1)
    for kw, word in ((dict(ids_only=True), "ids_only"), (dict(refine_rounds=2, refine_method="mask_predict"), "mask_predict"), (dict(no_repeat=True), "no_repeat"),
                     (dict(block_trigrams=True), "block_trigrams"), (dict(require_ids=[9]), "require_ids")):
        with pytest.raises(hip.BofiHipError, match=word) as e:
            eng.decode_naic(a, nbest=3, nbest_no_repeat=True, **kw)
        assert "nbest" in str(e.value)
    z = torch.zeros(4, cfg.bound_len, dtype=torch.int32, device="cuda")
    one = torch.ones(4, dtype=torch.int32, device="cuda")
    with pytest.raises(hip.BofiHipError, match="needs nbest"):
        eng.fill_naic(z, one, 36, nbest_no_repeat=True)
    with pytest.raises(hip.BofiHipError, match=r"1\.\.6"):
        eng.fill_naic(z, one, 36, nbest=7, nbest_no_repeat=True)
    with pytest.raises(hip.BofiHipError, match="no_repeat"):
        eng.fill_naic(z, one, 36, nbest=3, nbest_no_repeat=True, no_repeat=True)
    with pytest.raises(hip.BofiHipError, match="float32"):
        hip.vocab_nbest_norepeat(torch.zeros(20, 61, dtype=torch.float64, device="cuda"), 61, 20, 3)
    with pytest.raises(hip.BofiHipError, match=r"1\.\.6"):
        hip.vocab_nbest_norepeat(torch.zeros(20, 61, device="cuda"), 61, 20, 7)
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
    out = model(fc, att, masks, opt={"train_mode": "NAIC", "nbest": 4, "nbest_no_repeat": 1}, mode="sample")
    assert len(out) == 6 and sorted(model.last_nbest) == ["count", "logp", "seq"]
    last = {k: v.clone() for k, v in model.last_nbest.items()}
    e = model.engine().decode_naic(att, masks.sum(1).to(torch.int32), nbest=4, nbest_no_repeat=True)
    torch.cuda.synchronize()
    assert torch.equal(out[0], e["seq"]) and torch.equal(out[0], plain[0]) and torch.equal(_bits(out[1]), _bits(plain[1]))
    assert torch.equal(last["seq"], e["nbest_seq"]) and torch.equal(last["count"], e["nbest_count"]) and torch.equal(_bits(last["logp"]), _bits(e["nbest_logp"]))
    assert last["seq"].shape == (6, 4, TINY.seq_length)
    _holds_the_rule(TINY, e, 4)
    for bad, word in (({"nbest": 0}, "needs"), ({"nbest": 7}, r"1\.\.6"), ({"decoding_constraint": 1}, "decoding_constraint"), ({"block_trigrams": 1}, "block_trigrams"),
                      ({"sample_method": "sample"}, "sample_method")):
        with pytest.raises(H.BofiHipError, match=word) as err:
            model(fc, att, masks, opt=dict({"train_mode": "NAIC", "nbest": 3, "nbest_no_repeat": 1}, **bad), mode="sample")
        assert "nbest" in str(err.value)
    again = model(fc, att, masks, opt={"train_mode": "NAIC"}, mode="sample")
    assert model.last_nbest is None and torch.equal(again[0], plain[0]) and torch.equal(_bits(again[1]), _bits(plain[1]))


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
    kw = dict(base, sample_n=3, sample_n_method="nbest", nbest_no_repeat=1)
    _, predictions, stats = eval_utils.eval_split(model, labels.feats, labels, kw)
    preds_n = kw["preds_n"]
    assert len(preds_n) == 24 and [p["image_id"] for p in preds_n] == [j // 3 for j in range(24)]
    assert all(set(p) == {"image_id", "seq", "logp"} for p in preds_n)
    for p in preds_n:                                           # no entry repeats a word
        assert is_valid(p["seq"], (), MIN_ID), p
    # the list is the engine's on the same images; the greedy predictions are the plain decode's
    e = model.engine().decode_naic(torch.from_numpy(labels.feats[:4]).cuda(), nbest=3, nbest_no_repeat=True)
    torch.cuda.synchronize()
    assert [p["logp"] for p in preds_n[:12]] == e["nbest_logp"].reshape(-1).cpu().tolist()
    rows_e = e["nbest_seq"].reshape(12, -1).cpu().numpy()
    for j in range(12):
        row = rows_e[j].tolist()
        stop = next((i for i, v in enumerate(row) if v <= 0), len(row))
        assert preds_n[j]["seq"] == row[:stop]
    assert stats["nbest_short"] == kw["nbest_short"] == sum(1 for i in range(8) if preds_n[3 * i + 2]["logp"] == -np.inf)
    kw_p = dict(base, sample_n=3, sample_n_method="nbest")
    _, predictions_p, stats_p = eval_utils.eval_split(model, labels.feats, labels, kw_p)
    assert [p["seq"] for p in predictions] == [p["seq"] for p in predictions_p]
    # diversity and oracle scores are those of exactly these rows
    rows = np.zeros((24, TINY.seq_length), dtype=np.int64)
    for j, p in enumerate(preds_n):
        rows[j, :len(p["seq"])] = p["seq"]
    again = kw["lang_eval"].evaluate_n(rows, 3)
    assert all(again[k] == stats[k] for k in again if k != "per_image") and any(k.startswith("oracle_") for k in again)
    div = DiversityEval(path, torch.device("cuda")).evaluate(torch.from_numpy(rows).cuda(), 3)
    assert all(div[k] == stats[k] for k in DIV_KEYS)
    assert list(stats) == list(stats_p)
    # the refusals
    for bad, word in ((dict(sample_n_method="sample"), "nbest_no_repeat"), (dict(sample_n=7), "at most 6"), (dict(decoding_constraint=1), "decoding_constraint")):
        with pytest.raises(ValueError, match=word):
            eval_utils.eval_split(model, labels.feats, labels, dict(kw, **bad))
    kw_q = dict(base, sample_n=3)
    kw_q["nbest_no_repeat"] = 1
    with pytest.raises(ValueError, match="nbest_no_repeat"):
        eval_utils.eval_split(model, labels.feats, labels, kw_q)
