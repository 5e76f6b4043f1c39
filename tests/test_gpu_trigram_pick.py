"""block_trigrams on the MI355X: bofi_vocab_pick against the numpy restatement (exact, the re-read of a row whose K candidates are all excluded included), the float32
engine against the restated decode (tests/test_trigram_pick.py), the bf16 engine held without a tolerance to ``pick3_np`` on its OWN returned log-probs (graph replay, fork,
phased form, grouped batches, feed-back, batch 1, ragged), "off is the decode as it was", the refusals, and the interface above the engine."""
import numpy as np
import pytest
import torch

import boficap_oracle as O
from conftest import record_parity
from test_constrained_pick import NAN, pick_np, plain_of
from test_gpu_constrained_pick import BIG_V, KEEP, LAYOUT, _at_offset, _big_ban_case, _bits, _clone, _rows, _same_bits, _short_case
from test_trigram_pick import FIGURES, adjacent_repeats, pick3_np, repeated_trigrams, restate3

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------- 1. the kernel
def _case_rows(rng, B, S, V, ldx, kind):
    """x [B, S, ldx]: 'identical' -- every row the same strictly descending preference over the word ids 7, 8, ... (the rule walks far down the order); 'small' -- plain
    random rows with ties (V too small for _rows' chains); else _rows' mixture, and on every other image six word ids that lead EVERY position in the same order (captions
    that loop until the rule breaks them, picks well past a row's two best)."""
    if kind == "identical":
        x = np.full((B, S, ldx), -50.0, np.float32)
        x[:, :, 7:V] = -0.125 * np.arange(V - 7, dtype=np.float32)
        return x
    if kind == "small":
        x = rng.integers(-3, 3, (B, S, ldx)).astype(np.float32)
        x[0, 1, 2] = NAN
        return x
    x = _rows(rng, B, S, V, ldx)
    for b in range(0, B, 2):
        hot = rng.choice(np.arange(7, V), 6, replace=False)
        x[b, :, hot] = (9.0 - 0.5 * np.arange(6, dtype=np.float32))[:, None]
    return x


KERNEL_CASES = [(5, 20, 9491, 9491, "mixed"), (3, 40, 67, 72, "mixed"), (4, 64, 33, 33, "mixed"), (2, 3, 8, 8, "small"), (3, 40, 48, 48, "identical")]


@pytest.mark.parametrize("B,S,V,ldx,kind", KERNEL_CASES)
def test_kernel_equals_pick3_np(B, S, V, ldx, kind):
    """seq, row_chosen and changed bit for bit: with and without a ban table, with and without no_repeat, ntok read with a bias and clamped, the tensor 0 and 3 floats off a
    16-byte boundary; block_trigrams = 0 equals bofi_vocab_constrain on the same tensors bit for bit.  The identical-rows case needs picks beyond the 8th best of a row --
    more than any K the kernel may keep --, so the row is read again there."""
    from boficap_amd import hip
    rng = np.random.default_rng(9000 + 100 * B + S + V)
    x = _case_rows(rng, B, S, V, ldx, kind)
    n = rng.integers(3, S + 1, B)
    n[0] = S
    if kind == "identical":
        n[:] = [S, S - 9, S - 14]
    ntok = (n + 1).astype(np.int32)                             # the engine's form: `last` with a bias of -1
    if kind == "mixed":
        ntok[1], n[1] = S + 9, S                                # clamped from above ...
        ntok[2], n[2] = -4, 0                                   # ... and from below
    words = np.arange(7, V)
    ban = sorted(set(rng.choice(words, max(1, (V - 7) // 8), replace=False).tolist()))      # word ids only: ids 0..6 are never excluded, so an eligible id always exists
    if kind == "identical":
        ban = [7, 9]
    old = rng.integers(0, V, (B, S)).astype(np.int64)
    old[::2] = pick_np(x[:, :, :V], n, pad=2)["seq"][::2]
    d_ntok, d_ban = torch.from_numpy(ntok).cuda(), hip.ban_bits(ban, V, "cuda")
    runs = [(use_ban, rep, tri) for use_ban in (False, True) for rep in (False, True) for tri in (True, False)]
    wants = {(use_ban, rep): pick3_np(x[:, :, :V], n, ban if use_ban else (), rep, True, 7, pad=2, old=old) for use_ban in (False, True) for rep in (False, True)}
    deepest = max(int(w["rank"].max()) for w in wants.values())
    moved = sum(int((wants[k]["seq"] != pick_np(x[:, :, :V], n, ban if k[0] else (), k[1], 7, pad=2)["seq"]).sum()) for k in wants)
    print(f"trigram pick kernel {(B, S, V, ldx, kind)}: deepest pick {deepest}, {moved} positions moved by the rule over the four variants")
    if kind == "identical":
        for k, w in wants.items():
            first = int(np.nonzero((w["rank"] >= 9).any(0))[0][0])
            print(f"  ban={k[0]} no_repeat={k[1]}: the 9th best first at s = {first}, deepest {int(w['rank'].max())}")
            assert int(w["rank"].max()) >= 9                    # beyond any K <= 8: the fallback runs
    elif kind == "mixed":
        assert deepest >= 3 and moved > 0                       # not served by two candidates
    else:
        assert moved == 0                                       # S = 3: nothing blockable
    work = torch.empty(hip.lib().bofi_vocab_pick_workspace(B * S) // 4, dtype=torch.int32, device="cuda")
    for off in (0, 3):
        buf = torch.full((B * S * ldx + 8,), 7.0, dtype=torch.float32, device="cuda")
        dx = buf[off:off + B * S * ldx].view(B * S, ldx)
        dx.copy_(torch.from_numpy(x.reshape(B * S, ldx)))
        for use_ban, rep, tri in runs:
            what = (B, S, V, ldx, off, use_ban, rep, tri)
            seq = torch.from_numpy(old.copy()).cuda().view(-1)
            chosen = torch.full((B * S,), KEEP, dtype=torch.float32, device="cuda")
            changed = torch.full((B,), -1, dtype=torch.int32, device="cuda")
            kw = dict(ntok=d_ntok, ntok_bias=-1, pad_idx=2, ban=d_ban if use_ban else None, no_repeat=rep, repeat_min_id=7, row_chosen=chosen, changed=changed)
            work.fill_(-7)
            hip.vocab_pick(dx, V, S, seq, block_trigrams=tri, work=work, **kw)
            torch.cuda.synchronize()
            if tri:
                want = wants[(use_ban, rep)]
                live = np.arange(S)[None, :] < n[:, None]
                assert np.array_equal(seq.cpu().numpy().reshape(B, S), want["seq"]), what
                expect = np.where(live, want["chosen"], np.float32(KEEP)).astype(np.float32)
                assert np.array_equal(chosen.cpu().numpy().reshape(B, S).view(np.int32), expect.view(np.int32)), what
                assert np.array_equal(changed.cpu().numpy(), want["changed"]), what
            else:                                               # the rule off: bofi_vocab_constrain's outputs
                seq2 = torch.from_numpy(old.copy()).cuda().view(-1)
                chosen2, changed2 = torch.full_like(chosen, KEEP), torch.full_like(changed, -1)
                hip.vocab_constrain(dx, V, S, seq2, **dict(kw, row_chosen=chosen2, changed=changed2))
                torch.cuda.synchronize()
                assert torch.equal(seq, seq2) and torch.equal(_bits(chosen), _bits(chosen2)) and torch.equal(changed, changed2), what
        assert np.array_equal(dx.cpu().numpy().view(np.int32), x.reshape(B * S, ldx).view(np.int32))      # (x is read only)
    # optional outputs and ntok left out
    seq = torch.from_numpy(old.copy()).cuda().view(-1)
    hip.vocab_pick(dx, V, S, seq, pad_idx=2, block_trigrams=True)
    torch.cuda.synchronize()
    assert np.array_equal(seq.cpu().numpy().reshape(B, S), pick3_np(x[:, :, :V], np.full(B, S), pad=2)["seq"])
    with pytest.raises(hip.BofiHipError, match="workspace"):
        hip.vocab_pick(dx, V, S, seq, work=torch.empty(work.numel() - 1, dtype=torch.int32, device="cuda"))


def _pick_equals(want, live, seq, chosen, changed, what):
    shape = want["seq"].shape
    assert np.array_equal(seq.cpu().numpy().reshape(shape), want["seq"]), what
    expect = np.where(live, want["chosen"], np.float32(KEEP)).astype(np.float32)
    assert np.array_equal(chosen.cpu().numpy().reshape(shape).view(np.int32), expect.view(np.int32)), what
    assert np.array_equal(changed.cpu().numpy(), want["changed"]), what


@pytest.mark.parametrize("V", [2, 3, 5, 6])
def test_kernel_on_rows_shorter_than_a_wavefronts_loads(V):
    """bofi_vocab_pick on test_gpu_constrained_pick's short-row case (ldx = V below 8 floats, every alignment of tensor and rows): seq, row_chosen and changed bit for bit
    against pick3_np, with the table and without.  (With block_trigrams the word floor stays 7, above every id: at V <= 6 a floor of 0 could leave a position no id.)"""
    from boficap_amd import hip
    B, S = 2, 8
    x, n, ntok, ban, old = _short_case(V, B, S)
    d_ntok, d_ban = torch.from_numpy(ntok).cuda(), hip.ban_bits(ban, V, "cuda")
    runs = [(use_ban, tri, min_id) for use_ban in (True, False) for tri, min_id in ((False, 0), (True, 7))]
    wants = {r: pick3_np(x, n, ban if r[0] else (), True, r[1], r[2], pad=2, old=old) for r in runs}
    live = np.arange(S)[None, :] < n[:, None]
    work = torch.empty(hip.lib().bofi_vocab_pick_workspace(B * S) // 4, dtype=torch.int32, device="cuda")
    for off in (0, 1, 2, 3):
        dx = _at_offset(x.reshape(B * S, V), off)
        for use_ban, tri, min_id in runs:
            seq = torch.from_numpy(old.copy()).cuda().view(-1)
            chosen = torch.full((B * S,), KEEP, dtype=torch.float32, device="cuda")
            changed = torch.full((B,), -1, dtype=torch.int32, device="cuda")
            work.fill_(-7)
            hip.vocab_pick(dx, V, S, seq, ntok=d_ntok, ntok_bias=-1, pad_idx=2, ban=d_ban if use_ban else None, no_repeat=True, block_trigrams=tri, repeat_min_id=min_id,
                           row_chosen=chosen, changed=changed, work=work)
            torch.cuda.synchronize()
            _pick_equals(wants[(use_ban, tri, min_id)], live, seq, chosen, changed, (V, off, use_ban, tri, min_id))


def test_kernel_reads_a_long_ban_table_through_the_cache():
    """bofi_vocab_pick with a ban table of 8 194 words, more than the 8 192 the candidates launch stages in LDS: bit for bit against pick3_np."""
    from boficap_amd import hip
    x, ban, old = _big_ban_case()
    want = pick3_np(x, [2], ban, True, True, 7, pad=2, old=old)
    assert not set(want["seq"].ravel().tolist()) & set(ban)
    dx = torch.from_numpy(x.reshape(2, BIG_V)).cuda()
    seq = torch.from_numpy(old.copy()).cuda().view(-1)
    chosen = torch.full((2,), KEEP, dtype=torch.float32, device="cuda")
    changed = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    hip.vocab_pick(dx, BIG_V, 2, seq, pad_idx=2, ban=hip.ban_bits(ban, BIG_V, "cuda"), no_repeat=True, block_trigrams=True, repeat_min_id=7, row_chosen=chosen, changed=changed)
    torch.cuda.synchronize()
    _pick_equals(want, np.ones((1, 2), bool), seq, chosen, changed, "long ban table")


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
    """Strict Q1, block_trigrams with no_repeat off and on, T feed-back rounds with the constrained ids fed back.  On every SAFE image (every decision of its scan, all
    passes, has a margin above 1e-3 in the restatement's own run; the counts are those test_trigram_pick asserts) seq and the counts are equal and row_chosen is within the
    float32 log-prob bar of the constrained-pick test."""
    BAR = 1e-3
    base = plain_of(name)
    eng = f32_engines(name)
    att = base["att"].cuda()
    att_len = None if base["masks"] is None else base["masks"].sum(1).to(torch.int32).cuda()
    worst = 0.0
    for rep in (False, True):
        ref = restate3(name, rep)[T]
        r = eng.decode_naic(att, att_len, refine_rounds=T, row_stats=True, no_repeat=rep, block_trigrams=True)
        torch.cuda.synchronize()
        for k in LAYOUT:
            assert torch.equal(r[k].cpu(), base[k]), (rep, k)
        safe = ref["safe"]
        assert (int(safe.sum()), len(safe)) == FIGURES[(name, rep, T)][2:]
        assert np.array_equal(r["seq"].cpu().numpy()[safe], ref["seq"][safe]), rep
        assert np.array_equal(r["constrained"].cpu().numpy()[safe], ref["changed"][safe]), rep
        live = (np.arange(base["cfg"].seq_length)[None, :] < base["n"][:, None]) & safe[:, None]
        err = float(np.abs(np.nan_to_num(r["row_chosen"].cpu().numpy() - ref["chosen"]))[live].max())
        lp_err = float((r["seq_logprob"].cpu() - torch.from_numpy(ref["lp"])).nan_to_num().abs()[torch.from_numpy(safe)].max())
        print(f"trigram pick {name} no_repeat={rep} T={T}: |row_chosen - restatement| max {err:.3e}, |seq_logprob - restatement| max {lp_err:.3e}; safe images {int(safe.sum())} of "
              f"{len(safe)}; {int(ref['changed'].sum())} positions changed, deepest pick {int(ref['rank'].max())}")
        worst = max(worst, err)
        assert err < BAR and lp_err < BAR, rep
        assert int(ref["rank"][safe].max()) >= 3                # (the compared images need more than two candidates)
    record_parity(f"trigram_pick_f32_row_chosen_{name}_T{T}", worst, BAR, "float32 engine, row_chosen of a decode with block_trigrams, against the restatement on the oracle")


# ----------------------------------------------------------------------------- 3. the bf16 engine, without a tolerance
@pytest.fixture(scope="module")
def bf16_full(weight_cache, manifest):
    """The full-size bf16 engine on full_b8's weights and 16 synthetic images, with the decodes made BEFORE any call with block_trigrams on this engine."""
    from boficap_amd import weights as W
    from boficap_amd.engine import BofiEngine
    m = manifest["full_b8"]
    cfg, sd = weight_cache(m["config"], m["seed"], m["gen_scale"], m["digest"], m.get("patch"))
    eng = BofiEngine(cfg, torch.bfloat16, max_batch=64, max_regions=36)
    eng.load_state_dict(sd)
    att = torch.from_numpy(W.synthetic_att_feats(16, 36, cfg.att_feat_size, seed=77)).cuda().to(torch.bfloat16)
    plain = _clone(eng.decode_naic(att, row_stats=True))
    torch.cuda.synchronize()
    live = plain["seq"][plain["seq"] >= 7]
    ids, counts = torch.unique(live, return_counts=True)
    top = int(ids[counts.argmax()])
    before = {"no_repeat": _clone(eng.decode_naic(att, row_stats=True, no_repeat=True)), "ban": _clone(eng.decode_naic(att, row_stats=True, ban_ids=[top]))}
    torch.cuda.synchronize()
    return cfg, eng, att, plain, top, before


def _holds_the_rule(cfg, r, ban, rep, min_id=7):
    """No repeated word trigram, no adjacent repeat under no_repeat, no banned id; and seq, row_chosen and constrained of ``r`` equal pick3_np on r's own seq_logprob, bit for
    bit: every pick is the best eligible id of the log-probs the call returned."""
    S = cfg.seq_length
    lp = r["seq_logprob"].cpu().numpy()
    n = r["phrase_length"].sum(1).cpu().numpy()
    seq = r["seq"].cpu().numpy()
    assert repeated_trigrams(seq, n, min_id) == 0
    assert not rep or adjacent_repeats(seq, n, min_id) == 0
    assert not np.isin(seq, np.asarray(list(ban), np.int64)).any() or cfg.pad_idx in ban
    want = pick3_np(lp, n, ban, rep, True, min_id, pad=cfg.pad_idx, old=pick_np(lp, n, pad=cfg.pad_idx)["seq"])
    assert np.array_equal(seq, want["seq"])
    live = np.arange(S)[None, :] < n[:, None]
    assert np.array_equal(r["row_chosen"].cpu().numpy().view(np.int32)[live], want["chosen"].view(np.int32)[live])
    assert np.array_equal(r["constrained"].cpu().numpy(), want["changed"])
    return want


def test_bf16_engine_holds_the_rule_graph_fork_phases_groups(bf16_full):
    cfg, eng, att, plain, top, _ = bf16_full
    kw = dict(row_stats=True, no_repeat=True, block_trigrams=True)
    keys = ("seq", "row_plogp", "row_chosen", "seq_logprob", "constrained") + LAYOUT
    r = _clone(eng.decode_naic(att, **kw))
    torch.cuda.synchronize()
    want = _holds_the_rule(cfg, r, (), True)
    assert torch.equal(_bits(r["seq_logprob"]), _bits(plain["seq_logprob"]))          # T = 0: the distribution is the plain decode's, bit for bit
    assert torch.equal(_bits(r["row_plogp"]), _bits(plain["row_plogp"])) and _same_bits(r, plain, LAYOUT)
    n = r["phrase_length"].sum(1).cpu().numpy()
    two = pick_np(r["seq_logprob"].cpu().numpy(), n, (), True, 7, pad=cfg.pad_idx)["seq"]
    assert repeated_trigrams(two, n) > 0 and int(want["rank"].max()) >= 3            # (the rule bites here, past a row's two best)
    # trigrams alone, with a ban, another floor, and one feed-back round (every pass constrained; the last one checked on its own tensor)
    for ban, rep, min_id, T in ((None, False, 7, 0), ([top], True, 7, 0), ([top], False, 0, 0), (None, True, 7, 1)):
        q = eng.decode_naic(att, row_stats=True, ban_ids=ban, no_repeat=rep, repeat_min_id=min_id, refine_rounds=T, block_trigrams=True)
        torch.cuda.synchronize()
        _holds_the_rule(cfg, q, ban or (), rep, min_id)
        if T:
            assert not torch.equal(_bits(q["seq_logprob"]), _bits(eng.decode_naic(att, refine_rounds=T, no_repeat=rep)["seq_logprob"]))      # (the ids of THIS rule were fed back)
    # graph: captured, then replayed
    g = eng.decode_naic(att, graph=True, **kw)
    g = eng.decode_naic(att, graph=True, out=g, **kw)
    torch.cuda.synchronize()
    assert _same_bits(g, r, keys)
    # a fork on its own stream (its own workspace)
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
    # two batches of 8 in one call, batch 1, and a ragged batch: the rule on the call's own tensor
    q1 = eng.decode_naic(att, q1_group=8, **kw)
    torch.cuda.synchronize()
    _holds_the_rule(cfg, q1, (), True)
    one = eng.decode_naic(att[:1].contiguous(), **kw)
    torch.cuda.synchronize()
    _holds_the_rule(cfg, one, (), True)
    lens = torch.tensor([36, 9, 30, 20, 36], dtype=torch.int32, device="cuda")
    rag = eng.decode_naic(att[:5].contiguous(), lens, **kw)
    torch.cuda.synchronize()
    _holds_the_rule(cfg, rag, (), True)
    # the filling pass alone on the decode's own layout
    ext, last = O.layout_of(cfg, r)
    eng.encode(att)
    fr = eng.fill_naic(ext.to(torch.int32).cuda(), torch.from_numpy(last).to(torch.int32).cuda(), att.size(1), no_repeat=True, block_trigrams=True)
    torch.cuda.synchronize()
    assert len(fr) == 3 and torch.equal(fr[0], r["seq"]) and torch.equal(fr[2]["constrained"], r["constrained"]) and torch.equal(_bits(fr[1]), _bits(r["seq_logprob"]))
    # raw logits: the pick is over logits
    raw = eng.decode_naic(att, raw_logits=True, block_trigrams=True)
    torch.cuda.synchronize()
    lg, nn = raw["seq_logprob"].cpu().numpy(), raw["phrase_length"].sum(1).cpu().numpy()
    assert np.array_equal(raw["seq"].cpu().numpy(), pick3_np(lg, nn, (), False, True, 7, pad=cfg.pad_idx)["seq"])


def test_off_is_the_decode_as_it_was(bf16_full):
    """With block_trigrams off the plain decode, the no_repeat decode and the ban decode are those made before any trigram call on this engine, bit for bit; so is a call
    with a zero flag and a zero record."""
    from boficap_amd import hip
    cfg, eng, att, plain, top, before = bf16_full
    keys = ("seq", "seq_logprob", "row_plogp", "row_chosen") + LAYOUT
    eng.decode_naic(att, no_repeat=True, block_trigrams=True)   # (a trigram call in between)
    for kw, want in (({}, plain), ({"block_trigrams": False}, plain), ({"no_repeat": True}, before["no_repeat"]), ({"ban_ids": [top], "block_trigrams": False}, before["ban"])):
        r = eng.decode_naic(att, row_stats=True, **kw)
        torch.cuda.synchronize()
        assert _same_bits(r, want, keys) and ("constrained" in r) == ("constrained" in want), kw
        if "constrained" in want:
            assert torch.equal(r["constrained"], want["constrained"])
    eng.decode_naic(att, block_trigrams=True)
    o = eng.decode_naic(att)
    rec = hip.BofiCallOpts()                                    # zero-filled
    rc = hip.lib().bofi_engine_decode_naic(eng._h, hip.ptr(att), hip.dtype_code(att), None, att.size(0), 36, hip.FLAG_STRICT_Q1, hip.ptr(o["seq"]), hip.ptr(o["seq_logprob"]),
                                           hip.ptr(o["phrase_num"]), hip.ptr(o["phrase_length"]), hip.ptr(o["phrase_syn"]), None, hip.ptr(o["bound_iters"]), rec, hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and _same_bits(o, plain, ("seq", "seq_logprob") + LAYOUT)


def test_engine_refuses_what_block_trigrams_excludes(bf16_full):
    from boficap_amd import hip
    from boficap_amd.engine import DecodePipeline
    cfg, eng, att, plain, top, _ = bf16_full
    a = att[:4].contiguous()
    with pytest.raises(hip.BofiHipError, match="ids_only"):
        eng.decode_naic(a, ids_only=True, block_trigrams=True)
    with pytest.raises(hip.BofiHipError, match="mask_predict"):
        eng.decode_naic(a, refine_rounds=2, refine_method="mask_predict", block_trigrams=True)
    with pytest.raises(hip.BofiHipError, match="seq_length"):
        eng.decode_naic(a, ban_ids=range(cfg.seq_length, cfg.tgt_vocab), block_trigrams=True)       # (seq_length ids stay: one too few)
    with pytest.raises(hip.BofiHipError, match="repeat_min_id"):
        eng.decode_naic(a, block_trigrams=True, repeat_min_id=-1)
    with pytest.raises(hip.BofiHipError, match="fused_vocab"):
        DecodePipeline(eng, fused_vocab=True, block_trigrams=True)
    with pytest.raises(hip.BofiHipError, match="mask_predict"):
        DecodePipeline(eng, refine_rounds=2, refine_method="mask_predict", block_trigrams=True)
    # the library's own checks, before anything is enqueued
    o = eng.decode_naic(a)
    lib = hip.lib()
    TRI = hip.FLAG_PICK_TRIGRAMS

    def args(flags, rec, lp=True):
        return (eng._h, hip.ptr(a), hip.dtype_code(a), None, 4, 36, flags, hip.ptr(o["seq"]), hip.ptr(o["seq_logprob"]) if lp else None, hip.ptr(o["phrase_num"]),
                hip.ptr(o["phrase_length"]), hip.ptr(o["phrase_syn"]), None, hip.ptr(o["bound_iters"]), rec, hip.stream_ptr())
    rec = lambda **kw: hip.BofiCallOpts(**dict(dict(pick_repeat_min_id=7), **kw))
    assert lib.bofi_engine_decode_naic(*args(TRI | hip.FLAG_IDS_ONLY, rec(), lp=False)) == 1 and b"IDS_ONLY" in lib.bofi_last_error()
    assert lib.bofi_engine_decode_naic(*args(TRI | hip.FLAG_MASK_PREDICT | (2 << 8), rec())) == 1 and b"MASK_PREDICT" in lib.bofi_last_error()
    assert lib.bofi_engine_decode_naic(*args(TRI, rec(pick_no_repeat=2))) == 1 and b"pick_no_repeat" in lib.bofi_last_error()
    assert lib.bofi_engine_decode_naic(*args(TRI, rec(pick_repeat_min_id=-1))) == 1 and b"pick_repeat_min_id" in lib.bofi_last_error()
    sa = args(TRI, rec())
    assert lib.bofi_engine_decode_saic(*(sa[:12] + sa[13:])) == 3 and b"semi-autoregressive" in lib.bofi_last_error()
    f = eng.fork(ids_only=True)                                  # a fork without vocabulary buffers (and without the workspace) never reaches the pick
    assert lib.bofi_engine_decode_naic(*((f._h,) + args(TRI, rec())[1:])) == 3
    assert lib.bofi_engine_decode_naic(*((f._h,) + args(TRI | hip.FLAG_IDS_ONLY, rec(), lp=False)[1:])) == 1
    torch.cuda.synchronize()
    again = eng.decode_naic(a)                                   # nothing was enqueued: the engine decodes as before
    torch.cuda.synchronize()
    assert _same_bits(again, o, ("seq", "seq_logprob"))
    assert torch.equal(eng.decode_naic(att)["seq"], plain["seq"])


# ----------------------------------------------------------------------------- 4. above the engine
def test_interface_gives_the_engine_level_result(weight_cache, monkeypatch):
    """decode_many (a ragged tail batch) and mode='sample' with opt['block_trigrams'] against BofiEngine.decode_naic on the same batches, same kernel family and hint."""
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
        feats = torch.from_numpy(W.synthetic_att_feats(16 + 5, 36, cfg.att_feat_size, seed=79)).to(torch.bfloat16)
        batches = [feats[:16], feats[16:]]                      # a batch of 16 and a tail of 5 ...
        tail_masks = torch.ones(5, 36)
        tail_masks[1, 9:] = 0; tail_masks[4, 30:] = 0           # ... which is ragged
        ref = BofiEngine(cfg, torch.bfloat16, max_batch=16, max_regions=36)
        ref.load_state_dict(sd)
        ref.set_decodes_in_flight(2)
        lens = lambda i: tail_masks.sum(1).to(torch.int32).cuda() if i == 1 else None
        plain = [ref.decode_naic(b.cuda(), lens(i))["seq"].cpu() for i, b in enumerate(batches)]
        want = []
        for i, b in enumerate(batches):
            r = ref.decode_naic(b.cuda(), lens(i), row_stats=True, no_repeat=True, block_trigrams=True)
            want.append({k: v.cpu() for k, v in r.items() if torch.is_tensor(v)})
        items = [batches[0].pin_memory(), (batches[1].pin_memory(), tail_masks)]
        got = list(model.decode_many(items, batches_per_launch=2, in_flight=2, no_repeat=True, block_trigrams=True))
        assert len(got) == 2
        for i, (g, w) in enumerate(zip(got, want)):
            for k in ("seq", "constrained") + LAYOUT:
                assert torch.equal(g[k], w[k]), (i, k)
            n = g["phrase_length"].sum(1).numpy()
            assert repeated_trigrams(g["seq"].numpy(), n) == 0 and adjacent_repeats(g["seq"].numpy(), n) == 0
        only_rep = list(model.decode_many(items, batches_per_launch=2, in_flight=2, no_repeat=True))
        assert any(not torch.equal(g["seq"], q["seq"]) for g, q in zip(got, only_rep))          # (the keyword does something beyond no_repeat)
        again = list(model.decode_many(items, batches_per_launch=2, in_flight=2))               # the defaults stay the plain decode
        assert all(torch.equal(g["seq"], p) and "constrained" not in g for g, p in zip(again, plain))
        with pytest.raises(H.BofiHipError, match="fused_vocab"):
            list(model.decode_many(items, fused_vocab=True, block_trigrams=True))
        # mode='sample' with the reference's name
        fc = torch.zeros(5, 0, device="cuda")
        out = model(fc, batches[1].cuda(), tail_masks.cuda(), opt={"train_mode": "NAIC", "block_trigrams": 1}, mode="sample")
        assert len(out) == 6
        counts_ = model.last_constrained.clone()
        e = model.engine().decode_naic(batches[1].cuda(), lens(1), block_trigrams=True)
        torch.cuda.synchronize()
        assert torch.equal(out[0], e["seq"]) and torch.equal(counts_, e["constrained"]) and torch.equal(out[3], e["phrase_length"])
        assert torch.equal(_bits(out[1].nan_to_num()), _bits(e["seq_logprob"].nan_to_num()))
        nn = e["phrase_length"].sum(1).cpu().numpy()
        assert int(counts_.sum()) > 0 and repeated_trigrams(out[0].cpu().numpy(), nn) == 0
        p6 = model(fc, batches[1].cuda(), tail_masks.cuda(), opt={"train_mode": "NAIC", "block_trigrams": 0}, mode="sample")
        assert model.last_constrained is None and repeated_trigrams(p6[0].cpu().numpy(), nn) > 0      # (the reference's default, 0, is the plain decode)
        for bad in ({"train_mode": "NAIC", "block_trigrams": 1, "sample_method": "sample"},
                    {"train_mode": "NAIC", "block_trigrams": 1, "refine_rounds": 2, "refine_method": "mask_predict"}, {"train_mode": "SAIC", "block_trigrams": 1}):
            with pytest.raises(H.BofiHipError, match="block_trigrams"):
                model(fc, batches[1].cuda(), tail_masks.cuda(), opt=bad, mode="sample")
    finally:
        monkeypatch.undo()
        H.lib().bofi_reload_env()


def test_eval_split_blocks_trigrams():
    from boficap_amd import eval_utils
    from boficap_amd.config import TINY
    from test_gpu_lang_eval import tiny_model
    labels = eval_utils.SyntheticLabels(TINY, 8, 5, seed=3)
    model = tiny_model()
    base = {"batch_size": 4, "language_eval": 1, "verbose_loss": 0}
    _, preds0, stats0 = eval_utils.eval_split(model, labels.feats, labels, dict(base))
    _, preds, stats = eval_utils.eval_split(model, labels.feats, labels, dict(base, block_trigrams=1))
    assert "constrained_rate" not in stats0 and list(stats)[:-1] == list(stats0) and list(stats)[-1] == "constrained_rate"
    host = torch.from_numpy(labels.feats)
    got = list(model.decode_many([host[i:i + 4] for i in range(0, 8, 4)], block_trigrams=True))
    changed, emitted = sum(int(g["constrained"].sum()) for g in got), sum(int(g["phrase_length"].sum()) for g in got)
    assert 0 < changed <= emitted and stats["constrained_rate"] == changed / emitted
    assert [p["seq"] for p in preds] == [[int(v) for v in row.tolist()[:next((q for q, v in enumerate(row.tolist()) if v <= 0), len(row))]] for g in got for row in g["seq"]]
    assert preds != preds0
    for g in got:
        assert repeated_trigrams(g["seq"].numpy(), g["phrase_length"].sum(1).numpy()) == 0
    with pytest.raises(ValueError, match="NAIC"):
        eval_utils.eval_split(model, labels.feats, labels, dict(base, inference_mode="SAIC", block_trigrams=1))
