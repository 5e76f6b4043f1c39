"""Required words on the MI355X: bofi_vocab_require against the numpy restatement (bit for bit), the float32 engine against the restated decode on the golden cases
(tests/test_required_words.py), the bf16 engine held without a tolerance to ``require_np`` on its OWN returned log-probs and the ids of the same decode without the
option (graph replay, fork, phased form, filling pass alone, grouped batches, feed-back, no log-prob tensor), "off is today's decode", the refusals, and the interface
above the engine (decode_many, mode='sample', eval_split)."""
import functools

import numpy as np
import pytest
import torch

import boficap_oracle as O
from test_constrained_pick import MARGIN, NAN, order_np, pick_np, plain_of
from test_gpu_constrained_pick import KEEP, LAYOUT, _bits, _clone, _same_bits
from test_required_words import classify_np, require_np

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------- 1. the kernel
def _kernel_case(rng, B, S, V, ldx, K):
    """x [B, S, ldx] from a small tie-rich set with NaN and +-inf sprinkled in and poison past column V; seq and the word rows drawn from the same few ids around
    repeat_min_id (words stand in seq already, next to each other too) with empties, ids >= V, duplicates; a few ids outside the vocabulary in seq."""
    vals = np.array([-0.125, -0.25, -0.25, -0.5, -0.5, -1.0, -2.0, -0.0, 0.0], np.float32)
    x = vals[rng.integers(0, len(vals), (B, S, ldx))]
    bad = rng.random((B, S, ldx)) < 0.04
    x[bad] = np.array([NAN, np.inf, -np.inf], np.float32)[rng.integers(0, 3, int(bad.sum()))]
    x[:, :, V:] = np.inf                                        # a padded pitch: never read
    if ldx > V + 1:
        x[:, :, V + 1] = NAN
    pool = np.arange(4, min(V, 4 + max(6, S // 2)))
    seq = rng.choice(pool, (B, S)).astype(np.int64)
    seq[rng.random((B, S)) < 0.03] = V + 5                      # ids outside the vocabulary: such a position is eligible for nothing
    seq[rng.random((B, S)) < 0.02] = -3
    words = rng.choice(pool, (B, K)).astype(np.int32)           # (duplicates follow from the small pool)
    words[rng.random((B, K)) < 0.15] = -1
    words[rng.random((B, K)) < 0.08] = V
    words[rng.random((B, K)) < 0.04] = 2 ** 31 - 1
    n = rng.integers(0, S + 1, B)
    n[0] = S
    ntok = (n + 1).astype(np.int32)                             # the engine's form: `last` with a bias of -1
    if B >= 5:
        n[1], n[2] = 0, 1
        ntok[1], ntok[2] = 1, 2
        ntok[3], n[3] = S + 9, S                                # clamped from above ...
        ntok[4], n[4] = -4, 0                                   # ... and from below
    words[0, 0] = pool[1]                                       # (image 0 always requires a word)
    for b in range(0, B, 3):                                    # every third image: its first word stands at the middle live position and is costly everywhere else
        if 0 <= words[b, 0] < V and n[b] > 0:
            seq[b, n[b] // 2] = words[b, 0]
            x[b, :, words[b, 0]] = -8.0
            x[b, n[b] // 2, words[b, 0]] = 0.0                  # (... and no other word gains by taking that position)
    ban = sorted({int(words[0, 0])} | {int(v) for v in rng.choice(pool, 2, replace=False)})
    return x, seq, words, n, ntok, ban


KERNEL_CASES = [(1, 20, 64, 64, 1), (5, 20, 9491, 9491, 4), (3, 64, 9491, 9600, 8), (130, 20, 257, 257, 3)]


@pytest.mark.parametrize("B,S,V,ldx,K", KERNEL_CASES)
def test_kernel_equals_require_np(B, S, V, ldx, K):
    """seq, row_chosen (the untouched entries included), pos and moved bit for bit: with and without a ban table, no_repeat, ntok, row_chosen and moved; ntok read with a
    bias and clamped; for the small-B shapes the tensor 0..3 floats off a 16-byte boundary; x is read only."""
    from boficap_amd import hip
    rng = np.random.default_rng(7000 + 100 * B + S + V + K)
    x, old, words, n, ntok, ban = _kernel_case(rng, B, S, V, ldx, K)
    d_ntok, d_ban, d_words = torch.from_numpy(ntok).cuda(), hip.ban_bits(ban, V, "cuda"), torch.from_numpy(words).cuda()
    keep = np.full((B, S), KEEP, np.float32)
    wants = {(use_ban, rep): require_np(x[:, :, :V], n, words, old, ban if use_ban else (), rep, 7, chosen=keep) for use_ban in (False, True) for rep in (False, True)}
    w = wants[(False, False)]
    kinds = np.concatenate([classify_np(words[b], V, ()) for b in range(B)])
    print(f"required words kernel {(B, S, V, ldx, K)}: {int((w['pos'] >= 0).sum())} placed, {int((w['pos'] == -3).sum())} unplaceable, {int((kinds == -2).sum())} skipped, "
          f"{int((kinds == -1).sum())} empty, {int(w['moved'].sum())} moved, {int((w['margin'] == 0).sum())} of {B} images with an exact tie; "
          f"{int((wants[(False, True)]['seq'] != w['seq']).sum())} positions differ under no_repeat, {int((wants[(True, False)]['seq'] != w['seq']).sum())} under the ban")
    assert int((w["pos"] >= 0).sum()) > int(w["moved"].sum())                         # words already standing in seq were "placed" where they stood
    assert (wants[(True, False)]["pos"] == -2).sum() > (w["pos"] == -2).sum()         # the ban table skips words
    if B >= 3:
        assert (w["moved"] > 0).any()
    if B >= 5:
        assert (w["pos"] == -3).any() and (kinds == -2).any() and (kinds == -1).any()
    for off in ((0, 1, 2, 3) if B <= 5 else (0,)):
        buf = torch.full((B * S * ldx + 8,), 7.0, dtype=torch.float32, device="cuda")
        dx = buf[off:off + B * S * ldx].view(B * S, ldx)
        dx.copy_(torch.from_numpy(x.reshape(B * S, ldx)))
        for (use_ban, rep), want in wants.items():
            what = (B, S, V, ldx, K, off, use_ban, rep)
            seq = torch.from_numpy(old.copy()).cuda().view(-1)
            chosen = torch.full((B * S,), KEEP, dtype=torch.float32, device="cuda")
            pos = torch.full((B, K), -9, dtype=torch.int32, device="cuda")
            moved = torch.full((B,), -9, dtype=torch.int32, device="cuda")
            hip.vocab_require(dx, V, S, seq, d_words, pos, ntok=d_ntok, ntok_bias=-1, ban=d_ban if use_ban else None, no_repeat=rep, repeat_min_id=7, row_chosen=chosen,
                              moved=moved)
            torch.cuda.synchronize()
            assert np.array_equal(seq.cpu().numpy().reshape(B, S), want["seq"]), what
            assert np.array_equal(chosen.cpu().numpy().reshape(B, S).view(np.int32), want["chosen"].view(np.int32)), what
            assert np.array_equal(pos.cpu().numpy(), want["pos"]), what
            assert np.array_equal(moved.cpu().numpy(), want["moved"]), what
        assert np.array_equal(dx.cpu().numpy().view(np.int32), x.reshape(B * S, ldx).view(np.int32))      # (x is read only)
    # optional outputs and ntok left out; another floor for the adjacency rule
    seq = torch.from_numpy(old.copy()).cuda().view(-1)
    pos = torch.full((B, K), -9, dtype=torch.int32, device="cuda")
    hip.vocab_require(dx, V, S, seq, d_words, pos, no_repeat=True, repeat_min_id=0)
    torch.cuda.synchronize()
    full = require_np(x[:, :, :V], np.full(B, S), words, old, (), True, 0)
    assert np.array_equal(seq.cpu().numpy().reshape(B, S), full["seq"]) and np.array_equal(pos.cpu().numpy(), full["pos"])


# ----------------------------------------------------------------------------- 2. the float32 engine against the restated decode
def words_of(lp, n, seq):
    """The word rule of the engine tests, per image, from a plain decode's log-probs lp [B, S, V], live counts and ids: an id the decode emits at exactly ONE position of
    the image (-1 where it has none: an id that stands twice is an exact tie between its positions, margin 0), the runner-up id of the middle live position, and an id
    that leads nowhere (V - 1 - b).  int32 [B, 3]."""
    B, _, V = lp.shape
    words = np.full((B, 3), -1, np.int32)
    for b in range(B):
        live = [int(v) for v in seq[b, :n[b]]]
        once = [v for v in live if v >= 7 and live.count(v) == 1]
        words[b, 0] = once[0] if once else -1
        words[b, 1] = int(order_np(lp[b, int(n[b]) // 2])[1]) if n[b] else -1
        words[b, 2] = V - 1 - b
    return words


@functools.lru_cache(maxsize=None)
def restated(name):
    """The decode of golden case ``name`` with the words of ``words_of``: require_np on the oracle's own log-probs and plain ids; ``safe`` [B]: the placement's margin AND
    every plain pick's margin exceed MARGIN."""
    base = plain_of(name)
    words = words_of(base["lp"], base["n"], base["seq"])
    r = require_np(base["lp"], base["n"], words, base["seq"])
    r["words"], r["safe"] = words, (r["margin"] > MARGIN) & (pick_np(base["lp"], base["n"], pad=base["cfg"].pad_idx)["margin"] > MARGIN)
    return r


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


@pytest.mark.parametrize("name", ["tiny_saic_multi", "full_b8"])
def test_f32_engine_equals_the_restated_decode(name, f32_engines):
    """seq and pos on the images whose restated margin exceeds MARGIN = 1e-3; at most a quarter of the images may be left out (5 of 6 and 7 of 8 are compared: checked on
    the oracle alone).  The goldens' untrained captions repeat every id they emit, so the rule's first word is absent here; words that stand in seq already are covered by
    the kernel test and the bf16 engine below."""
    base, ref = plain_of(name), restated(name)
    eng = f32_engines(name)
    att = base["att"].cuda()
    att_len = None if base["masks"] is None else base["masks"].sum(1).to(torch.int32).cuda()
    r = eng.decode_naic(att, att_len, row_stats=True, require_ids=torch.from_numpy(ref["words"]).cuda())
    torch.cuda.synchronize()
    for k in LAYOUT:
        assert torch.equal(r[k].cpu(), base[k]), k
    safe = ref["safe"]
    print(f"required words {name}: margins {np.round(ref['margin'], 5).tolist()}, safe {int(safe.sum())} of {len(safe)}, placed {int((ref['pos'] >= 0).sum())}, "
          f"moved {int(ref['moved'].sum())}")
    assert 4 * int((~safe).sum()) <= len(safe)
    assert np.array_equal(r["seq"].cpu().numpy()[safe], ref["seq"][safe])
    assert np.array_equal(r["required_pos"].cpu().numpy()[safe], ref["pos"][safe])
    assert np.array_equal(r["required_moved"].cpu().numpy()[safe], ref["moved"][safe])
    assert int(ref["moved"][safe].sum()) > 0 and (ref["pos"][safe] >= 0).sum() >= safe.sum()


# ----------------------------------------------------------------------------- 3. the bf16 engine, without a tolerance
@pytest.fixture(scope="module")
def bf16_full(weight_cache, manifest):
    """The full-size bf16 engine on full_b8's weights and 16 synthetic images, with the plain decodes made BEFORE any call with require_ids on this engine, and the word
    table [16, 4]: an id the image emits, the runner-up of its middle position, an id that leads nowhere, and one word for all."""
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
    before = {"pick": _clone(eng.decode_naic(att, row_stats=True, ban_ids=[top], no_repeat=True)), "T1": _clone(eng.decode_naic(att, row_stats=True, refine_rounds=1))}
    torch.cuda.synchronize()
    lp, seq, n = plain["seq_logprob"].cpu().numpy(), plain["seq"].cpu().numpy(), plain["phrase_length"].sum(1).cpu().numpy()
    words = np.full((16, 4), -1, np.int32)
    for b in range(16):
        emitted = [int(v) for v in seq[b, :n[b]] if v >= 7 and v != top]
        words[b, 0] = emitted[len(emitted) // 2] if emitted else -1
        words[b, 1] = int(order_np(lp[b, int(n[b]) // 2])[1]) if n[b] else -1
        words[b, 2] = cfg.tgt_vocab - 1 - b
        words[b, 3] = 4242
    return cfg, eng, att, plain, top, before, words


def _holds_the_rule(cfg, r, base, words, ban=(), rep=False, min_id=7):
    """``r`` (a decode with require_ids) against ``base`` (the same decode without): the log-probs are bit-equal, and seq, row_chosen, pos and moved of ``r`` equal
    require_np on those log-probs and base's ids, bit for bit.  Every placed word stands at its pos, no banned id is emitted, and under no_repeat no word stands twice in
    a row."""
    lp = r["seq_logprob"].cpu().numpy()
    assert torch.equal(_bits(r["seq_logprob"]), _bits(base["seq_logprob"])) and _same_bits(r, base, LAYOUT)
    n = r["phrase_length"].sum(1).cpu().numpy()
    want = require_np(lp, n, words, base["seq"].cpu().numpy(), ban, rep, min_id, chosen=base["row_chosen"].cpu().numpy())
    seq = r["seq"].cpu().numpy()
    assert np.array_equal(seq, want["seq"])
    assert np.array_equal(r["row_chosen"].cpu().numpy().view(np.int32), want["chosen"].view(np.int32))
    assert np.array_equal(r["required_pos"].cpu().numpy(), want["pos"]) and np.array_equal(r["required_moved"].cpu().numpy(), want["moved"])
    assert torch.equal(_bits(r["row_plogp"]), _bits(base["row_plogp"]))
    pos = want["pos"]
    for b, j in zip(*np.nonzero(pos >= 0)):
        assert seq[b, pos[b, j]] == words[b, j]
    assert not np.isin(seq, np.asarray(list(ban), np.int64)).any()
    if rep:
        assert sum(int(seq[b, s] == seq[b, s - 1] and seq[b, s] >= min_id) for b in range(len(n)) for s in range(1, int(n[b]))) == 0
    return want


def test_bf16_engine_holds_the_rule_graph_fork_phases_fill(bf16_full):
    cfg, eng, att, plain, top, before, words = bf16_full
    table = torch.from_numpy(words).cuda()
    kw = dict(row_stats=True, require_ids=table)
    keys = ("seq", "row_plogp", "row_chosen", "seq_logprob", "required_pos", "required_moved") + LAYOUT
    r = _clone(eng.decode_naic(att, **kw))
    torch.cuda.synchronize()
    want = _holds_the_rule(cfg, r, plain, words)
    assert int(want["moved"].sum()) > 0 and int((want["pos"] >= 0).sum()) > int(want["moved"].sum())      # words were moved in, and words stood there already
    as_lists = eng.decode_naic(att, row_stats=True, require_ids=[[int(v) for v in row if v >= 0] for row in words])      # host lists give the same table
    torch.cuda.synchronize()
    assert _same_bits(as_lists, r, ("seq", "row_chosen", "required_moved", "seq_logprob"))      # (the host table drops a row's duplicates: its columns may differ)
    # ban_ids + no_repeat: the placement follows the constrained pick, is handed its table and rule, and reads the emitted ids
    q = eng.decode_naic(att, ban_ids=[top], no_repeat=True, **kw)
    torch.cuda.synchronize()
    _holds_the_rule(cfg, q, before["pick"], words, (top,), True)
    assert torch.equal(q["constrained"], before["pick"]["constrained"])
    # one feed-back round: the last pass alone is placed on; the earlier pass was fed the unforced ids
    q = eng.decode_naic(att, refine_rounds=1, **kw)
    torch.cuda.synchronize()
    _holds_the_rule(cfg, q, before["T1"], words)
    # graph: captured, then replayed; the post-pass stays outside the graph
    g = eng.decode_naic(att, graph=True, **kw)
    g = eng.decode_naic(att, graph=True, out=g, **kw)
    torch.cuda.synchronize()
    assert _same_bits(g, r, keys)
    # a fork on its own stream
    f = eng.fork()
    st = f.stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        fo = f.decode_naic(att, **kw)
    st.synchronize()
    assert _same_bits(fo, r, keys)
    # no log-prob tensor asked for: the engine's own workspace is read
    nl = eng.decode_naic(att, want_logprob=False, **kw)
    torch.cuda.synchronize()
    assert nl["seq_logprob"] is None and _same_bits(nl, r, tuple(k for k in keys if k != "seq_logprob"))
    # the phased form: the filling phase owns the launch
    ph = eng.decode_naic(att, phases="e", **kw)
    assert "required_pos" not in ph
    ph = eng.decode_naic(att, phases="b", out=ph, **kw)
    ph = eng.decode_naic(att, phases="f", out=ph, **kw)
    torch.cuda.synchronize()
    assert _same_bits(ph, r, keys)
    # the filling pass alone on the decode's own layout
    ext, last = O.layout_of(cfg, plain)
    eng.encode(att)
    fr = eng.fill_naic(ext.to(torch.int32).cuda(), torch.from_numpy(last).to(torch.int32).cuda(), att.size(1), require_ids=table)
    torch.cuda.synchronize()
    assert len(fr) == 3 and torch.equal(fr[0], r["seq"]) and torch.equal(_bits(fr[1]), _bits(r["seq_logprob"]))
    assert torch.equal(fr[2]["required_pos"], r["required_pos"]) and torch.equal(fr[2]["required_moved"], r["required_moved"])
    # raw logits: the normaliser cancels within a position
    raw = eng.decode_naic(att, raw_logits=True, require_ids=table)
    raw0 = eng.decode_naic(att, raw_logits=True)
    torch.cuda.synchronize()
    lg, nn = raw["seq_logprob"].cpu().numpy(), raw["phrase_length"].sum(1).cpu().numpy()
    w = require_np(lg, nn, words, raw0["seq"].cpu().numpy())
    assert np.array_equal(raw["seq"].cpu().numpy(), w["seq"]) and np.array_equal(raw["required_pos"].cpu().numpy(), w["pos"])


def test_off_is_the_decode_as_it_was(bf16_full):
    """require_ids None, [], and rows of -1 only add no keys and give the outputs of the decodes made before any required-words call on this engine, bit for bit."""
    cfg, eng, att, plain, top, before, words = bf16_full
    keys = ("seq", "seq_logprob", "row_plogp", "row_chosen") + LAYOUT
    used = eng.decode_naic(att, row_stats=True, require_ids=torch.from_numpy(words).cuda())      # (a call with the option in between, and its dict reused below)
    assert "required_pos" in used
    for off in (None, [], [[-1, -1]] * 16, [[]] * 16, np.full((16, 3), -1)):
        r = eng.decode_naic(att, row_stats=True, require_ids=off)
        torch.cuda.synchronize()
        assert _same_bits(r, plain, keys) and "required_pos" not in r and "required_moved" not in r and "constrained" not in r
    r = eng.decode_naic(att, row_stats=True, out=used)
    torch.cuda.synchronize()
    assert _same_bits(r, plain, keys) and "required_pos" not in r and "required_moved" not in r
    r = eng.decode_naic(att, row_stats=True, ban_ids=[top], no_repeat=True, require_ids=[])
    torch.cuda.synchronize()
    assert _same_bits(r, before["pick"], keys) and torch.equal(r["constrained"], before["pick"]["constrained"]) and "required_pos" not in r


def test_engine_refuses_what_required_words_exclude(bf16_full):
    from boficap_amd import hip
    from boficap_amd.engine import DecodePipeline
    cfg, eng, att, plain, top, before, words = bf16_full
    a = att[:4].contiguous()
    with pytest.raises(hip.BofiHipError, match="ids_only"):
        eng.decode_naic(a, ids_only=True, require_ids=[9])
    with pytest.raises(hip.BofiHipError, match="mask_predict"):
        eng.decode_naic(a, refine_rounds=2, refine_method="mask_predict", require_ids=[9])
    with pytest.raises(hip.BofiHipError, match="block_trigrams"):
        eng.decode_naic(a, block_trigrams=True, require_ids=[9])
    with pytest.raises(hip.BofiHipError, match="ban_ids"):
        eng.decode_naic(a, ban_ids=[9], require_ids=[9])
    with pytest.raises(hip.BofiHipError, match="0.."):
        eng.decode_naic(a, require_ids=[cfg.tgt_vocab])
    with pytest.raises(hip.BofiHipError, match="at most 8"):
        eng.decode_naic(a, require_ids=list(range(10, 19)))
    with pytest.raises(hip.BofiHipError, match="K"):
        eng.decode_naic(a, require_ids=torch.zeros(4, 9, dtype=torch.int32, device="cuda"))
    with pytest.raises(hip.BofiHipError, match="mask_predict"):
        eng.fill_naic(torch.zeros(4, cfg.bound_len, dtype=torch.int32, device="cuda"), torch.ones(4, dtype=torch.int32, device="cuda"), 36, refine_rounds=2,
                      refine_method="mask_predict", require_ids=[9])
    for kw, word in ((dict(fused_vocab=True), "fused_vocab"), (dict(refine_rounds=2, refine_method="mask_predict"), "mask_predict"), (dict(block_trigrams=True), "block_trigrams")):
        with pytest.raises(hip.BofiHipError, match=word):
            DecodePipeline(eng, require_ids=[9], **kw)
        with pytest.raises(hip.BofiHipError, match=word):
            DecodePipeline(eng, **kw).run([a], require_ids=[9])      # (raised by the call, before the generator is advanced)
    torch.cuda.synchronize()
    assert torch.equal(eng.decode_naic(att)["seq"], plain["seq"])   # nothing was enqueued: the engine decodes as before
    # a device table goes through unchecked: the kernel classifies it
    t = torch.tensor([[top, top, cfg.tgt_vocab, -1]] * 4, dtype=torch.int32, device="cuda")
    r = eng.decode_naic(a, ban_ids=[top], require_ids=t)
    torch.cuda.synchronize()
    assert r["required_pos"].cpu().tolist() == [[-2, -2, -2, -1]] * 4 and int(r["required_moved"].sum()) == 0 and not (r["seq"] == top).any()


# ----------------------------------------------------------------------------- 4. above the engine
def test_interface_gives_the_engine_level_result(weight_cache, monkeypatch):
    """decode_many with per-batch tables (grouped batches in one launch, a ragged tail, a batch without words) and mode='sample' with opt['require_ids'] against
    BofiEngine.decode_naic on the same batches, same kernel family and hint."""
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
        feats = torch.from_numpy(W.synthetic_att_feats(8 + 8 + 8 + 5, 36, cfg.att_feat_size, seed=79)).to(torch.bfloat16)
        batches = [feats[:8], feats[8:16], feats[16:24], feats[24:]]      # three batches of 8 (one launch carries them) and a tail of 5 ...
        tail_masks = torch.ones(5, 36)
        tail_masks[1, 9:] = 0; tail_masks[4, 30:] = 0           # ... which is ragged
        ref = BofiEngine(cfg, torch.bfloat16, max_batch=16, max_regions=36)
        ref.load_state_dict(sd)
        ref.set_decodes_in_flight(2)
        lens = lambda i: tail_masks.sum(1).to(torch.int32).cuda() if i == 3 else None
        plain = [ref.decode_naic(b.cuda(), lens(i))["seq"].cpu() for i, b in enumerate(batches)]
        tables = [[[4242, 77]] * 8, None, [[int(plain[2][k, 0])] if k % 2 else [] for k in range(8)], [901, 902, 903]]      # per-image lists, none, some empty, one flat list
        want = []
        for i, b in enumerate(batches):
            r = ref.decode_naic(b.cuda(), lens(i), row_stats=True, no_repeat=True, require_ids=tables[i])
            want.append({k: v.cpu() for k, v in r.items() if torch.is_tensor(v)})
        items = [batches[0].pin_memory(), batches[1].pin_memory(), batches[2].pin_memory(), (batches[3].pin_memory(), tail_masks)]
        got = list(model.decode_many(items, batches_per_launch=3, in_flight=2, no_repeat=True, require_ids=tables))
        assert len(got) == 4
        for i, (g, w) in enumerate(zip(got, want)):
            for k in ("seq", "constrained") + LAYOUT + (("required_pos", "required_moved") if tables[i] is not None else ()):
                assert torch.equal(g[k], w[k]), (i, k)
            assert ("required_pos" in g) == (tables[i] is not None)
        assert got[0]["required_pos"].shape == (8, 2) and got[2]["required_pos"].shape == (8, 1) and got[3]["required_pos"].shape == (5, 3)
        assert any(not torch.equal(g["seq"], p) for g, p in zip(got, plain))
        flat = list(model.decode_many(items, batches_per_launch=3, in_flight=2, require_ids=[901, 902]))      # one flat list: every image of every batch
        for i, (g, b) in enumerate(zip(flat, batches)):
            e = ref.decode_naic(b.cuda(), lens(i), require_ids=[901, 902])
            assert torch.equal(g["seq"], e["seq"].cpu()) and torch.equal(g["required_pos"], e["required_pos"].cpu())
        again = list(model.decode_many(items, batches_per_launch=3, in_flight=2))               # the defaults stay the plain decode
        assert all(torch.equal(g["seq"], p) and "required_pos" not in g for g, p in zip(again, plain))
        for kw, word in ((dict(fused_vocab=True), "fused_vocab"), (dict(block_trigrams=True), "block_trigrams"), (dict(refine_rounds=2, refine_method="mask_predict"), "mask_predict")):
            with pytest.raises(H.BofiHipError, match=word):
                model.decode_many(items, require_ids=[901], **kw)
        with pytest.raises(H.BofiHipError, match="fewer"):
            list(model.decode_many(items, require_ids=[[901], [902]]))
        # mode='sample'
        fc = torch.zeros(5, 0, device="cuda")
        out = model(fc, batches[3].cuda(), tail_masks.cuda(), opt={"train_mode": "NAIC", "require_ids": [901, 902, 903]}, mode="sample")
        assert len(out) == 6
        last = {k: v.clone() for k, v in model.last_required.items()}
        e = model.engine().decode_naic(batches[3].cuda(), lens(3), require_ids=[901, 902, 903])
        torch.cuda.synchronize()
        assert torch.equal(out[0], e["seq"]) and torch.equal(last["pos"], e["required_pos"]) and torch.equal(last["moved"], e["required_moved"])
        assert int(last["moved"].sum()) > 0 and sorted(last) == ["moved", "pos"]
        out3 = model(fc, batches[3].cuda(), tail_masks.cuda(), opt={"train_mode": "NAIC", "require_ids": [901], "sample_n": 3}, mode="sample")
        assert out3[0].shape[0] == 15 and model.last_required["pos"].shape == (15, 1) and torch.equal(model.last_required["pos"][::3], model.last_required["pos"][2::3])
        model(fc, batches[3].cuda(), tail_masks.cuda(), opt={"train_mode": "NAIC"}, mode="sample")
        assert model.last_required is None
        model(fc, batches[3].cuda(), tail_masks.cuda(), opt={"train_mode": "NAIC", "require_ids": []}, mode="sample")
        assert model.last_required is None
        for bad in ({"train_mode": "NAIC", "require_ids": [901], "sample_method": "sample"},
                    {"train_mode": "NAIC", "require_ids": [901], "refine_rounds": 2, "refine_method": "mask_predict"}, {"train_mode": "SAIC", "require_ids": [901]}):
            with pytest.raises(H.BofiHipError, match="require_ids"):
                model(fc, batches[3].cuda(), tail_masks.cuda(), opt=bad, mode="sample")
    finally:
        monkeypatch.undo()
        H.lib().bofi_reload_env()


def test_eval_split_places_required_words():
    from boficap_amd import eval_utils
    from boficap_amd.config import TINY
    from test_gpu_lang_eval import tiny_model
    labels = eval_utils.SyntheticLabels(TINY, 8, 5, seed=3)
    model = tiny_model()
    base = {"batch_size": 4, "language_eval": 1, "verbose_loss": 0}
    _, preds0, stats0 = eval_utils.eval_split(model, labels.feats, labels, dict(base))
    spec = {0: ["w30", "w31"], "3": ["w32"], 6: "w33,w34,w35"}
    _, preds, stats = eval_utils.eval_split(model, labels.feats, labels, dict(base, require_words=spec))
    assert "required_rate" not in stats0 and list(stats)[:-2] == list(stats0) and list(stats)[-2:] == ["required_rate", "required_moved_rate"]
    host = torch.from_numpy(labels.feats)
    ids = [[30, 31], [], [], [32], [], [], [33, 34, 35], []]
    got = list(model.decode_many([host[i:i + 4] for i in range(0, 8, 4)], require_ids=[ids[:4], ids[4:]]))
    pos = [row for g in got for row in g["required_pos"]]        # (every batch has its own K: 2 and 3 here)
    assert got[0]["required_pos"].shape == (4, 2) and got[1]["required_pos"].shape == (4, 3)
    placed = sum(int(pos[k][j] >= 0) for k in range(8) for j in range(len(ids[k])))
    assert stats["required_rate"] == placed / 6 and placed > 0
    assert stats["required_moved_rate"] == sum(int(g["required_moved"].sum()) for g in got) / sum(int(g["phrase_length"].sum()) for g in got)
    assert [p["seq"] for p in preds] == [[int(v) for v in row.tolist()[:next((q for q, v in enumerate(row.tolist()) if v <= 0), len(row))]] for g in got for row in g["seq"]]
    assert preds != preds0 and "required" not in preds0[0]
    assert [p["required"] for p in preds] == [[[f"w{w}", (int(pos[k][j]) if pos[k][j] >= 0 else None)] for j, w in enumerate(ids[k])] for k in range(8)]
    for p in preds:
        for w, where in p["required"]:
            assert where is None or p["seq"][where] == int(w[1:])
    _, _, only = eval_utils.eval_split(model, labels.feats, labels, {"batch_size": 4, "verbose_loss": 0, "require_words": "w30"})
    assert sorted(only) == ["required_moved_rate", "required_rate"]      # (no language scores asked for: the two rates alone)
    with pytest.raises(ValueError, match="NAIC"):
        eval_utils.eval_split(model, labels.feats, labels, dict(base, inference_mode="SAIC", require_words="w30"))
    with pytest.raises(ValueError, match="w99"):
        eval_utils.eval_split(model, labels.feats, labels, dict(base, require_words="w99"))
