"""Required phrases on the MI355X: bofi_vocab_require_units against the numpy restatement of tests/test_required_phrases.py (bit for bit) and, on units of length 1,
against bofi_vocab_require; the float32 engine against the restated decode on the golden cases; the bf16 engine held without a tolerance to ``require_units_np`` on its
OWN returned log-probs (graph replay, fork, filling pass alone, feed-back, grouped batches through decode_many); "off is today's decode"; the refusals; and the interface
above the engine (mode='sample', eval_split)."""
import functools

import numpy as np
import pytest
import torch

import boficap_oracle as O
from test_constrained_pick import MARGIN, order_np, pick_np, plain_of
from test_gpu_constrained_pick import KEEP, LAYOUT, _bits, _clone, _same_bits
from test_gpu_required_words import _kernel_case, bf16_full, f32_engines      # noqa: F401  (the fixtures: an engine per module)
from test_required_phrases import classify_units_np, require_units_np

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------- 1. the kernel
def _units_case(rng, B, S, V, ldx, K, L):
    """The data of ``_kernel_case`` (tie-rich x with NaN and +-inf, poison past column V, ids outside the vocabulary in seq, ntok with a bias and clamped both ways, n = 0
    and 1) with its word rows grown into units [B, K, L]: a unit's first id is the row's word (with its empties, ids >= V and 2^31 - 1), the further ids come from the
    same small pool (units overlap each other's ids, repeat a word, could meet), a random length with garbage behind the first negative id, ids >= V inside a unit, a
    duplicated unit on every fourth image, and on every third image a unit that already stands in seq.  Image 0's first unit has two ids, of which the first stands."""
    x, seq, words, n, ntok, ban = _kernel_case(rng, B, S, V, ldx, K)
    pool = np.arange(4, min(V, 4 + max(6, S // 2)))
    units = rng.choice(pool, (B, K, L)).astype(np.int32)
    units[:, :, 0] = words
    for b in range(B):
        for k in range(K):
            ln = int(rng.integers(1, L + 1))
            if ln < L:
                units[b, k, ln] = -1 - int(rng.integers(0, 3))  # (what stands behind it is not read)
    units[:, :, 1:][rng.random((B, K, L - 1)) < 0.04] = V
    for b in range(1, B, 4):
        if K >= 2:
            units[b, 1] = units[b, 0]
    for b in range(3, B, 3):                                    # the whole unit stands around the middle live position and is costly everywhere else
        u = [int(v) for v in units[b, 0, :next((i for i, v in enumerate(units[b, 0]) if v < 0), L)]]
        if u and max(u) < V and len(u) <= n[b] and len(set(u)) == len(u):
            p0 = min(int(n[b]) // 2, int(n[b]) - len(u))
            x[b, :, u] = -8.0
            for i, w in enumerate(u):
                seq[b, p0 + i] = w
                x[b, p0 + i, w] = 0.0
    if L >= 2:                                                  # image 0 (n = S): its first id stands at S // 2 (``_kernel_case``), the second is moved in beside it
        units[0, 0, :2] = [pool[1], pool[2]]
        if L > 2:
            units[0, 0, 2] = -1
        if S // 2 + 1 < S:
            seq[0, S // 2 + 1] = pool[3]
            x[0, S // 2 + 1, pool[3]], x[0, S // 2 + 1, pool[2]] = -0.125, -0.25
    if B == 2 and L > S:
        units[1, 0] = pool[:L]                                  # a unit longer than S: kept, never placeable
    return x, seq, units, n, ntok, ban


UNIT_CASES = [(1, 20, 64, 64, 1, 2), (5, 20, 9491, 9491, 4, 3), (3, 64, 9491, 9600, 8, 4), (130, 20, 257, 257, 3, 4), (2, 3, 64, 64, 2, 4)]


@pytest.mark.parametrize("B,S,V,ldx,K,L", UNIT_CASES)
def test_kernel_equals_require_units_np(B, S, V, ldx, K, L):
    """seq, row_chosen (the untouched entries included), pos and moved bit for bit: with and without a ban table, no_repeat, ntok, row_chosen and moved; ntok read with a
    bias and clamped; for the small-B shapes the tensor 0..3 floats off a 16-byte boundary; x is read only.  (3, 64, 9491, 9600, 8, 4) is the LDS ceiling (one image per
    workgroup), (130, ...) has the partial last workgroup, (2, 3, ...) units longer than S."""
    from boficap_amd import hip
    rng = np.random.default_rng(9000 + 100 * B + S + V + K + L)
    x, old, units, n, ntok, ban = _units_case(rng, B, S, V, ldx, K, L)
    d_ntok, d_ban, d_units = torch.from_numpy(ntok).cuda(), hip.ban_bits(ban, V, "cuda"), torch.from_numpy(units).cuda()
    keep = np.full((B, S), KEEP, np.float32)
    wants = {(use_ban, rep): require_units_np(x[:, :, :V], n, units, old, ban if use_ban else (), rep, 7, chosen=keep) for use_ban in (False, True) for rep in (False, True)}
    w = wants[(False, False)]
    kinds = [k for b in range(B) for k in classify_units_np(units[b], V, ())]
    lens = [len(k) for k in kinds if isinstance(k, list)]
    print(f"required units kernel {(B, S, V, ldx, K, L)}: {int((w['pos'] >= 0).sum())} placed, {int((w['pos'] == -3).sum())} unplaceable, {kinds.count(-2)} skipped, "
          f"{kinds.count(-1)} empty, unit lengths {np.bincount(lens, minlength=L + 1).tolist()}, {int(w['moved'].sum())} moved, "
          f"{int((w['margin'] == 0).sum())} of {B} images with an exact tie; {int((wants[(False, True)]['seq'] != w['seq']).sum())} positions differ under no_repeat, "
          f"{int((wants[(True, False)]['seq'] != w['seq']).sum())} under the ban")
    # not vacuous: something was placed, something moved, something was skipped or unplaceable (for B = 1, K = 1 the ban variant supplies the skip)
    assert int((w["pos"] >= 0).sum()) > 0 and int(w["moved"].sum()) > 0
    assert int((w["pos"] <= -2).sum()) > 0 or (B == 1 and int((wants[(True, False)]["pos"] == -2).sum()) > 0)
    assert (wants[(True, False)]["pos"] == -2).sum() > (w["pos"] == -2).sum()         # the ban table skips units
    if L >= 2:
        assert max(lens) >= 2 and any(isinstance(k, list) and len(k) >= 2 and w["pos"].reshape(-1)[i] >= 0 for i, k in enumerate(kinds))      # a multi-word unit was placed
    if B >= 5:
        assert (w["pos"] == -3).any() and kinds.count(-2) and kinds.count(-1)
    if B * K >= 24:                                             # enough units for some to repeat a word or to meet another: skipped under no_repeat alone
        assert (wants[(False, True)]["pos"] == -2).sum() > (w["pos"] == -2).sum()
    for off in ((0, 1, 2, 3) if B <= 5 else (0,)):
        buf = torch.full((B * S * ldx + 8,), 7.0, dtype=torch.float32, device="cuda")
        dx = buf[off:off + B * S * ldx].view(B * S, ldx)
        dx.copy_(torch.from_numpy(x.reshape(B * S, ldx)))
        for (use_ban, rep), want in wants.items():
            what = (B, S, V, ldx, K, L, off, use_ban, rep)
            seq = torch.from_numpy(old.copy()).cuda().view(-1)
            chosen = torch.full((B * S,), KEEP, dtype=torch.float32, device="cuda")
            pos = torch.full((B, K), -9, dtype=torch.int32, device="cuda")
            moved = torch.full((B,), -9, dtype=torch.int32, device="cuda")
            hip.vocab_require_units(dx, V, S, seq, d_units, pos, ntok=d_ntok, ntok_bias=-1, ban=d_ban if use_ban else None, no_repeat=rep, repeat_min_id=7,
                                    row_chosen=chosen, moved=moved)
            torch.cuda.synchronize()
            assert np.array_equal(seq.cpu().numpy().reshape(B, S), want["seq"]), what
            assert np.array_equal(chosen.cpu().numpy().reshape(B, S).view(np.int32), want["chosen"].view(np.int32)), what
            assert np.array_equal(pos.cpu().numpy(), want["pos"]), what
            assert np.array_equal(moved.cpu().numpy(), want["moved"]), what
        assert np.array_equal(dx.cpu().numpy().view(np.int32), x.reshape(B * S, ldx).view(np.int32))      # (x is read only)
    # optional outputs and ntok left out; another floor for the adjacency rule
    seq = torch.from_numpy(old.copy()).cuda().view(-1)
    pos = torch.full((B, K), -9, dtype=torch.int32, device="cuda")
    hip.vocab_require_units(dx, V, S, seq, d_units, pos, no_repeat=True, repeat_min_id=0)
    torch.cuda.synchronize()
    full = require_units_np(x[:, :, :V], np.full(B, S), units, old, (), True, 0)
    assert np.array_equal(seq.cpu().numpy().reshape(B, S), full["seq"]) and np.array_equal(pos.cpu().numpy(), full["pos"])


@pytest.mark.parametrize("B,S,V,ldx,K", [(5, 20, 9491, 9491, 4), (3, 64, 9491, 9600, 8), (130, 20, 257, 257, 3)])
def test_units_of_length_one_equal_the_words_kernel(B, S, V, ldx, K):
    """bofi_vocab_require_units on [B, K, 1] -- and on [B, K, 3] with -1 behind every id -- equals bofi_vocab_require on the same inputs, bit for bit: seq, row_chosen,
    pos, moved; with and without the ban table and no_repeat."""
    from boficap_amd import hip
    rng = np.random.default_rng(7000 + 100 * B + S + V + K)
    x, old, words, n, ntok, ban = _kernel_case(rng, B, S, V, ldx, K)
    dx, d_ntok, d_ban, d_words = torch.from_numpy(x.reshape(B * S, ldx)).cuda(), torch.from_numpy(ntok).cuda(), hip.ban_bits(ban, V, "cuda"), torch.from_numpy(words).cuda()
    wide = torch.full((B, K, 3), -1, dtype=torch.int32, device="cuda")
    wide[:, :, 0] = d_words
    placed = 0
    for use_ban in (False, True):
        for rep in (False, True):
            got = []
            for table in (d_words, d_words.view(B, K, 1).contiguous(), wide):
                seq = torch.from_numpy(old.copy()).cuda().view(-1)
                chosen = torch.full((B * S,), KEEP, dtype=torch.float32, device="cuda")
                pos = torch.full((B, K), -9, dtype=torch.int32, device="cuda")
                moved = torch.full((B,), -9, dtype=torch.int32, device="cuda")
                call = hip.vocab_require if table.dim() == 2 else hip.vocab_require_units
                call(dx, V, S, seq, table, pos, ntok=d_ntok, ntok_bias=-1, ban=d_ban if use_ban else None, no_repeat=rep, repeat_min_id=7, row_chosen=chosen, moved=moved)
                torch.cuda.synchronize()
                got.append((seq.cpu(), chosen.cpu().view(torch.int32), pos.cpu(), moved.cpu()))
            for other in got[1:]:
                assert all(torch.equal(a, b) for a, b in zip(got[0], other)), (use_ban, rep)
            placed += int((got[0][2] >= 0).sum())
    assert placed > 0


# ----------------------------------------------------------------------------- 2. the float32 engine against the restated decode
def units_of(lp, n, seq):
    """The unit rule of the engine tests, per image, from a plain decode's log-probs lp [B, S, V], live counts and ids -- int32 [B, 3, 3]: the runner-up ids of the
    middle live position and of the one behind it, side by side (a phrase the pass nearly said); three ids that lead nowhere (V - 1 - 3b ..: the cheapest span decides);
    a bigram of words that the caption emits exactly ONCE (it stands: gain 0; a bigram that stands twice would be an exact tie between its places, margin 0; -1 where
    the caption has none).  (Single ids such as a position's runner-up tie exactly on untrained weights, whose rows repeat: they are left to the kernel tests.)"""
    B, _, V = lp.shape
    units = np.full((B, 3, 3), -1, np.int32)
    for b in range(B):
        nb = int(n[b])
        if nb >= 2:
            units[b, 0, :2] = [int(order_np(lp[b, nb // 2 - 1])[1]), int(order_np(lp[b, nb // 2])[1])]
        units[b, 1] = [V - 1 - 3 * b, V - 2 - 3 * b, V - 3 - 3 * b]
        live = [int(v) for v in seq[b, :nb]]
        grams = [(live[p], live[p + 1]) for p in range(nb - 1)]
        once = [g for g in grams if min(g) >= 7 and g[0] != g[1] and grams.count(g) == 1]
        if once:
            units[b, 2, :2] = once[len(once) // 2]
    return units


@functools.lru_cache(maxsize=None)
def restated(name):
    """The decode of golden case ``name`` with the units of ``units_of``: require_units_np on the oracle's own log-probs and plain ids; ``safe`` [B]: the placement's
    margin AND every plain pick's margin exceed MARGIN."""
    base = plain_of(name)
    units = units_of(base["lp"], base["n"], base["seq"])
    r = require_units_np(base["lp"], base["n"], units, base["seq"])
    r["units"], r["safe"] = units, (r["margin"] > MARGIN) & (pick_np(base["lp"], base["n"], pad=base["cfg"].pad_idx)["margin"] > MARGIN)
    return r


@pytest.mark.parametrize("name", ["tiny_saic_multi", "full_b8"])
def test_f32_engine_equals_the_restated_decode(name, f32_engines):
    """seq, pos and moved on the images whose restated margin exceeds MARGIN = 1e-3; at most a quarter of the images may be left out."""
    base, ref = plain_of(name), restated(name)
    eng = f32_engines(name)
    att = base["att"].cuda()
    att_len = None if base["masks"] is None else base["masks"].sum(1).to(torch.int32).cuda()
    r = eng.decode_naic(att, att_len, row_stats=True, require_phrases=torch.from_numpy(ref["units"]).cuda())
    torch.cuda.synchronize()
    for k in LAYOUT:
        assert torch.equal(r[k].cpu(), base[k]), k
    safe = ref["safe"]
    print(f"required phrases {name}: margins {np.round(ref['margin'], 5).tolist()}, safe {int(safe.sum())} of {len(safe)}, placed {int((ref['pos'] >= 0).sum())}, "
          f"moved {int(ref['moved'].sum())}")
    assert 4 * int((~safe).sum()) <= len(safe)
    assert np.array_equal(r["seq"].cpu().numpy()[safe], ref["seq"][safe])
    assert np.array_equal(r["required_pos"].cpu().numpy()[safe], ref["pos"][safe])
    assert np.array_equal(r["required_moved"].cpu().numpy()[safe], ref["moved"][safe])
    assert int(ref["moved"][safe].sum()) > 0 and (ref["pos"][safe] >= 0).sum() >= safe.sum()


# ----------------------------------------------------------------------------- 3. the bf16 engine, without a tolerance
def _holds_the_rule(r, base, units, ban=(), rep=False, min_id=7):
    """``r`` (a decode with require_phrases) against ``base`` (the same decode without): the log-probs are bit-equal; pos, moved and -- on the images whose margin is not
    an exact 0, at least three quarters -- seq and row_chosen equal require_units_np on those log-probs and base's ids, bit for bit.  Every placed unit stands at its pos."""
    lp = r["seq_logprob"].cpu().numpy()
    assert torch.equal(_bits(r["seq_logprob"]), _bits(base["seq_logprob"])) and _same_bits(r, base, LAYOUT)
    n = r["phrase_length"].sum(1).cpu().numpy()
    want = require_units_np(lp, n, units, base["seq"].cpu().numpy(), ban, rep, min_id, chosen=base["row_chosen"].cpu().numpy())
    sure = want["margin"] != 0.0
    assert 4 * int((~sure).sum()) <= len(sure), want["margin"]
    seq = r["seq"].cpu().numpy()
    assert np.array_equal(seq[sure], want["seq"][sure])
    assert np.array_equal(r["row_chosen"].cpu().numpy().view(np.int32)[sure], want["chosen"].view(np.int32)[sure])
    assert np.array_equal(r["required_pos"].cpu().numpy()[sure], want["pos"][sure]) and np.array_equal(r["required_moved"].cpu().numpy()[sure], want["moved"][sure])
    assert torch.equal(_bits(r["row_plogp"]), _bits(base["row_plogp"]))
    pos = r["required_pos"].cpu().numpy()
    for b, j in zip(*np.nonzero(pos >= 0)):
        u = [int(v) for v in units[b, j] if v >= 0]
        assert seq[b, pos[b, j]:pos[b, j] + len(u)].tolist() == u
    assert not np.isin(seq, np.asarray(list(ban), np.int64)).any()
    return want


def test_bf16_engine_holds_the_rule_graph_fork_fill_feedback(bf16_full):
    cfg, eng, att, plain, top, before, _ = bf16_full
    lp, seq0, n = plain["seq_logprob"].cpu().numpy(), plain["seq"].cpu().numpy(), plain["phrase_length"].sum(1).cpu().numpy()
    units = units_of(lp, n, seq0)
    table = torch.from_numpy(units).cuda()
    kw = dict(row_stats=True, require_phrases=table)
    keys = ("seq", "row_plogp", "row_chosen", "seq_logprob", "required_pos", "required_moved") + LAYOUT
    r = _clone(eng.decode_naic(att, **kw))
    torch.cuda.synchronize()
    want = _holds_the_rule(r, plain, units)
    lens = (units >= 0).sum(2)
    print(f"required phrases bf16: {int((want['pos'] >= 0).sum())} of {int((lens > 0).sum())} units placed, {int(want['moved'].sum())} positions moved, "
          f"{int((want['margin'] == 0).sum())} images with an exact tie")
    assert int(want["moved"].sum()) > 0 and ((want["pos"] >= 0) & (lens >= 2)).sum() >= 16      # multi-word units were placed, and ids moved in
    as_lists = eng.decode_naic(att, row_stats=True, require_phrases=[[[int(v) for v in u if v >= 0] for u in row] for row in units])      # host lists give the same table
    torch.cuda.synchronize()
    assert _same_bits(as_lists, r, ("seq", "row_chosen", "required_moved", "seq_logprob"))
    # ban_ids + no_repeat: the placement follows the constrained pick, is handed its table and rule, and reads the emitted ids (the device table is classified there)
    q = eng.decode_naic(att, ban_ids=[top], no_repeat=True, **kw)
    torch.cuda.synchronize()
    _holds_the_rule(q, before["pick"], units, (top,), True)
    # one feed-back round: the last pass alone is placed on; the earlier pass was fed the unforced ids
    q = eng.decode_naic(att, refine_rounds=1, **kw)
    torch.cuda.synchronize()
    _holds_the_rule(q, before["T1"], units)
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
    # the filling pass alone on the decode's own layout
    ext, last = O.layout_of(cfg, plain)
    eng.encode(att)
    fr = eng.fill_naic(ext.to(torch.int32).cuda(), torch.from_numpy(last).to(torch.int32).cuda(), att.size(1), require_phrases=table)
    torch.cuda.synchronize()
    assert len(fr) == 3 and torch.equal(fr[0], r["seq"]) and torch.equal(_bits(fr[1]), _bits(r["seq_logprob"]))
    assert torch.equal(fr[2]["required_pos"], r["required_pos"]) and torch.equal(fr[2]["required_moved"], r["required_moved"])


def test_off_is_the_decode_as_it_was(bf16_full):
    """require_phrases None, [] and empty per-image lists add no keys and give the outputs of the decodes made before any required call on this engine, bit for bit."""
    cfg, eng, att, plain, top, before, _ = bf16_full
    keys = ("seq", "seq_logprob", "row_plogp", "row_chosen") + LAYOUT
    used = eng.decode_naic(att, row_stats=True, require_phrases=[[4242, 4243]])      # (a call with the option in between, and its dict reused below)
    assert "required_pos" in used and used["required_pos"].shape == (16, 1)
    for off in (None, [], [[]] * 16, [[[]]] * 16):
        r = eng.decode_naic(att, row_stats=True, require_phrases=off)
        torch.cuda.synchronize()
        assert _same_bits(r, plain, keys) and "required_pos" not in r and "required_moved" not in r and "constrained" not in r
    r = eng.decode_naic(att, row_stats=True, out=used)
    torch.cuda.synchronize()
    assert _same_bits(r, plain, keys) and "required_pos" not in r and "required_moved" not in r


def test_engine_refuses_what_required_phrases_exclude(bf16_full):
    from boficap_amd import hip
    from boficap_amd.engine import DecodePipeline
    cfg, eng, att, plain, top, before, _ = bf16_full
    a = att[:4].contiguous()
    ph = [[9, 10]]
    for kw, word in ((dict(ids_only=True), "ids_only"), (dict(refine_rounds=2, refine_method="mask_predict"), "mask_predict"), (dict(block_trigrams=True), "block_trigrams"),
                     (dict(nbest=3), "nbest"), (dict(ban_ids=[9]), "ban_ids"), (dict(require_ids=[11]), "give one")):
        with pytest.raises(hip.BofiHipError, match=word):
            eng.decode_naic(a, require_phrases=ph, **kw)
    for bad, word in (([[cfg.tgt_vocab, 9]], "0.."), ([[9, 10, 11, 12, 13]], "at most 4"), ([[i + 10, i + 30] for i in range(9)], "at most 8"),
                      (torch.zeros(4, 2, 5, dtype=torch.int32, device="cuda"), "L"), (torch.zeros(4, 9, 2, dtype=torch.int32, device="cuda"), "K")):
        with pytest.raises(hip.BofiHipError, match=word):
            eng.decode_naic(a, require_phrases=bad)
    with pytest.raises(hip.BofiHipError, match=r"\[9, 10\] and \[10, 11\] could meet"):
        eng.decode_naic(a, no_repeat=True, require_phrases=[[9, 10], [10, 11]])
    with pytest.raises(hip.BofiHipError, match="mask_predict"):
        eng.fill_naic(torch.zeros(4, cfg.bound_len, dtype=torch.int32, device="cuda"), torch.ones(4, dtype=torch.int32, device="cuda"), 36, refine_rounds=2,
                      refine_method="mask_predict", require_phrases=ph)
    for kw, word in ((dict(fused_vocab=True), "fused_vocab"), (dict(refine_rounds=2, refine_method="mask_predict"), "mask_predict"), (dict(block_trigrams=True), "block_trigrams")):
        with pytest.raises(hip.BofiHipError, match=word):
            DecodePipeline(eng, require_phrases=ph, **kw)
        with pytest.raises(hip.BofiHipError, match=word):
            DecodePipeline(eng, **kw).run([a], require_phrases=ph)      # (raised by the call, before the generator is advanced)
    with pytest.raises(hip.BofiHipError, match="give one"):
        DecodePipeline(eng).run([a], require_ids=[9], require_phrases=ph)
    torch.cuda.synchronize()
    assert torch.equal(eng.decode_naic(att)["seq"], plain["seq"])   # nothing was enqueued: the engine decodes as before
    # a device table goes through unchecked: the kernel classifies it (banned, out of range, a repeat of an earlier unit, could meet under no_repeat, empty)
    t = torch.tensor([[[top, 9], [cfg.tgt_vocab, 9], [20, 21], [20, 21], [21, 30], [-1, 5]]] * 16, dtype=torch.int32, device="cuda")
    r = eng.decode_naic(att, ban_ids=[top], no_repeat=True, require_phrases=t)
    torch.cuda.synchronize()
    pos, n = r["required_pos"].cpu(), r["phrase_length"].sum(1).cpu()
    print(f"device table: live counts {n.tolist()}, the kept unit's positions {pos[:, 2].tolist()}")
    assert pos[:, [0, 1, 3, 4, 5]].tolist() == [[-2, -2, -2, -2, -1]] * 16 and not (r["seq"] == top).any()
    assert torch.equal(pos[:, 2] >= 0, n >= 2) and (pos[:, 2][n < 2] == -3).all() and int((n >= 2).sum()) >= 8      # (two ids need two live positions)
    for b in range(16):
        if n[b] >= 2:
            assert r["seq"][b, int(pos[b, 2]):int(pos[b, 2]) + 2].tolist() == [20, 21]


# ----------------------------------------------------------------------------- 4. above the engine
def test_interface_gives_the_engine_level_result(weight_cache, monkeypatch):
    """decode_many with per-batch unit tables (grouped batches in one launch, a ragged tail, a batch without units) and mode='sample' with opt['require_phrases'] against
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
        tables = [[[[4242, 77], [901]]] * 8, None, [[[int(plain[2][k, 0]), 902, 903]] if k % 2 else [] for k in range(8)], [[901, 902], [903, 904, 905, 906]]]
        want = []
        for i, b in enumerate(batches):
            r = ref.decode_naic(b.cuda(), lens(i), row_stats=True, no_repeat=True, require_phrases=tables[i])
            want.append({k: v.cpu() for k, v in r.items() if torch.is_tensor(v)})
        items = [batches[0].pin_memory(), batches[1].pin_memory(), batches[2].pin_memory(), (batches[3].pin_memory(), tail_masks)]
        got = list(model.decode_many(items, batches_per_launch=3, in_flight=2, no_repeat=True, require_phrases=tables))
        assert len(got) == 4
        for i, (g, w) in enumerate(zip(got, want)):
            for k in ("seq", "constrained") + LAYOUT + (("required_pos", "required_moved") if tables[i] is not None else ()):
                assert torch.equal(g[k], w[k]), (i, k)
            assert ("required_pos" in g) == (tables[i] is not None)
        assert got[0]["required_pos"].shape == (8, 2) and got[2]["required_pos"].shape == (8, 1) and got[3]["required_pos"].shape == (5, 2)
        assert any(not torch.equal(g["seq"], p) for g, p in zip(got, plain)) and all(int((g["required_pos"] >= 0).sum()) > 0 for g in (got[0], got[2], got[3]))
        flat = list(model.decode_many(items, batches_per_launch=3, in_flight=2, require_phrases=[[901, 902], [77]]))      # one flat list of units: every image of every batch
        for i, (g, b) in enumerate(zip(flat, batches)):
            e = ref.decode_naic(b.cuda(), lens(i), require_phrases=[[901, 902], [77]])
            assert torch.equal(g["seq"], e["seq"].cpu()) and torch.equal(g["required_pos"], e["required_pos"].cpu())
        again = list(model.decode_many(items, batches_per_launch=3, in_flight=2))               # the defaults stay the plain decode
        assert all(torch.equal(g["seq"], p) and "required_pos" not in g for g, p in zip(again, plain))
        for kw, word in ((dict(fused_vocab=True), "fused_vocab"), (dict(block_trigrams=True), "block_trigrams"), (dict(refine_rounds=2, refine_method="mask_predict"), "mask_predict"),
                         (dict(require_ids=[901]), "give one")):
            with pytest.raises(H.BofiHipError, match=word):
                model.decode_many(items, require_phrases=[[901, 902]], **kw)
        with pytest.raises(H.BofiHipError, match="fewer"):
            list(model.decode_many(items, require_phrases=[[[[901, 902]]] * 8, None]))
        # mode='sample'
        fc = torch.zeros(5, 0, device="cuda")
        ph = [[901, 902, 903], [77]]
        out = model(fc, batches[3].cuda(), tail_masks.cuda(), opt={"train_mode": "NAIC", "require_phrases": ph}, mode="sample")
        assert len(out) == 6
        last = {k: v.clone() for k, v in model.last_required.items()}
        e = model.engine().decode_naic(batches[3].cuda(), lens(3), require_phrases=ph)
        torch.cuda.synchronize()
        assert torch.equal(out[0], e["seq"]) and torch.equal(last["pos"], e["required_pos"]) and torch.equal(last["moved"], e["required_moved"])
        assert int(last["moved"].sum()) > 0 and sorted(last) == ["moved", "pos"]
        model(fc, batches[3].cuda(), tail_masks.cuda(), opt={"train_mode": "NAIC", "require_phrases": []}, mode="sample")
        assert model.last_required is None
        for bad, word in (({"train_mode": "NAIC", "require_phrases": ph, "sample_method": "sample"}, "require_phrases"),
                          ({"train_mode": "NAIC", "require_phrases": ph, "refine_rounds": 2, "refine_method": "mask_predict"}, "require_phrases"),
                          ({"train_mode": "SAIC", "require_phrases": ph}, "require_phrases"), ({"train_mode": "NAIC", "require_phrases": ph, "require_ids": [5]}, "give one")):
            with pytest.raises(H.BofiHipError, match=word):
                model(fc, batches[3].cuda(), tail_masks.cuda(), opt=bad, mode="sample")
    finally:
        monkeypatch.undo()
        H.lib().bofi_reload_env()


def test_eval_split_places_required_phrases():
    from boficap_amd import eval_utils
    from boficap_amd.config import TINY
    from test_gpu_lang_eval import tiny_model
    labels = eval_utils.SyntheticLabels(TINY, 8, 5, seed=3)
    model = tiny_model()
    base = {"batch_size": 4, "language_eval": 1, "verbose_loss": 0}
    _, preds0, stats0 = eval_utils.eval_split(model, labels.feats, labels, dict(base))
    spec = {0: ["w30 w31", "w36"], "3": ["w32"], 6: "w33 w34 w35,w37 w38"}
    _, preds, stats = eval_utils.eval_split(model, labels.feats, labels, dict(base, require_words=spec))
    assert "required_rate" not in stats0 and list(stats)[:-2] == list(stats0) and list(stats)[-2:] == ["required_rate", "required_moved_rate"]
    host = torch.from_numpy(labels.feats)
    units = [[[30, 31], [36]], [], [], [[32]], [], [], [[33, 34, 35], [37, 38]], []]
    names = [["w30 w31", "w36"], [], [], ["w32"], [], [], ["w33 w34 w35", "w37 w38"], []]
    got = list(model.decode_many([host[i:i + 4] for i in range(0, 8, 4)], require_phrases=[units[:4], units[4:]]))
    pos = [row for g in got for row in g["required_pos"]]
    assert got[0]["required_pos"].shape == (4, 2) and got[1]["required_pos"].shape == (4, 2)
    placed = sum(int(pos[k][j] >= 0) for k in range(8) for j in range(len(units[k])))
    assert stats["required_rate"] == placed / 5 and placed > 0      # (the rate counts units)
    assert stats["required_moved_rate"] == sum(int(g["required_moved"].sum()) for g in got) / sum(int(g["phrase_length"].sum()) for g in got)
    assert preds != preds0 and "required" not in preds0[0]
    assert [p["required"] for p in preds] == [[[w, (int(pos[k][j]) if pos[k][j] >= 0 else None)] for j, w in enumerate(names[k])] for k in range(8)]
    for p, us in zip(preds, units):
        for (w, where), u in zip(p["required"], us):
            assert where is None or p["seq"][where:where + len(u)] == u
    with pytest.raises(ValueError, match="'w99'"):
        eval_utils.eval_split(model, labels.feats, labels, dict(base, require_words="w30 w99"))
    with pytest.raises(ValueError, match="NAIC"):
        eval_utils.eval_split(model, labels.feats, labels, dict(base, inference_mode="SAIC", require_words="w30 w31"))
