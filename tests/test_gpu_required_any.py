"""Required alternatives on the MI355X: bofi_vocab_require_any against the numpy restatement of tests/test_required_any.py (bit for bit) and, with one alternative per
group, against bofi_vocab_require_units; the float32 engine against the restated decode on the golden cases; the bf16 engine held without a tolerance to
``require_any_np`` on its OWN returned log-probs (graph replay, fork, filling pass alone, feed-back, grouped batches through decode_many); "off is the decode as it was";
the refusals; and the interface above the engine (mode='sample', eval_split)."""
import functools

import numpy as np
import pytest
import torch

import boficap_oracle as O
from test_constrained_pick import MARGIN, order_np, pick_np, plain_of
from test_gpu_constrained_pick import KEEP, LAYOUT, _bits, _clone, _same_bits
from test_gpu_required_phrases import _units_case
from test_gpu_required_words import bf16_full, f32_engines      # noqa: F401  (the fixtures: an engine per module)
from test_required_any import classify_any_np, group_codes, require_any_np

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------- 1. the kernel
def _any_case(rng, B, S, V, ldx, K, A, L):
    """The data of ``_units_case`` (tie-rich x with NaN and +-inf, poison past column V, ids outside the vocabulary in seq, ntok with a bias and clamped both ways) with
    each unit grown into A alternatives [B, K, A, L]: alternative 0 is the unit; the others come from the same small pool with a random length and garbage behind the
    first negative id; empties in the middle of a group; ids >= V; on every fourth image an alternative that duplicates one of ANOTHER group; on every fifth a group whose
    only kept alternative is the last (the others hold an id >= V or are empty); on every sixth the alternative that stands in seq (``_units_case``: every third image)
    is moved to the group's last slot."""
    x, seq, units, n, ntok, ban = _units_case(rng, B, S, V, ldx, K, L)
    pool = np.arange(4, min(V, 4 + max(6, S // 2)))
    alts = rng.choice(pool, (B, K, A, L)).astype(np.int32)
    alts[:, :, 0] = units
    for b in range(B):
        for k in range(K):
            for a in range(1, A):
                ln = int(rng.integers(1, L + 1))
                if ln < L:
                    alts[b, k, a, ln] = -1 - int(rng.integers(0, 3))
    alts[:, :, 1:, 0][rng.random((B, K, A - 1)) < 0.2] = -1     # empties, in the middle of a group too
    alts[:, :, 1:][rng.random((B, K, A - 1, L)) < 0.03] = V
    for b in range(1, B, 4):
        if K >= 2:
            alts[b, 1, A - 1] = alts[b, 0, 0]
    for b in range(2, B, 5):
        for a in range(A - 1):
            alts[b, K - 1, a, 0] = V if a % 2 == 0 else -1
        alts[b, K - 1, A - 1] = -1
        alts[b, K - 1, A - 1, 0] = pool[(b + 2) % len(pool)]
    for b in range(3, B, 6):
        alts[b, 0, [0, A - 1]] = alts[b, 0, [A - 1, 0]]
    if B < 3:                                                   # the two smallest shapes: image 0's LAST alternative gains 0.875 at position 1 and is moved in there
        alts[0, 0, A - 1] = -1
        alts[0, 0, A - 1, 0] = pool[5]
        seq[0, 1] = pool[4]
        x[0, 1, pool[4]], x[0, 1, pool[5]] = -1.0, -0.125
    return x, seq, alts, n, ntok, ban


ANY_CASES = [(1, 20, 64, 64, 1, 2, 1), (5, 20, 9491, 9491, 4, 3, 3), (3, 64, 9491, 9600, 8, 4, 4), (130, 20, 257, 257, 3, 2, 4), (2, 3, 64, 64, 2, 4, 4)]


def _any_wants(B, S, V, ldx, K, A, L):
    """The case's data and ``require_any_np`` on it for (ban, no_repeat) in four variants; the checks that the case is not vacuous."""
    rng = np.random.default_rng(9100 + 100 * B + S + V + K + 7 * A + L)
    x, old, alts, n, ntok, ban = _any_case(rng, B, S, V, ldx, K, A, L)
    keep = np.full((B, S), KEEP, np.float32)
    wants = {(use_ban, rep): require_any_np(x[:, :, :V], n, alts, old, ban if use_ban else (), rep, 7, chosen=keep) for use_ban in (False, True) for rep in (False, True)}
    w = wants[(False, False)]
    kinds = [k for b in range(B) for k in classify_any_np(alts[b], V, ())]
    codes = np.array([group_codes(classify_any_np(alts[b], V, ()), K, A) for b in range(B)])
    only_last = sum(1 for b in range(B) for j in range(K) if [isinstance(k, list) for k in classify_any_np(alts[b], V, ())[j * A:(j + 1) * A]] == [False] * (A - 1) + [True])
    print(f"required alternatives kernel {(B, S, V, ldx, K, A, L)}: {int((w['pos'] >= 0).sum())} groups placed, by alternative {np.bincount(w['which'][w['which'] >= 0], minlength=A).tolist()}, "
          f"{int((w['pos'] == -3).sum())} unplaceable, {int((codes == -2).sum())} skipped groups, {kinds.count(-2)} skipped and {kinds.count(-1)} empty slots, "
          f"{only_last} groups whose only kept alternative is the last, {int(w['moved'].sum())} moved, {int((w['margin'] == 0).sum())} of {B} images with an exact tie; "
          f"{int((wants[(False, True)]['seq'] != w['seq']).sum())} positions differ under no_repeat, {int((wants[(True, False)]['seq'] != w['seq']).sum())} under the ban")
    any_w = list(wants.values())
    # not vacuous: something was placed, something moved, a group was placed by an alternative with a > 0 (for the two smallest shapes: in one of the variants)
    assert int((w["pos"] >= 0).sum()) > 0 and int(w["moved"].sum()) > 0
    assert (w["which"] > 0).any() if B >= 3 else any((v["which"] > 0).any() for v in any_w)
    assert sum(int((v["pos"] <= -2).sum()) for v in any_w) > 0
    assert (wants[(True, False)]["which"] != w["which"]).any() or (wants[(True, False)]["pos"] != w["pos"]).any()      # the ban table changes the placement
    if B >= 5:
        assert (w["pos"] == -3).any() and (codes == -2).any() and kinds.count(-2) and kinds.count(-1) and only_last
        assert any(kinds[i] == -1 and isinstance(kinds[i + 1], list) for i in range(len(kinds) - 1) if (i + 1) % A)      # an empty slot in front of a kept one of its group
    return x, old, alts, n, ntok, ban, wants


@pytest.mark.parametrize("B,S,V,ldx,K,A,L", ANY_CASES)
def test_kernel_equals_require_any_np(B, S, V, ldx, K, A, L):
    """seq, row_chosen (the untouched entries included), pos, which and moved bit for bit: with and without a ban table, no_repeat, ntok, row_chosen and moved; ntok read
    with a bias and clamped; for the small-B shapes the tensor 0..3 floats off a 16-byte boundary; x is read only.  (3, 64, 9491, 9600, 8, 4, 4) is the LDS ceiling
    (one image per workgroup, a mask per lane), (130, ...) has the partial last workgroup, (2, 3, ...) units longer than S."""
    from boficap_amd import hip
    x, old, alts, n, ntok, ban, wants = _any_wants(B, S, V, ldx, K, A, L)
    d_ntok, d_ban, d_alts = torch.from_numpy(ntok).cuda(), hip.ban_bits(ban, V, "cuda"), torch.from_numpy(alts).cuda()
    for off in ((0, 1, 2, 3) if B <= 5 else (0,)):
        buf = torch.full((B * S * ldx + 8,), 7.0, dtype=torch.float32, device="cuda")
        dx = buf[off:off + B * S * ldx].view(B * S, ldx)
        dx.copy_(torch.from_numpy(x.reshape(B * S, ldx)))
        for (use_ban, rep), want in wants.items():
            what = (B, S, V, ldx, K, A, L, off, use_ban, rep)
            seq = torch.from_numpy(old.copy()).cuda().view(-1)
            chosen = torch.full((B * S,), KEEP, dtype=torch.float32, device="cuda")
            pos = torch.full((B, K), -9, dtype=torch.int32, device="cuda")
            which = torch.full((B, K), -9, dtype=torch.int32, device="cuda")
            moved = torch.full((B,), -9, dtype=torch.int32, device="cuda")
            hip.vocab_require_any(dx, V, S, seq, d_alts, pos, which, ntok=d_ntok, ntok_bias=-1, ban=d_ban if use_ban else None, no_repeat=rep, repeat_min_id=7,
                                  row_chosen=chosen, moved=moved)
            torch.cuda.synchronize()
            assert np.array_equal(seq.cpu().numpy().reshape(B, S), want["seq"]), what
            assert np.array_equal(chosen.cpu().numpy().reshape(B, S).view(np.int32), want["chosen"].view(np.int32)), what
            assert np.array_equal(pos.cpu().numpy(), want["pos"]), what
            assert np.array_equal(which.cpu().numpy(), want["which"]), what
            assert np.array_equal(moved.cpu().numpy(), want["moved"]), what
        assert np.array_equal(dx.cpu().numpy().view(np.int32), x.reshape(B * S, ldx).view(np.int32))      # (x is read only)
    # optional outputs and ntok left out; another floor for the adjacency rule
    seq = torch.from_numpy(old.copy()).cuda().view(-1)
    pos = torch.full((B, K), -9, dtype=torch.int32, device="cuda")
    which = torch.full((B, K), -9, dtype=torch.int32, device="cuda")
    hip.vocab_require_any(dx, V, S, seq, d_alts, pos, which, no_repeat=True, repeat_min_id=0)
    torch.cuda.synchronize()
    full = require_any_np(x[:, :, :V], np.full(B, S), alts, old, (), True, 0)
    assert np.array_equal(seq.cpu().numpy().reshape(B, S), full["seq"]) and np.array_equal(pos.cpu().numpy(), full["pos"]) and np.array_equal(which.cpu().numpy(), full["which"])


@pytest.mark.parametrize("B,S,V,ldx,K", [(5, 20, 9491, 9491, 4), (3, 64, 9491, 9600, 8), (130, 20, 257, 257, 3)])
def test_one_alternative_per_group_equals_the_units_kernel(B, S, V, ldx, K):
    """bofi_vocab_require_any on [B, K, 1, L] -- and on [B, K, 3, L] with -1 slots behind -- equals bofi_vocab_require_units on the same inputs, bit for bit: seq,
    row_chosen, pos, moved, and which = 0 exactly where a unit was placed; with and without the ban table and no_repeat."""
    from boficap_amd import hip
    L = 4 if K != 4 else 3
    rng = np.random.default_rng(7100 + 100 * B + S + V + K)
    x, old, units, n, ntok, ban = _units_case(rng, B, S, V, ldx, K, L)
    dx, d_ntok, d_ban, d_units = torch.from_numpy(x.reshape(B * S, ldx)).cuda(), torch.from_numpy(ntok).cuda(), hip.ban_bits(ban, V, "cuda"), torch.from_numpy(units).cuda()
    wide = torch.full((B, K, 3, L), -1, dtype=torch.int32, device="cuda")
    wide[:, :, 0] = d_units
    wide[:, :, 2, 1:] = 9                                       # (behind a slot's first negative id: not read)
    placed = 0
    for use_ban in (False, True):
        for rep in (False, True):
            got = []
            for table in (d_units, d_units.view(B, K, 1, L).contiguous(), wide):
                seq = torch.from_numpy(old.copy()).cuda().view(-1)
                chosen = torch.full((B * S,), KEEP, dtype=torch.float32, device="cuda")
                pos = torch.full((B, K), -9, dtype=torch.int32, device="cuda")
                which = torch.full((B, K), -9, dtype=torch.int32, device="cuda")
                moved = torch.full((B,), -9, dtype=torch.int32, device="cuda")
                kw = dict(ntok=d_ntok, ntok_bias=-1, ban=d_ban if use_ban else None, no_repeat=rep, repeat_min_id=7, row_chosen=chosen, moved=moved)
                if table.dim() == 3:
                    hip.vocab_require_units(dx, V, S, seq, table, pos, **kw)
                else:
                    hip.vocab_require_any(dx, V, S, seq, table, pos, which, **kw)
                torch.cuda.synchronize()
                got.append((seq.cpu(), chosen.cpu().view(torch.int32), pos.cpu(), moved.cpu()))
                if table.dim() == 4:
                    assert torch.equal(which.cpu(), torch.where(got[0][2] >= 0, 0, -1).to(torch.int32)), (use_ban, rep)
            for other in got[1:]:
                assert all(torch.equal(a, b) for a, b in zip(got[0], other)), (use_ban, rep)
            placed += int((got[0][2] >= 0).sum())
    assert placed > 0


# ----------------------------------------------------------------------------- 2. the float32 engine against the restated decode
def alts_of(lp, n, seq):
    """The table rule of the engine tests, per image, from a plain decode's log-probs lp [B, S, V], live counts and ids -- int32 [B, 3, 3, 3].
    Group 0: the runner-up ids of the two middle live positions side by side; then the third-best ids there; then the bigram (V - 40 - 3b, V - 41 - 3b).
    Group 1: (V - 1 - 3b, V - 2 - 3b, V - 3 - 3b); then (V - 80 - 3b, V - 81 - 3b).
    Group 2: the fourth-best ids of positions 0 and 1; then a bigram the caption emits exactly once (it stands: gain 0)."""
    B, _, V = lp.shape
    t = np.full((B, 3, 3, 3), -1, np.int32)
    for b in range(B):
        nb = int(n[b])
        if nb >= 2:
            for a, k in ((0, 1), (1, 2)):
                t[b, 0, a, :2] = [int(order_np(lp[b, nb // 2 - 1])[k]), int(order_np(lp[b, nb // 2])[k])]
            t[b, 2, 0, :2] = [int(order_np(lp[b, 0])[3]), int(order_np(lp[b, 1])[3])]
        t[b, 0, 2, :2] = [V - 40 - 3 * b, V - 41 - 3 * b]
        t[b, 1, 0] = [V - 1 - 3 * b, V - 2 - 3 * b, V - 3 - 3 * b]
        t[b, 1, 1, :2] = [V - 80 - 3 * b, V - 81 - 3 * b]
        live = [int(v) for v in seq[b, :nb]]
        grams = [(live[p], live[p + 1]) for p in range(nb - 1)]
        once = [g for g in grams if min(g) >= 7 and g[0] != g[1] and grams.count(g) == 1]
        if once:
            t[b, 2, 1, :2] = once[len(once) // 2]
    return t


@functools.lru_cache(maxsize=None)
def restated(name):
    """The decode of golden case ``name`` with the table of ``alts_of``: require_any_np on the oracle's own log-probs and plain ids; ``safe`` [B]: the placement's margin
    AND every plain pick's margin exceed MARGIN."""
    base = plain_of(name)
    alts = alts_of(base["lp"], base["n"], base["seq"])
    r = require_any_np(base["lp"], base["n"], alts, base["seq"])
    r["alts"], r["safe"] = alts, (r["margin"] > MARGIN) & (pick_np(base["lp"], base["n"], pad=base["cfg"].pad_idx)["margin"] > MARGIN)
    return r


@pytest.mark.parametrize("name", ["tiny_saic_multi", "full_b8"])
def test_f32_engine_equals_the_restated_decode(name, f32_engines):
    """seq, pos, alt and moved on the images whose restated margin, and whose every plain pick's margin, exceed MARGIN = 1e-3; at most a quarter of the images may be
    left out.  (On the oracle's own log-probs the rule leaves out 0 of 6 images of tiny_saic_multi -- smallest margin 0.0017 -- and 1 of 8 of full_b8, which has one
    exact tie; the placements use alternative 0 in some groups and alternative 1 in others.)"""
    base, ref = plain_of(name), restated(name)
    eng = f32_engines(name)
    att = base["att"].cuda()
    att_len = None if base["masks"] is None else base["masks"].sum(1).to(torch.int32).cuda()
    r = eng.decode_naic(att, att_len, row_stats=True, require_any=torch.from_numpy(ref["alts"]).cuda())
    torch.cuda.synchronize()
    for k in LAYOUT:
        assert torch.equal(r[k].cpu(), base[k]), k
    safe = ref["safe"]
    print(f"required alternatives {name}: margins {np.round(ref['margin'], 5).tolist()}, safe {int(safe.sum())} of {len(safe)}, placed {int((ref['pos'] >= 0).sum())} by "
          f"alternative {np.bincount(ref['which'][ref['which'] >= 0], minlength=3).tolist()}, moved {int(ref['moved'].sum())}")
    assert 4 * int((~safe).sum()) <= len(safe)
    assert np.array_equal(r["seq"].cpu().numpy()[safe], ref["seq"][safe])
    assert np.array_equal(r["required_pos"].cpu().numpy()[safe], ref["pos"][safe])
    assert np.array_equal(r["required_alt"].cpu().numpy()[safe], ref["which"][safe])
    assert np.array_equal(r["required_moved"].cpu().numpy()[safe], ref["moved"][safe])
    assert int(ref["moved"][safe].sum()) > 0 and (ref["pos"][safe] >= 0).sum() >= safe.sum()
    assert (ref["which"][safe] == 0).any() and (ref["which"][safe] >= 1).any()


# ----------------------------------------------------------------------------- 3. the bf16 engine, without a tolerance
def _holds_the_rule(r, base, alts, ban=(), rep=False, min_id=7):
    """``r`` (a decode with require_any) against ``base`` (the same decode without): the log-probs are bit-equal; pos, alt, moved and -- on the images whose margin is
    not an exact 0, at least three quarters -- seq and row_chosen equal require_any_np on those log-probs and base's ids, bit for bit.  Every placed alternative stands
    at its pos."""
    lp = r["seq_logprob"].cpu().numpy()
    assert torch.equal(_bits(r["seq_logprob"]), _bits(base["seq_logprob"])) and _same_bits(r, base, LAYOUT)
    n = r["phrase_length"].sum(1).cpu().numpy()
    want = require_any_np(lp, n, alts, base["seq"].cpu().numpy(), ban, rep, min_id, chosen=base["row_chosen"].cpu().numpy())
    sure = want["margin"] != 0.0
    assert 4 * int((~sure).sum()) <= len(sure), want["margin"]
    seq = r["seq"].cpu().numpy()
    assert np.array_equal(seq[sure], want["seq"][sure])
    assert np.array_equal(r["row_chosen"].cpu().numpy().view(np.int32)[sure], want["chosen"].view(np.int32)[sure])
    assert np.array_equal(r["required_pos"].cpu().numpy()[sure], want["pos"][sure]) and np.array_equal(r["required_moved"].cpu().numpy()[sure], want["moved"][sure])
    assert np.array_equal(r["required_alt"].cpu().numpy()[sure], want["which"][sure])
    assert torch.equal(_bits(r["row_plogp"]), _bits(base["row_plogp"]))
    pos, alt = r["required_pos"].cpu().numpy(), r["required_alt"].cpu().numpy()
    assert ((pos >= 0) == (alt >= 0)).all()
    for b, j in zip(*np.nonzero(pos >= 0)):
        u = [int(v) for v in alts[b, j, alt[b, j]] if v >= 0]
        assert seq[b, pos[b, j]:pos[b, j] + len(u)].tolist() == u
    assert not np.isin(seq, np.asarray(list(ban), np.int64)).any()
    return want


def _as_lists(alts):
    return [[[[int(v) for v in u if v >= 0] for u in g] for g in row] for row in alts]


def test_bf16_engine_holds_the_rule_graph_fork_fill_feedback(bf16_full):
    cfg, eng, att, plain, top, before, _ = bf16_full
    lp, seq0, n = plain["seq_logprob"].cpu().numpy(), plain["seq"].cpu().numpy(), plain["phrase_length"].sum(1).cpu().numpy()
    alts = alts_of(lp, n, seq0)
    table = torch.from_numpy(alts).cuda()
    kw = dict(row_stats=True, require_any=table)
    keys = ("seq", "row_plogp", "row_chosen", "seq_logprob", "required_pos", "required_alt", "required_moved") + LAYOUT
    r = _clone(eng.decode_naic(att, **kw))
    torch.cuda.synchronize()
    want = _holds_the_rule(r, plain, alts)
    print(f"required alternatives bf16: {int((want['pos'] >= 0).sum())} of {want['pos'].size} groups placed, by alternative "
          f"{np.bincount(want['which'][want['which'] >= 0], minlength=3).tolist()}, {int(want['moved'].sum())} positions moved, {int((want['margin'] == 0).sum())} images with an exact tie")
    assert int(want["moved"].sum()) > 0 and (want["which"] == 0).any() and (want["which"] >= 1).any()
    as_lists = eng.decode_naic(att, row_stats=True, require_any=_as_lists(alts))      # host lists give the same table
    torch.cuda.synchronize()
    assert _same_bits(as_lists, r, ("seq", "row_chosen", "required_pos", "required_alt", "required_moved", "seq_logprob"))
    # ban_ids + no_repeat: the placement follows the constrained pick, is handed its table and rule, and reads the emitted ids (the device table is classified there)
    q = eng.decode_naic(att, ban_ids=[top], no_repeat=True, **kw)
    torch.cuda.synchronize()
    _holds_the_rule(q, before["pick"], alts, (top,), True)
    # one feed-back round: the last pass alone is placed on; the earlier pass was fed the unforced ids
    q = eng.decode_naic(att, refine_rounds=1, **kw)
    torch.cuda.synchronize()
    _holds_the_rule(q, before["T1"], alts)
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
    fr = eng.fill_naic(ext.to(torch.int32).cuda(), torch.from_numpy(last).to(torch.int32).cuda(), att.size(1), require_any=table)
    torch.cuda.synchronize()
    assert len(fr) == 3 and torch.equal(fr[0], r["seq"]) and torch.equal(_bits(fr[1]), _bits(r["seq_logprob"]))
    assert all(torch.equal(fr[2][k], r[k]) for k in ("required_pos", "required_alt", "required_moved"))


def test_off_is_the_decode_as_it_was(bf16_full):
    """require_any None, [] and empty per-image lists add no keys and give the outputs of the decodes made before any required call on this engine, bit for bit; so does
    a call without the option that reuses the dict of one that had it."""
    cfg, eng, att, plain, top, before, _ = bf16_full
    keys = ("seq", "seq_logprob", "row_plogp", "row_chosen") + LAYOUT
    new = ("required_pos", "required_alt", "required_moved", "constrained")
    used = eng.decode_naic(att, row_stats=True, require_any=[[[4242, 4243], [4244]]])      # (a call with the option in between, and its dict reused below)
    assert used["required_pos"].shape == (16, 1) and used["required_alt"].shape == (16, 1)
    for off in (None, [], [[]] * 16, [[[]]] * 16, [[[[]]]] * 16):
        r = eng.decode_naic(att, row_stats=True, require_any=off)
        torch.cuda.synchronize()
        assert _same_bits(r, plain, keys) and not any(k in r for k in new)
    r = eng.decode_naic(att, row_stats=True, out=used)
    torch.cuda.synchronize()
    assert _same_bits(r, plain, keys) and not any(k in r for k in new)
    used = eng.decode_naic(att, row_stats=True, require_any=[[[4242, 4243], [4244]]])
    r = eng.decode_naic(att, row_stats=True, out=used, require_phrases=[[4242, 4243]])      # the other options keep their keys alone
    torch.cuda.synchronize()
    assert "required_pos" in r and "required_alt" not in r


def test_engine_refuses_what_required_alternatives_exclude(bf16_full):
    from boficap_amd import hip
    from boficap_amd.engine import DecodePipeline
    cfg, eng, att, plain, top, before, _ = bf16_full
    a = att[:4].contiguous()
    ph = [[[9, 10], [11]]]
    for kw, word in ((dict(ids_only=True), "ids_only"), (dict(refine_rounds=2, refine_method="mask_predict"), "mask_predict"), (dict(block_trigrams=True), "block_trigrams"),
                     (dict(nbest=3), "nbest"), (dict(ban_ids=[9]), "ban_ids"), (dict(require_ids=[11]), "give one"), (dict(require_phrases=[[12, 13]]), "give one")):
        with pytest.raises(hip.BofiHipError, match=word):
            eng.decode_naic(a, require_any=ph, **kw)
    for bad, word in (([[[cfg.tgt_vocab, 9]]], "0.."), ([[[9, 10, 11, 12, 13]]], "at most 4 ids"), ([[[i + 10, i + 30]] for i in range(9)], "at most 8"),
                      ([[[i + 10] for i in range(5)]], "at most 4 alternatives"), ([[[9], [9]]], "given twice"), ([[9, 10]], "bare id 9"),
                      (torch.zeros(4, 2, 2, 5, dtype=torch.int32, device="cuda"), "L"), (torch.zeros(4, 9, 2, 2, dtype=torch.int32, device="cuda"), "K"),
                      (torch.zeros(4, 2, 5, 2, dtype=torch.int32, device="cuda"), "A"), (torch.zeros(4, 2, 2, dtype=torch.int32, device="cuda"), r"\[B, K, A, L\]")):
        with pytest.raises(hip.BofiHipError, match=word):
            eng.decode_naic(a, require_any=bad)
    with pytest.raises(hip.BofiHipError, match=r"\[9, 10\] and \[10, 11\] of different groups could meet"):
        eng.decode_naic(a, no_repeat=True, require_any=[[[9, 10]], [[10, 11]]])
    with pytest.raises(hip.BofiHipError, match="mask_predict"):
        eng.fill_naic(torch.zeros(4, cfg.bound_len, dtype=torch.int32, device="cuda"), torch.ones(4, dtype=torch.int32, device="cuda"), 36, refine_rounds=2,
                      refine_method="mask_predict", require_any=ph)
    for kw, word in ((dict(fused_vocab=True), "fused_vocab"), (dict(refine_rounds=2, refine_method="mask_predict"), "mask_predict"), (dict(block_trigrams=True), "block_trigrams")):
        with pytest.raises(hip.BofiHipError, match=word):
            DecodePipeline(eng, require_any=ph, **kw)
        with pytest.raises(hip.BofiHipError, match=word):
            DecodePipeline(eng, **kw).run([a], require_any=ph)      # (raised by the call, before the generator is advanced)
    with pytest.raises(hip.BofiHipError, match="give one"):
        DecodePipeline(eng).run([a], require_ids=[9], require_any=ph)
    with pytest.raises(hip.BofiHipError, match="give one"):
        DecodePipeline(eng, require_phrases=[[9, 10]], require_any=ph)
    torch.cuda.synchronize()
    assert torch.equal(eng.decode_naic(att)["seq"], plain["seq"])   # nothing was enqueued: the engine decodes as before
    # a device table goes through unchecked: the kernel classifies it (banned, out of range, a repeat of an earlier slot, could meet under no_repeat, empty)
    t = torch.tensor([[[[top, 9], [cfg.tgt_vocab, 9]], [[20, 21], [21, 20]], [[20, 21], [-1, 5]], [[21, 30], [-1, -1]], [[-1, 5], [-1, -1]]]] * 16, dtype=torch.int32, device="cuda")
    r = eng.decode_naic(att, ban_ids=[top], no_repeat=True, require_any=t)
    torch.cuda.synchronize()
    pos, alt, n = r["required_pos"].cpu(), r["required_alt"].cpu(), r["phrase_length"].sum(1).cpu()
    print(f"device table: live counts {n.tolist()}, the kept group's positions {pos[:, 1].tolist()} by alternative {alt[:, 1].tolist()}")
    assert pos[:, [0, 2, 3, 4]].tolist() == [[-2, -2, -2, -1]] * 16 and alt[:, [0, 2, 3, 4]].tolist() == [[-1] * 4] * 16 and not (r["seq"] == top).any()
    assert torch.equal(pos[:, 1] >= 0, n >= 2) and (pos[:, 1][n < 2] == -3).all() and int((n >= 2).sum()) >= 8      # (two ids need two live positions)
    for b in range(16):
        if n[b] >= 2:
            assert r["seq"][b, int(pos[b, 1]):int(pos[b, 1]) + 2].tolist() == [[20, 21], [21, 20]][int(alt[b, 1])]


# ----------------------------------------------------------------------------- 4. above the engine
def test_interface_gives_the_engine_level_result(weight_cache, monkeypatch):
    """decode_many with per-batch tables (grouped batches in one launch, a ragged tail, a batch without a table) and with one flat list, and mode='sample' with
    opt['require_any'], against BofiEngine.decode_naic on the same batches, same kernel family and hint."""
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
        tables = [[[[[4242, 77], [4243]], [[901], [902], [903]]]] * 8, None, [[[[int(plain[2][k, 0]), 902, 903], [904]]] if k % 2 else [] for k in range(8)],
                  [[[901, 902], [905]], [[903, 904, 905, 906]]]]
        want = []
        for i, b in enumerate(batches):
            r = ref.decode_naic(b.cuda(), lens(i), row_stats=True, no_repeat=True, require_any=tables[i])
            want.append({k: v.cpu() for k, v in r.items() if torch.is_tensor(v)})
        items = [batches[0].pin_memory(), batches[1].pin_memory(), batches[2].pin_memory(), (batches[3].pin_memory(), tail_masks)]
        got = list(model.decode_many(items, batches_per_launch=3, in_flight=2, no_repeat=True, require_any=tables))
        assert len(got) == 4
        new = ("required_pos", "required_alt", "required_moved")
        for i, (g, w) in enumerate(zip(got, want)):
            for k in ("seq", "constrained") + LAYOUT + (new if tables[i] is not None else ()):
                assert torch.equal(g[k], w[k]), (i, k)
            assert all((k in g) == (tables[i] is not None) for k in new)
        assert got[0]["required_pos"].shape == got[0]["required_alt"].shape == (8, 2) and got[2]["required_alt"].shape == (8, 1) and got[3]["required_alt"].shape == (5, 2)
        assert any(not torch.equal(g["seq"], p) for g, p in zip(got, plain)) and all(int((g["required_pos"] >= 0).sum()) > 0 for g in (got[0], got[2], got[3]))
        one = [[[901, 902], [77]], [[905]]]
        flat = list(model.decode_many(items, batches_per_launch=3, in_flight=2, require_any=one))      # one flat list of groups: every image of every batch
        for i, (g, b) in enumerate(zip(flat, batches)):
            e = ref.decode_naic(b.cuda(), lens(i), require_any=one)
            assert torch.equal(g["seq"], e["seq"].cpu()) and torch.equal(g["required_pos"], e["required_pos"].cpu()) and torch.equal(g["required_alt"], e["required_alt"].cpu())
        again = list(model.decode_many(items, batches_per_launch=3, in_flight=2))               # the defaults stay the plain decode
        assert all(torch.equal(g["seq"], p) and not any(k in g for k in new) for g, p in zip(again, plain))
        for kw, word in ((dict(fused_vocab=True), "fused_vocab"), (dict(block_trigrams=True), "block_trigrams"), (dict(refine_rounds=2, refine_method="mask_predict"), "mask_predict"),
                         (dict(require_ids=[901]), "give one"), (dict(require_phrases=[[901]]), "give one")):
            with pytest.raises(H.BofiHipError, match=word):
                model.decode_many(items, require_any=one, **kw)
        with pytest.raises(H.BofiHipError, match="fewer"):
            list(model.decode_many(items, require_any=[[[[[901, 902]]]] * 8, None]))
        # mode='sample'
        fc = torch.zeros(5, 0, device="cuda")
        ph = [[[901, 902, 903], [904]], [[77]]]
        out = model(fc, batches[3].cuda(), tail_masks.cuda(), opt={"train_mode": "NAIC", "require_any": ph}, mode="sample")
        assert len(out) == 6
        last = {k: v.clone() for k, v in model.last_required.items()}
        e = model.engine().decode_naic(batches[3].cuda(), lens(3), require_any=ph)
        torch.cuda.synchronize()
        assert torch.equal(out[0], e["seq"]) and all(torch.equal(last[k], e["required_" + k]) for k in ("pos", "alt", "moved"))
        assert int(last["moved"].sum()) > 0 and sorted(last) == ["alt", "moved", "pos"]
        model(fc, batches[3].cuda(), tail_masks.cuda(), opt={"train_mode": "NAIC", "require_phrases": [[901, 902]]}, mode="sample")
        assert sorted(model.last_required) == ["moved", "pos"]     # the other options' record is unchanged
        model(fc, batches[3].cuda(), tail_masks.cuda(), opt={"train_mode": "NAIC", "require_any": []}, mode="sample")
        assert model.last_required is None
        for bad, word in (({"train_mode": "NAIC", "require_any": ph, "sample_method": "sample"}, "require_any"),
                          ({"train_mode": "NAIC", "require_any": ph, "refine_rounds": 2, "refine_method": "mask_predict"}, "require_any"),
                          ({"train_mode": "SAIC", "require_any": ph}, "require_any"), ({"train_mode": "NAIC", "require_any": ph, "require_ids": [5]}, "give one"),
                          ({"train_mode": "NAIC", "require_any": ph, "require_phrases": [[5, 6]]}, "give one")):
            with pytest.raises(H.BofiHipError, match=word):
                model(fc, batches[3].cuda(), tail_masks.cuda(), opt=bad, mode="sample")
    finally:
        monkeypatch.undo()
        H.lib().bofi_reload_env()


def test_eval_split_places_required_alternatives():
    from boficap_amd import eval_utils
    from boficap_amd.config import TINY
    from test_gpu_lang_eval import tiny_model
    labels = eval_utils.SyntheticLabels(TINY, 8, 5, seed=3)
    model = tiny_model()
    base = {"batch_size": 4, "language_eval": 1, "verbose_loss": 0}
    _, preds0, stats0 = eval_utils.eval_split(model, labels.feats, labels, dict(base))
    spec = {0: ["w30 w31|w39", "w36"], "3": ["w32|w40|w41"], 6: "w33 w34 w35|w42 w43,w37 w38"}      # plain words, phrases and '|' items
    _, preds, stats = eval_utils.eval_split(model, labels.feats, labels, dict(base, require_words=spec))
    assert "required_rate" not in stats0 and list(stats)[:-2] == list(stats0) and list(stats)[-2:] == ["required_rate", "required_moved_rate"]
    host = torch.from_numpy(labels.feats)
    groups = [[[[30, 31], [39]], [[36]]], [], [], [[[32], [40], [41]]], [], [], [[[33, 34, 35], [42, 43]], [[37, 38]]], []]
    names = [["w30 w31|w39", "w36"], [], [], ["w32|w40|w41"], [], [], ["w33 w34 w35|w42 w43", "w37 w38"], []]
    texts = [[n.split("|") for n in row] for row in names]
    got = list(model.decode_many([host[i:i + 4] for i in range(0, 8, 4)], require_any=[groups[:4], groups[4:]]))
    pos, alt = [row for g in got for row in g["required_pos"]], [row for g in got for row in g["required_alt"]]
    assert got[0]["required_pos"].shape == (4, 2) and got[1]["required_alt"].shape == (4, 2)
    placed = sum(int(pos[k][j] >= 0) for k in range(8) for j in range(len(groups[k])))
    assert stats["required_rate"] == placed / 5 and placed > 0      # (the rate counts groups)
    assert stats["required_moved_rate"] == sum(int(g["required_moved"].sum()) for g in got) / sum(int(g["phrase_length"].sum()) for g in got)
    assert preds != preds0 and "required" not in preds0[0]
    assert [p["required"] for p in preds] == [[[w, (int(pos[k][j]) if pos[k][j] >= 0 else None), (texts[k][j][int(alt[k][j])] if pos[k][j] >= 0 else None)]
                                               for j, w in enumerate(names[k])] for k in range(8)]
    for p, gs in zip(preds, groups):
        for (w, where, text), g in zip(p["required"], gs):
            if where is not None:
                u = g[w.split("|").index(text)]
                assert p["seq"][where:where + len(u)] == u
    # a spec without '|' gives the output it gave: two-field entries through require_phrases
    _, preds2, _ = eval_utils.eval_split(model, labels.feats, labels, dict(base, require_words={0: ["w30 w31", "w36"]}))
    e = list(model.decode_many([host[:4], host[4:]], require_phrases=[[[[30, 31], [36]], [], [], []], None]))[0]
    assert preds2[0]["required"] == [[w, (int(p) if p >= 0 else None)] for w, p in zip(["w30 w31", "w36"], e["required_pos"][0].tolist())] and preds2[1]["required"] == []
    with pytest.raises(ValueError, match="'w99'"):
        eval_utils.eval_split(model, labels.feats, labels, dict(base, require_words="w30|w99"))
    with pytest.raises(ValueError, match="NAIC"):
        eval_utils.eval_split(model, labels.feats, labels, dict(base, inference_mode="SAIC", require_words="w30|w31"))
