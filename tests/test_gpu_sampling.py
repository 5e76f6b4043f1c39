"""The device's sampled ids against the exact host restatement of the counter streams (tests/counter_streams.py): every id the
Gumbel-max sampler draws -- through bofi_vocab_sample, BofiEngine.sample_tokens and the engine's sampled SAIC loop -- must be
the restatement's, up to a derived float32 near-tie tolerance; and the two small kernels beside it (bofi_vocab_stats,
bofi_rl_take_draws) against plain torch."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import counter_streams as cs
from conftest import load_golden

pytestmark = pytest.mark.gpu

B, S = 3, 5
ROWS = B * S
VS = [1, 255, 256, 257, 9491]                      # the sampler's sweep is 256 wide; 9491 is the product's vocabulary
NS = [1, 7]
TS = [1.0, 0.7, 1e-3]
SEEDS = [0, 987654321, 2 ** 63 + 12345, 2 ** 64 - 1]
NTOK = [5, 2, 0]
NAN_AT, INF_ROW = (1, 0), 4                        # (row, column) of the NaN; the row that is -inf throughout
EDGE_AT = ((0, -1), (3, 256), (5, 255), (10, 0))   # (row, column; -1: the last) of the rows whose mass sits on an edge of the sweep
TIE_CAP = 0.005                                   # share of draws with more than one candidate, from the restatement alone
BOFI_OK, BOFI_ERR_ARG = 0, 1


@functools.lru_cache(maxsize=None)
def _lp(V):
    """float32 [ROWS, V] log-probs with a NaN, a few -inf entries and one all -inf row, all on rows that ntok keeps.  Four rows carry
    their largest logit (the row's maximum + 2) on an edge of the 256-wide sweep -- the last element, 256, 255, 0 -- so that an element
    the sweep leaves out is drawn often at T >= 0.7 and always at T = 1e-3."""
    g = torch.Generator().manual_seed(1000 + V)
    x = 3 * torch.randn(ROWS, V, generator=g)
    for r, c in EDGE_AT:
        x[r, min(c, V - 1) if c >= 0 else V - 1] = float(x[r].max()) + 2
    lp = torch.log_softmax(x, -1)
    lp[NAN_AT] = float("nan")
    lp[INF_ROW] = float("-inf")
    if V > 1:
        for r, c in ((2, 3), (2, V - 1), (5, V // 2), (6, 0)):
            lp[r, c] = float("-inf")
    return lp.numpy().copy()


@functools.lru_cache(maxsize=None)
def _candidates(V, n, T, seed):
    """[ROWS][n] candidate index arrays of the restatement."""
    lp = _lp(V)
    tol = cs.near_tie_tol(lp, T)
    sc = cs.all_scores(lp, seed, n, T)
    assert np.isfinite(sc[np.broadcast_to(np.isfinite(lp)[:, None, :] | np.isnan(lp)[:, None, :], sc.shape)]).all()
    return [[cs.draw_candidates(sc[r, c], tol) for c in range(n)] for r in range(ROWS)]


def _sample(lp, V, n, T, seed, ntok, pad, rows=ROWS, s=S, fill=-7):
    from boficap_amd import hip
    lpd = torch.from_numpy(lp).cuda()
    out = torch.full((max(rows // max(s, 1), 1) * max(n, 1), s), fill, dtype=torch.int64, device="cuda")
    nt = None if ntok is None else torch.tensor(ntok, dtype=torch.int32, device="cuda")
    rc = hip.lib().bofi_vocab_sample(hip.ptr(lpd), rows, V, s, n, float(T), seed, hip.ptr(nt), pad, hip.ptr(out), hip.stream_ptr())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def _check_ids(out, cands, n, ntok, pad, what):
    for row in range(ROWS):
        b, t = divmod(row, S)
        for c in range(n):
            got = int(out[b * n + c, t])                           # draw c of image b lands in row b * n + c
            if ntok is not None and t >= ntok[b]:
                assert got == pad, (what, row, c, got)
            else:
                assert got in cands[row][c], (what, row, c, got, cands[row][c][:4])


def test_near_tie_share_of_the_cases_below():
    """From the restatement alone: how many of the draws the cases below check have more than one candidate."""
    ties = total = 0
    for V in VS:
        for n in NS:
            for T in TS:
                for seed in SEEDS:
                    for row in _candidates(V, n, T, seed):
                        total += len(row)
                        ties += sum(len(c) > 1 for c in row)
    print(f"bofi_vocab_sample cases: {ties} of {total} draws have more than one candidate")
    assert ties <= TIE_CAP * total, (ties, total)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("V", VS)
def test_vocab_sample_draws_the_restated_ids(V, n, T, seed):
    lp = _lp(V)
    cands = _candidates(V, n, T, seed)
    pad = 3 if (V > 3 and n == 7) else 0                             # (a pad id of its own: a hard-wired 0 would show)
    rc, out = _sample(lp, V, n, T, seed, NTOK, pad)
    assert rc == BOFI_OK and out.shape == (B * n, S)
    _check_ids(out, cands, n, NTOK, pad, "ntok")
    rc, out = _sample(lp, V, n, T, seed, None, pad)
    assert rc == BOFI_OK
    _check_ids(out, cands, n, None, pad, "ntok = NULL")
    assert (out.reshape(B, n, S)[INF_ROW // S, :, INF_ROW % S] == 0).all()          # nothing beats -inf: id 0
    if T == 1e-3:
        # the Gumbel term lies in [-3.14, 16.64]: a row whose two largest log-probs differ by more than 19.8 T draws its argmax
        x = np.where(np.isnan(lp), np.float32(-10.0), lp).astype(np.float64)
        for row in range(ROWS):
            if V == 1 or not np.isfinite(x[row]).any():
                continue
            top = np.sort(x[row])[-2:]
            if top[1] - top[0] > 19.8 * T + 1e-6:
                b, t = divmod(row, S)
                assert (out[b * n:(b + 1) * n, t] == int(x[row].argmax())).all(), row


def test_vocab_sample_argument_checks():
    lp = _lp(257)
    assert _sample(lp, 257, 0, 1.0, 1, None, 0)[0] == BOFI_ERR_ARG
    assert _sample(lp, 257, 1, 0.0, 1, None, 0)[0] == BOFI_ERR_ARG
    assert _sample(lp, 257, 1, 1.0, 1, None, 0, rows=ROWS - 1)[0] == BOFI_ERR_ARG
    rc, out = _sample(lp, 257, 2, 1.0, 1, None, 0, rows=0)
    assert rc == BOFI_OK and (out == -7).all()                       # nothing written


@functools.lru_cache(maxsize=None)
def _edge_counter(s0=12345):
    """The first counter j of stream s0 whose hash is one of the 128 that the float32 conversion rounds to 2^32."""
    step = 1 << 22
    for lo in range(0, 1 << 28, step):
        h = cs.hash64_hi(s0, np.arange(lo, lo + step, dtype=np.uint64))
        hit = np.flatnonzero(h >= 0xFFFFFF80)
        if hit.size:
            return lo + int(hit[0]), int(h[hit[0]])
    raise AssertionError("no edge hash in 2^28 counters")


@pytest.mark.parametrize("i_star", [100, 400])
def test_vocab_sample_at_the_rounding_edge_of_the_uniform(i_star):
    """A hash >= 0xFFFFFF80 placed on element i* (log-prob -40) of one draw: the uniform number must stay below 1, so the draw is the
    restatement's id and not i*.  (Without the bound u == 1.0f, the Gumbel value is +inf and i* wins.)"""
    s0, V, n, row, c, T = 12345, 600, 7, 7, 3, 1.0
    j, h = _edge_counter(s0)
    assert h >= 0xFFFFFF80
    target = (row * n + c) * V + i_star
    seed = (s0 + (j - target) * cs.GOLDEN) % (1 << 64)
    assert int(cs.hash64_hi(seed, np.array([target], dtype=np.uint64))[0]) == h
    g = torch.Generator().manual_seed(77 + i_star)
    lp = torch.log_softmax(torch.randn(ROWS, V, generator=g), -1).numpy().copy()
    lp[row, i_star] = -40.0
    tol = cs.near_tie_tol(lp, T)
    sc = cs.all_scores(lp, seed, n, T)
    assert np.isfinite(sc).all()
    cands = [[cs.draw_candidates(sc[r, k], tol) for k in range(n)] for r in range(ROWS)]
    ties = sum(len(x) > 1 for r_ in cands for x in r_)
    print(f"placed edge, i* = {i_star}: counter {j} of stream {s0} has hash {h:#x}; {ties} of {ROWS * n} draws have more than one candidate")
    assert ties <= TIE_CAP * ROWS * n and len(cands[row][c]) == 1 and int(cands[row][c][0]) != i_star
    # the rule without the bound does draw i* here: the case is placed where it matters
    assert int(np.argmax(cs.gumbel_scores(lp[row], seed, row, c, n, T, cs.uniform_unclamped))) == i_star
    rc, out = _sample(lp, V, n, T, seed, None, 0)
    assert rc == BOFI_OK
    b, t = divmod(row, S)
    got = int(out[b * n + c, t])
    assert got == int(cands[row][c][0]), f"device drew {got}, the restatement {int(cands[row][c][0])} (i* = {i_star})"
    _check_ids(out, cands, n, None, 0, "edge")


# ------------------------------------------------------------------------------------------------ bofi_vocab_stats
@pytest.mark.parametrize("V", [1, 255, 257, 9491])
def test_vocab_stats_against_float64(V):
    from boficap_amd import hip
    rows = 7
    g = torch.Generator().manual_seed(50 + V)
    lp = torch.log_softmax(3 * torch.randn(rows, V, generator=g), -1)
    lp[3, V // 2] = float("-inf")                                    # exp(-inf) * -inf = NaN, as in torch's float32 expression
    seq = torch.randint(0, V, (rows,), generator=g)
    seq[3] = V // 2
    lpd, seqd = lp.cuda(), seq.cuda()
    plogp = torch.full((rows,), -5.0, device="cuda")
    chosen = torch.full((rows,), -5.0, device="cuda")
    assert hip.lib().bofi_vocab_stats(hip.ptr(lpd), hip.ptr(seqd), rows, V, hip.ptr(plogp), hip.ptr(chosen), hip.stream_ptr()) == BOFI_OK
    torch.cuda.synchronize()
    ref64 = (lp.double().exp() * lp.double()).sum(1)
    ref32 = (lp.exp() * lp).sum(1)
    got = plogp.cpu()
    assert torch.equal(got.isnan(), ref32.isnan()) and bool(got.isnan()[3]) and int(got.isnan().sum()) == 1
    ok = ~ref64.isnan()
    err = float((got.double()[ok] - ref64[ok]).abs().max())
    print(f"vocab_stats V = {V}: max |sum p log p - float64| = {err:.2e}")
    assert err < 1e-4
    assert torch.equal(chosen.cpu().view(torch.int32), lp[torch.arange(rows), seq].view(torch.int32))       # bit-equal
    assert hip.lib().bofi_vocab_stats(hip.ptr(lpd), hip.ptr(seqd), 0, V, hip.ptr(plogp), hip.ptr(chosen), hip.stream_ptr()) == BOFI_OK
    assert hip.lib().bofi_vocab_stats(hip.ptr(lpd), hip.ptr(seqd), rows, 0, hip.ptr(plogp), hip.ptr(chosen), hip.stream_ptr()) == BOFI_ERR_ARG


# ------------------------------------------------------------------------------------------------ bofi_rl_take_draws
@pytest.mark.parametrize("with_mask", [True, False])
@pytest.mark.parametrize("p0,p1", [(0, 6), (2, 3), (3, 3), (1, 10)])
def test_rl_take_draws_against_torch_indexing(p0, p1, with_mask):
    from boficap_amd import hip
    N, S_, V = 5, 6, 37
    g = torch.Generator().manual_seed(9)
    lp = torch.log_softmax(torch.randn(N, S_, V, generator=g), -1)
    tok = torch.randint(0, V, (N, S_), generator=g)
    tok[0, 0], tok[1, 2], tok[2, 1], tok[4, 3] = -1, V, -1, V                  # ids outside the vocabulary: a NaN log-prob
    plen = torch.tensor([[2, 1, 0, 2, 1, 0], [0, 3, 1, 0, 0, 2], [1, 1, 1, 1, 1, 1], [0, 0, 0, 0, 0, 0], [3, 0, 2, 1, 0, 0]], dtype=torch.int32)
    seq0 = torch.full((N, S_), -99, dtype=torch.int64)
    drawn0 = torch.full((N, S_), -777.0)
    mask0 = torch.full((N, S_), 7, dtype=torch.uint8)
    # reference: positions of phrases [p0, p1) take the token, its log-prob under its own row, and the mark
    cum = torch.cat([torch.zeros(N, 1, dtype=torch.int64), plen.long().cumsum(1)], 1)
    lo, hi = cum[:, min(p0, S_)], cum[:, min(p1, S_)]
    t = torch.arange(S_)
    inside = (t >= lo[:, None]) & (t < hi[:, None])
    valid = (tok >= 0) & (tok < V)
    picked = torch.where(valid, lp.gather(2, tok.clamp(0, V - 1).unsqueeze(2)).squeeze(2), torch.tensor(float("nan")))
    seq_ref, drawn_ref = torch.where(inside, tok, seq0), torch.where(inside, picked, drawn0)
    mask_ref = torch.where(inside, torch.tensor(1, dtype=torch.uint8), mask0)
    if (p0, p1) == (0, 6):
        assert bool((inside & ~valid).any()) and bool((~inside).any())         # the cases do hold what they are for
    lpd, tokd, plend = lp.cuda(), tok.cuda(), plen.cuda()
    seq, drawn, mask = seq0.cuda(), drawn0.cuda(), mask0.cuda()
    rc = hip.lib().bofi_rl_take_draws(hip.ptr(lpd), hip.ptr(tokd), hip.ptr(plend), N, S_, V, p0, p1, hip.ptr(seq), hip.ptr(drawn),
                                      hip.ptr(mask) if with_mask else None, hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == BOFI_OK
    assert torch.equal(seq.cpu(), seq_ref)
    assert torch.equal(drawn.cpu().isnan(), drawn_ref.isnan())
    assert torch.equal(drawn.cpu().nan_to_num(0.0).view(torch.int32), drawn_ref.nan_to_num(0.0).view(torch.int32))
    assert torch.equal(mask.cpu(), mask_ref if with_mask else mask0)
    assert hip.lib().bofi_rl_take_draws(hip.ptr(lpd), hip.ptr(tokd), hip.ptr(plend), N, S_, V, 3, 2, hip.ptr(seq), hip.ptr(drawn), None,
                                        hip.stream_ptr()) == BOFI_ERR_ARG


# ------------------------------------------------------------------------------------------------ the engine's callers
def _engine(weight_cache, manifest, case):
    from boficap_amd.engine import BofiEngine
    m = manifest[case]
    cfg, sd = weight_cache(m["config"], m["seed"], m["gen_scale"], m["digest"], m.get("patch"))
    eng = BofiEngine(cfg, torch.float32, max_batch=16, max_regions=36)
    eng.load_state_dict(sd)
    g = load_golden(case)
    att = torch.from_numpy(g["att_feats"]).cuda()
    att_len = torch.from_numpy(g["att_masks"]).sum(1).to(torch.int32).cuda() if "att_masks" in g else None
    return cfg, eng, att, att_len


def _check_saic(r, T, seed, pad):
    """Every id inside a phrase against the restatement.  The loop's iteration `it` draws phrase it - 1 of every image with the seed
    seed + it * golden, n = 1, from the row it returns as seq_logprob[b, t] (saic_copy_kernel copies the drawn id and its row from the
    same index b * S + t).  An iteration that ends the decode on a NaN copies nothing: its rows stay zero and its ids pad.
    Returns (ids checked, near ties, last iteration seen)."""
    seq, lp, pl = r["seq"].cpu().numpy(), r["seq_logprob"].cpu().numpy(), r["phrase_length"].cpu().numpy()
    nb, s = seq.shape
    checked = ties = last_it = 0
    for b in range(nb):
        t = 0
        for j in range(s):
            for _ in range(int(pl[b, j])):
                if t >= s:
                    break
                if (lp[b, t] == 0).all():
                    assert seq[b, t] == pad
                else:
                    eff = (seed + (j + 1) * cs.GOLDEN) % (1 << 64)
                    cand = cs.draw_candidates(cs.gumbel_scores(lp[b, t], eff, b * s + t, 0, 1, T), cs.near_tie_tol(lp[b, t], T))
                    assert int(seq[b, t]) in cand, (b, t, j + 1, int(seq[b, t]), cand[:4])
                    checked += 1
                    ties += len(cand) > 1
                    last_it = max(last_it, j + 1)
                t += 1
    return checked, ties, last_it


@pytest.mark.parametrize("case", ["tiny_mix", "tiny_saic_multi"])
def test_sampled_saic_loop_replayed_on_the_host(case, weight_cache, manifest):
    """decode_saic(sample=...) eager and captured: the row list, the halt word and the seed word in device memory are arguments that
    only the engine passes to the sampler.  tiny_mix ends on the reference's 'phrase nan!' return in its first iteration (nothing is
    emitted: the check is that nothing is); tiny_saic_multi runs several iterations, the row-list ones among them."""
    cfg, eng, att, att_len = _engine(weight_cache, manifest, case)
    T = 0.7
    checked = ties = 0
    for seed in (4242, 2 ** 63 + 99):
        r = eng.decode_saic(att, att_len, sample=(T, seed))
        torch.cuda.synchronize()
        k, ti, last_it = _check_saic(r, T, seed, cfg.pad_idx)
        checked, ties = checked + k, ties + ti
        if case == "tiny_saic_multi":
            assert k > 2 * att.size(0) and last_it >= 3, (k, last_it)
    rg = None
    for seed in (31337, 2 ** 64 - 5):                                # one capture, replayed with a new seed word
        rg = eng.decode_saic(att, att_len, sample=(T, seed), graph=True, out=rg)
        torch.cuda.synchronize()
        k, ti, last_it = _check_saic(rg, T, seed, cfg.pad_idx)
        checked, ties = checked + k, ties + ti
        if case == "tiny_saic_multi":
            assert k > 2 * att.size(0) and last_it >= 3, (k, last_it)
    print(f"sampled SAIC loop ({case}): {ties} of {checked} checked ids have more than one candidate")
    assert ties <= TIE_CAP * max(checked, 1)


def test_engine_sample_tokens_at_every_position(weight_cache, manifest):
    cfg, eng, att, att_len = _engine(weight_cache, manifest, "tiny_mix")
    out = eng.decode_naic(att, att_len)
    n, T, seed = 4, 0.7, 2 ** 63 + 777
    ids = eng.sample_tokens(out, n=n, temperature=T, seed=seed).cpu().numpy()
    lp, ntok = out["seq_logprob"].cpu().numpy(), out["phrase_length"].sum(1).cpu().numpy()
    nb, s, V = lp.shape
    assert ids.shape == (nb * n, s) and int(ntok.max()) > 1
    checked = ties = 0
    for b in range(nb):
        for t in range(s):
            if t >= ntok[b]:
                assert (ids[b * n:(b + 1) * n, t] == cfg.pad_idx).all()
                continue
            sc = cs.gumbel_scores(lp[b, t], seed, b * s + t, np.arange(n), n, T)
            tol = cs.near_tie_tol(lp[b, t], T)
            for c in range(n):
                cand = cs.draw_candidates(sc[c], tol)
                assert int(ids[b * n + c, t]) in cand, (b, t, c, int(ids[b * n + c, t]), cand[:4])
                checked += 1
                ties += len(cand) > 1
    print(f"sample_tokens: {ties} of {checked} checked ids have more than one candidate")
    assert checked >= n * int(ntok.sum()) > 0 and ties <= TIE_CAP * checked
