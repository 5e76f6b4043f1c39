"""bofi_vocab_block (rb_vocab_kernel, boficap_amd/csrc/rowblock.hip) on the MI355X: the generator with the vocabulary epilogue inside, against the logits
bofi_linear_block(y_f32 = 1) forms from the same inputs -- ids, pad tail and NaN behaviour exactly, the two row statistics against float64 computed from
those float32 logits.  Bar of the statistics: 2e-5 absolute, the project's bar for these two quantities (test_gpu_naic.py,
test_entropy_perplexity_without_materialising_logprobs)."""
import itertools
import math

import pytest
import torch

from conftest import record_parity

pytestmark = pytest.mark.gpu

STAT_BAR = 2e-5
D = 512
SHAPES = [(M, V, Npad) for M in (1, 70, 97) for V, Npad in ((40, 64), (300, 320), (1000, 1024))] + [(70, 9491, 9600)]
# (40, 64): one chunk, seven idle wavefronts; (300, 320): fewer chunks than wavefronts; (1000, 1024): two chunks per wavefront (the running maximum is rescaled);
# (9491, 9600): the model's shape, uneven chunks per wavefront, a chunk of pad columns only.  M: 70 / 97 = a full 64- / 96-row block and a ragged one.
VARIANTS = ["negative", "twins", "last_column", "first_column"]
CASES = [(M, V, Npad, v) for (M, V, Npad) in SHAPES for v in VARIANTS if not (v == "twins" and Npad < 128)]      # (one chunk: no second wavefront to own the twin)


@pytest.fixture(scope="module")
def H():
    from boficap_amd import hip
    assert torch.cuda.is_available(), "these tests need the MI355X"
    hip.lib()
    return hip


def _case(H, M, V, Npad, variant):
    """Inputs on the device + the reference logits [M, V] (float32, bofi_linear_block on the same inputs)."""
    g = torch.Generator().manual_seed(M * 131 + V + len(variant))
    x = torch.randn(M, D, generator=g) * 2.0 - 0.3
    w = torch.zeros(Npad, D)
    w[:V] = (torch.randn(V, D, generator=g) / math.sqrt(D)).to(torch.bfloat16).float()
    c, cs = torch.zeros(Npad), torch.zeros(Npad)
    c[:V] = torch.randn(V, generator=g) * 0.1
    if variant == "negative":                 # every real logit below the pad columns' 0: an unmasked pad column would win
        c[:V] -= 8.0
    elif variant == "twins":                  # the same weight row and bias in two chunks that different wavefronts own (at 1 024 columns on: different column classes too)
        a, b = 5, 69 if Npad < 1024 else 581
        assert b < V and (b // 64) % 8 != (a // 64) % 8
        w[b] = w[a]
        c[a] = c[b] = 40.0
    elif variant == "last_column":
        c[V - 1] = 40.0
    elif variant == "first_column":
        c[0] = 40.0
    cs[:V] = w[:V].double().sum(1).float()
    nan_row = 3 if M > 8 else None
    if nan_row is not None:
        x[nan_row, 77] = float("nan")
    S = 7 if M % 7 == 0 else M
    ntok = torch.randint(2, S + 2, (M // S,), generator=g).to(torch.int32)          # row (b, t) is padded when t >= ntok[b] - 1
    if nan_row is not None:
        ntok[0] = S + 1                                                             # (the NaN row emits its own id)
    xc, cc, csc = x.cuda(), c.cuda(), cs.cuda()
    wp = torch.empty(Npad * D, dtype=torch.bfloat16, device="cuda")
    H.check(H.lib().bofi_pack_frag(H.ptr(w.to(torch.bfloat16).cuda()), H.ptr(wp), Npad, D, H.stream_ptr()))
    y = torch.empty(M, Npad, dtype=torch.float32, device="cuda")
    H.check(H.lib().bofi_linear_block(H.ptr(xc), D, H.ptr(wp), H.ptr(cc), H.ptr(csc), H.ptr(y), Npad, 1, M, Npad, 0, H.stream_ptr()))
    torch.cuda.synchronize()
    return dict(x=xc, wp=wp, c=cc, cs=csc, ntok=ntok.cuda(), S=S, nan_row=nan_row, ref=y.cpu()[:, :V].clone(), ntok_host=ntok)


def _run(H, k, M, V, pad_idx, alone):
    seq = torch.full((M,), -7, dtype=torch.int64, device="cuda")
    plogp = torch.full((M,), 7.0, device="cuda")
    chosen = torch.full((M,), 7.0, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    H.vocab_block(k["x"], k["wp"], k["c"], k["cs"], V, k["S"], seq, ntok=k["ntok"], ntok_bias=-1, pad_idx=pad_idx, row_plogp=plogp, row_chosen=chosen,
                  nan_flag=flag, alone=alone)
    torch.cuda.synchronize()
    return seq.cpu(), plogp.cpu(), chosen.cpu(), int(flag.cpu())


@pytest.mark.parametrize("M,V,Npad,variant", CASES)
def test_vocab_block_vs_materialised_logits(H, M, V, Npad, variant, monkeypatch):
    k = _case(H, M, V, Npad, variant)
    pad_idx = 0 if variant != "first_column" else 2
    ref, S = k["ref"], k["S"]
    rows = torch.arange(M)
    padded = (rows % S) >= (k["ntok_host"][rows // S].long() - 1)
    nan = torch.zeros(M, dtype=torch.bool)
    if k["nan_row"] is not None:
        nan[k["nan_row"]] = True
        assert ref[k["nan_row"]].isnan().all() and not ref[~nan].isnan().any()
    want = ref.nan_to_num(nan=-1e30).argmax(1)                  # first maximum of the raw logits over [0, V)
    want[nan] = 0
    want[padded] = pad_idx
    lp = torch.log_softmax(ref.double(), 1)
    want_plogp = (lp.exp() * lp).sum(1)
    want_chosen = lp[rows, want]
    if variant == "twins":
        assert (want[~padded & ~nan] == 5).all()
    if variant == "last_column":
        assert (want[~padded & ~nan] == V - 1).all()
    if variant == "negative":
        assert float(ref[~nan].max()) < 0.0

    outs = []
    try:
        for mt, split, alone in itertools.product((4, 6), (0, 1, 2, 4), (False, True)):
            monkeypatch.setenv("BOFI_VOCAB_MT", str(mt))
            monkeypatch.setenv("BOFI_VOCAB_SPLIT", str(split))
            H.lib().bofi_reload_env()
            outs.append(_run(H, k, M, V, pad_idx, alone))
    finally:
        monkeypatch.delenv("BOFI_VOCAB_MT")
        monkeypatch.delenv("BOFI_VOCAB_SPLIT")
        H.lib().bofi_reload_env()
    seq, plogp, chosen, flag = outs[0]
    assert torch.equal(seq, want), (seq != want).nonzero().flatten()[:8]
    assert flag == int(nan.any())
    assert plogp[nan].isnan().all() and chosen[nan].isnan().all() and not plogp[~nan].isnan().any() and not chosen[~nan].isnan().any()
    e_plogp = float((plogp[~nan].double() - want_plogp[~nan]).abs().max())
    e_chosen = float((chosen[~nan].double() - want_chosen[~nan]).abs().max())
    print(f"vocab_block M={M} V={V} {variant}: |row_plogp - f64| max {e_plogp:.3e}, |row_chosen - f64| max {e_chosen:.3e}")
    if variant == "negative":
        record_parity(f"vocab_block_row_plogp_M{M}_V{V}", e_plogp, STAT_BAR, "rb_vocab_kernel against float64 on bofi_linear_block's float32 logits")
        record_parity(f"vocab_block_row_chosen_M{M}_V{V}", e_chosen, STAT_BAR, "as above, log-prob of the emitted id (pad tail included)")
    assert e_plogp <= STAT_BAR and e_chosen <= STAT_BAR
    # block size, column split and `alone`: the same bits
    for o in outs[1:]:
        assert torch.equal(o[0], seq) and o[3] == flag
        assert torch.equal(o[1].view(torch.int32), plogp.view(torch.int32)) and torch.equal(o[2].view(torch.int32), chosen.view(torch.int32))


def test_vocab_block_rows_do_not_depend_on_the_launch(H):
    """A row's outputs are the same bits whether it is decoded among 97 rows or alone."""
    M, V, Npad = 97, 1000, 1024
    k = _case(H, M, V, Npad, "negative")
    whole = _run(H, dict(k, ntok=None), M, V, 0, False)
    for r in (0, 64, 96):
        one = dict(k, x=k["x"][r:r + 1].contiguous(), ntok=None, S=1)
        got = _run(H, one, 1, V, 0, False)
        assert int(got[0]) == int(whole[0][r])
        assert torch.equal(got[1].view(torch.int32), whole[1][r:r + 1].view(torch.int32)) and torch.equal(got[2].view(torch.int32), whole[2][r:r + 1].view(torch.int32))
