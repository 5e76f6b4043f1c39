"""bofi_rouge_score (csrc/rouge.hip) against the float64 restatement of tests/test_rouge.py: the longest-common-subsequence integers and the
argmax references exactly, the scores within 1e-15 (every operation is one correctly rounded fp64 operation in the restatement's order, so
bit equality is expected; the margin is one ulp per operation of a value below 1)."""
import numpy as np
import pytest
import torch

from test_rouge import eval_ids, restated_rouge, reward_ids, rouge_of

pytestmark = pytest.mark.gpu

TOL = 1e-15


def launch(refs, seq, seq_per_img, rule="reward", cand_len=None):
    """The kernel on token lists ``refs`` (per image) and rows ``seq``: (scores, lcs of every pair, best) as numpy arrays."""
    from boficap_amd import cider
    from boficap_amd.rouge import Rouge
    sc = Rouge(rule=rule, device="cuda")
    seq = torch.as_tensor(np.asarray(seq, dtype=np.int64)).cuda().contiguous()
    pk = cider.upload(cider.pack_host(refs, seq.shape[0], seq.shape[1], seq_per_img, None), sc.device, None)
    cl = None if cand_len is None else torch.as_tensor(np.asarray(cand_len, dtype=np.int32)).cuda()
    out, lcs, best = sc._launch(pk, seq, cl, seq_per_img, True, True)
    torch.cuda.synchronize()
    return out.cpu().numpy(), lcs.cpu().numpy(), best.cpu().numpy()


def restate(refs, seq, seq_per_img, rule="reward", cand_len=None):
    """The restatement on the same token lists."""
    ids = reward_ids if rule == "reward" else eval_ids
    scores, pairs, best = [], [], []
    for j, row in enumerate(np.asarray(seq).tolist()):
        cand = row[: int(cand_len[j])] if cand_len is not None else ids(row)
        s, l, bp, br = rouge_of(cand, refs[j // seq_per_img])
        scores.append(s); pairs.extend(l); best.append([bp, br])
    return np.array(scores), np.array(pairs), np.array(best).reshape(-1, 2)


def check(refs, seq, seq_per_img, rule="reward", cand_len=None):
    got = launch(refs, seq, seq_per_img, rule, cand_len)
    want = restate(refs, seq, seq_per_img, rule, cand_len)
    assert got[1].tolist() == want[1].tolist()
    assert got[2].tolist() == want[2].tolist()
    err = float(np.abs(got[0] - want[0]).max())
    print(f"max |score - restatement| = {err:.3e} over {len(want[0])} candidates, lcs in [{want[1].min()}, {want[1].max()}]")
    assert err <= TOL
    return got, want


CAND_LENS = [0, 1, 20, 32, 33, 63, 64]
REF_LENS = [1, 31, 32, 33, 64]


@pytest.mark.parametrize("how", ["cand_len", "eval", "reward"])
def test_word_and_half_word_edges(how):
    """Candidate lengths 0, 1, 20, 32, 33, 63, 64 against reference lengths 1, 31, 32, 33, 64 (the edges of a 64-bit bit-vector form), the lengths
    handed over or found by either token rule."""
    rng = np.random.default_rng(3)
    lens = [t for t in CAND_LENS if not (how == "reward" and t == 0)]      # (array_to_str's rule has no empty row: the first 0 counts)
    seq = rng.integers(1, 5, (len(lens), 64))
    refs = [[[int(t) for t in rng.integers(1, 5, n)] for n in REF_LENS] for _ in lens]
    if how == "eval":
        for j, t in enumerate(lens):
            seq[j, t:] = 0                                                 # T ids, then the stop
    elif how == "reward":
        for j, t in enumerate(lens):
            seq[j, t - 1:] = 0                                             # T - 1 ids and the 0 that counts
    got, want = check(refs, seq, 1, "eval" if how == "eval" else "reward", lens if how == "cand_len" else None)
    assert want[1].max() >= 20


def test_equal_reversed_and_extreme_ids():
    S = 64
    up = list(range(1, S + 1))
    seq = np.array([[7] * S, up, up[::-1], [0, 65534] * (S // 2), [65534] * S], dtype=np.int64)
    refs = [[[7] * 64, [7] * 33, [7]],                    # all tokens equal: lcs = the shorter length
            [up[::-1], up],                               # strictly reversed: 1; identical: 64
            [up, up[::-1][:40]],
            [[65534, 0] * 32, [0] * 10, [65534]],
            [[65534] * 5, [0, 65534, 0]]]
    got, want = check(refs, seq, 1, cand_len=[S] * 5)
    assert want[1].tolist()[:5] == [64, 33, 1, 1, 64]
    check(refs, seq, 1, "reward")                        # the 0 of row 3 ends it at once under the first-0 rule
    check(refs, seq, 1, "eval")


@pytest.mark.parametrize("seq_per_img", [1, 5])
def test_ragged_reference_counts_and_the_lane_loop(seq_per_img):
    """1, 5 and 7 references per image, ragged in one call, and an image with 70 (more than a wavefront's lanes)."""
    rng = np.random.default_rng(11 + seq_per_img)
    counts = [1, 5, 7, 70, 5]
    refs = [[[int(t) for t in rng.integers(1, 9, int(rng.integers(1, 21)))] for _ in range(c)] for c in counts]
    refs[3][2] = [1, 2, 3, 4, 5, 6, 7, 8] * 2 + [1, 2, 3, 4]
    refs[3][66] = list(refs[3][2])                       # a tie across the lane loop: the lower index wins
    seq = rng.integers(0, 9, (len(counts) * seq_per_img, 20))
    seq[:, 0] = np.maximum(seq[:, 0], 1)
    seq[3 * seq_per_img] = 0
    seq[3 * seq_per_img, :len(refs[3][2])] = refs[3][2]  # this candidate IS reference 2 (and 66) of its image
    got, want = check(refs, seq, seq_per_img, "eval")
    assert want[2][3 * seq_per_img, 0] == 2 and want[1].max() == 20
    check(refs, seq, seq_per_img, "reward")
    check(refs, seq, seq_per_img, cand_len=rng.integers(0, 21, seq.shape[0]))


def test_random_corpus_and_the_public_interface():
    """64 images x 5 samples x 5-7 random references over a 30-id vocabulary; ``score`` (no synchronisation, rows as the trainer hands them),
    ``bind`` and ``compute_score``; two runs agree bit for bit."""
    from boficap_amd.rouge import Rouge
    rng = np.random.default_rng(5)
    data_gts = []
    for _ in range(64):
        g = rng.integers(1, 31, (int(rng.integers(5, 8)), 18))
        for row in g:
            row[int(rng.integers(3, 18)):] = 0
        data_gts.append(g)
    seq = rng.integers(1, 31, (64 * 5, 16))
    for row in seq:
        row[int(rng.integers(0, 17)):] = 0
    for rule in ("reward", "eval"):
        sc = Rouge(rule=rule)
        dseq = torch.from_numpy(seq).cuda()
        out, o64, lcs, best = sc.score(data_gts, dseq, 5, out64=True, lcs=True, best=True)
        again = sc.bind(data_gts, 5)(dseq)
        torch.cuda.synchronize()
        want = restated_rouge(data_gts, seq, 5, rule)
        assert lcs.cpu().numpy().tolist() == want[1].tolist() and best.cpu().numpy().tolist() == want[2].tolist()
        err = float(np.abs(o64.cpu().numpy() - want[0]).max())
        print(f"{rule}: max |score - restatement| = {err:.3e}; lcs values {sorted(set(want[1].tolist()))}")
        assert err <= TOL
        assert len(set(want[1].tolist())) >= 7                                   # the subsequence lengths are spread widely
        assert out.dtype == torch.float32 and torch.equal(out, o64.float()) and torch.equal(out, again)
    # the package's contract, on the 'eval' token lists as id strings
    gts = {i: [" ".join(map(str, eval_ids(r))) for r in g] for i, g in enumerate(data_gts)}
    res = {i: [" ".join(map(str, eval_ids(seq[5 * i])))] for i in range(64)}
    mean, arr = Rouge(device="cuda").compute_score(gts, res)
    want = np.array([rouge_of(eval_ids(seq[5 * i]), [eval_ids(r) for r in data_gts[i]])[0] for i in range(64)])
    assert float(np.abs(arr - want).max()) <= TOL and abs(mean - float(np.mean(want))) <= TOL


def test_bad_arguments_are_refused_without_a_launch():
    from boficap_amd import hip
    lib = hip.lib()
    seq = torch.ones(2, 8, dtype=torch.int64, device="cuda")
    start = torch.tensor([0, 1, 2], dtype=torch.int32, device="cuda")
    tok = torch.ones(2, 65, dtype=torch.int32, device="cuda")
    lens = torch.ones(2, dtype=torch.int32, device="cuda")
    out = torch.full((2,), -1.0, dtype=torch.float64, device="cuda")

    def call(seq=seq, N=2, S=8, spi=1, start=start, tok=tok, lens=lens, width=8, rule=0, beta=1.2, out=out):
        return lib.bofi_rouge_score(hip.ptr(seq), None, N, S, spi, hip.ptr(start), hip.ptr(tok), hip.ptr(lens), width, rule, beta, hip.ptr(out), None, None,
                                    hip.stream_ptr())
    assert call(width=65) == 1
    assert call(start=None) == 1
    assert call(S=65) == 1 and call(S=0) == 1 and call(spi=0) == 1 and call(N=3, spi=2) == 1 and call(rule=2) == 1 and call(beta=0.0) == 1
    assert call(seq=None) == 1 and call(lens=None) == 1 and call(out=None) == 1 and call(tok=None) == 1
    torch.cuda.synchronize()
    assert out.tolist() == [-1.0, -1.0]                                          # nothing ran
    assert call(N=0) == 0
    assert call() == 0
    torch.cuda.synchronize()
    assert all(abs(v - rouge_of([1] * 8, [[1]])[0]) <= TOL for v in out.tolist())
