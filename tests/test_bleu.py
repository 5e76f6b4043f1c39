"""BLEU-4 reward term, host side: a float64 restatement of BLEU as the pycocoevalcap package computes it (``Bleu(4)``, bleu_scorer.py with
option 'closest', the ``bleu_scores[3]`` of captioning/utils/rewards.py:86-131) written here from the rules alone, the issue's worked
table, and boficap_amd.bleu's host packing and argument checks.  tests/test_gpu_bleu.py holds the device side against the same
restatement."""
import math

import numpy as np
import pytest

from test_cider import ids_of_row, ngram_counts

# ---------------------------------------------------------------- the float64 restatement (independent of boficap_amd)

TINY, SMALL = 1e-15, 1e-9


def bleu_comps(cand, refs, n=4):
    """(testlen, reflen, guess[n], correct[n]) of one candidate token list against its references' token lists."""
    T = len(cand)
    maxref = {}
    for r in refs:
        for g, c in ngram_counts(r, n).items():
            maxref[g] = max(maxref.get(g, 0), c)
    correct = [0] * n
    for g, c in ngram_counts(cand, n).items():
        correct[len(g) - 1] += min(maxref.get(g, 0), c)
    reflen = min((abs(len(r) - T), len(r)) for r in refs)[1]          # 'closest'; a tie goes to the shorter reference
    return T, reflen, [max(0, T - k) for k in range(n)], correct


def bleu_of(testlen, reflen, guess, correct, n=4):
    """BLEU-1..n of one sentence's counts (or of the corpus' summed counts)."""
    b, out = 1.0, []
    for k in range(n):
        b *= (float(correct[k]) + TINY) / (float(guess[k]) + SMALL)
        out.append(b ** (1.0 / (k + 1)))
    ratio = (testlen + TINY) / (reflen + SMALL)
    if ratio < 1:
        out = [x * math.exp(1 - 1 / ratio) for x in out]
    return out


def corpus_bleu(comps, n=4):
    """The corpus score: the same formula on the summed counts."""
    tl = sum(c[0] for c in comps)
    rl = sum(c[1] for c in comps)
    return bleu_of(tl, rl, [sum(c[2][k] for c in comps) for k in range(n)], [sum(c[3][k] for c in comps) for k in range(n)], n)


def restated_bleu(data_gts, seq, seq_per_img):
    """get_scores' BLEU for every row of seq [N, S]: (BLEU-4 float64 [N], comps int [N, 10] as the device lays them out, comps as tuples)."""
    seq = np.asarray(seq)
    refs = [[ids_of_row(r) for r in np.asarray(g)] for g in data_gts]
    comps = [bleu_comps(ids_of_row(seq[j]), refs[j // seq_per_img]) for j in range(seq.shape[0])]
    flat = np.array([[c[0], c[1], *c[2], *c[3]] for c in comps], dtype=np.int64).reshape(-1, 10)
    return np.array([bleu_of(*c)[3] for c in comps]), flat, comps


# the issue's worked table: candidate, references, comps (testlen, reflen, guess, correct), BLEU-4
WORKED = [
    ([5, 6, 7, 8, 0], [[5, 6, 7, 9, 0], [5, 6, 0]], (5, 5, [5, 4, 3, 2], [4, 2, 1, 0]), 9.036020031392194e-05),
    ([5, 6, 0], [[5, 6, 7, 9, 0], [4, 5, 6, 7, 0]], (3, 5, [3, 2, 1, 0], [3, 1, 0, 0]), 2.427799659296287e-06),
    ([3, 3, 3, 3, 3, 3, 0], [[3, 3, 0], [7, 3, 3, 3, 8, 0]], (7, 6, [7, 6, 5, 4], [4, 3, 2, 0]), 7.31110445570201e-05),
    ([0], [[1, 2, 0]], (1, 3, [1, 0, 0, 0], [1, 0, 0, 0]), 4.2796774227674215e-06),
]


def test_restatement_reproduces_the_worked_table():
    for cand, refs, comps, b4 in WORKED:
        got = bleu_comps(cand, refs)
        assert got == comps, (cand, got)
        assert abs(bleu_of(*got)[3] - b4) <= 1e-20 + 1e-15 * b4, (cand, bleu_of(*got))
    assert abs(bleu_of(*WORKED[0][2])[0] - 0.7999999996800004) <= 1e-16


def test_restatement_rules():
    # 'closest': T = 4 against references of 3 and 5 tokens -> the shorter
    assert bleu_comps([1, 2, 3, 0], [[1, 2, 3, 4, 0], [1, 2, 0]])[1] == 3
    assert bleu_comps([1, 2, 3, 0], [[1, 2, 0], [1, 2, 3, 4, 0]])[1] == 3
    # a row with no 0 is its whole self (array_to_str)
    assert ids_of_row([5, 6, 7]) == [5, 6, 7] and bleu_comps(ids_of_row([5, 6, 7]), [[5, 6, 7, 0]])[:2] == (3, 4)
    # clipping: a candidate n-gram counts at most as often as the reference that holds it most
    T, _, guess, correct = bleu_comps([3, 3, 3, 3, 0], [[3, 3, 0], [3, 0]])
    assert (T, guess, correct) == (5, [5, 4, 3, 2], [3, 2, 1, 0])               # four 3s count 2, (3 3) 1 of 3, (3 3 0) once
    # brevity penalty only below the reference length
    assert bleu_of(4, 4, [4, 3, 2, 1], [4, 3, 2, 1])[3] == pytest.approx(1.0, abs=1e-9)
    assert bleu_of(4, 8, [4, 3, 2, 1], [4, 3, 2, 1])[3] == pytest.approx(math.exp(1 - 2), rel=1e-8)


# ---------------------------------------------------------------- boficap_amd.bleu, host side


def test_host_formula_is_the_restatement():
    from boficap_amd.bleu import bleu_of_comps
    for _, _, comps, _ in WORKED:
        assert bleu_of_comps(*comps) == bleu_of(*comps)                      # the same float operations: bit-equal
    rows = [w[2] for w in WORKED]
    total = (sum(c[0] for c in rows), sum(c[1] for c in rows), [sum(c[2][k] for c in rows) for k in range(4)],
             [sum(c[3][k] for c in rows) for k in range(4)])
    assert bleu_of_comps(*total) == corpus_bleu(rows)


def test_compute_score_checks_its_arguments():
    """The package's assertions, before any device work."""
    from boficap_amd.bleu import Bleu
    sc = Bleu(4, device="cuda")
    with pytest.raises(AssertionError):
        sc.compute_score({0: ["5 6 0"], 1: ["5 0"]}, {0: ["5 6 0"]})             # key sets differ
    with pytest.raises(AssertionError):
        sc.compute_score({0: ["5 6 0"]}, {0: ["5 6 0", "5 0"]})                # two hypotheses
    with pytest.raises(AssertionError):
        sc.compute_score({0: []}, {0: ["5 6 0"]})                              # no reference
    with pytest.raises(AssertionError):
        sc.compute_score({0: "5 6 0"}, {0: ["5 6 0"]})                         # references not a list
    with pytest.raises(ValueError):
        Bleu(3, device="cuda")


def test_reward_scorer_needs_a_term():
    from boficap_amd.rewards import RewardScorer
    with pytest.raises(ValueError):
        RewardScorer(df=None, cider_weight=0.0, bleu_weight=0.0, device="cuda")
    with pytest.raises(ValueError):
        RewardScorer(df=None, cider_weight=-1.0, bleu_weight=0.0, device="cuda")
    sc = RewardScorer(df="no-such-table", cider_weight=0.0, bleu_weight=0.5, device="cuda")    # no CIDEr-D term: the df is never read
    assert sc.df is None and sc.cider_weight == 0.0 and sc.bleu_weight == 0.5


def test_host_packing():
    from boficap_amd import cider, hip
    refs = [[[5, 6, 7, 9, 0], [5, 6, 0]], [[4, 0]]]
    pk = cider.pack_host(refs, 4, 6, 2, None)
    assert pk.R == 3 and pk.width == 5 and pk.stride == 128
    start, lens, tok = pk.parts[:3]
    assert start.tolist() == [0, 2, 3] and lens.tolist() == [5, 3, 2]
    assert tok.reshape(3, 5).tolist() == [[5, 6, 7, 9, 0], [5, 6, 0, 0, 0], [4, 0, 0, 0, 0]]
    assert pk.parts[3].size == 0 and pk.L == 0.0                              # no df table without a CIDEr-D term
    for p, a in zip(pk.parts, pk.offs):                                      # 8-byte aligned sections of the one buffer
        assert a % 2 == 0 and (pk.buf[a:a + p.size] == p).all()
    # df='corpus': every candidate's reference set counts once, L = log(candidates)
    df = cider.DfTable("corpus", "cuda")
    pk = cider.pack_host(refs, 4, 6, 2, df)
    keys, vals = pk.parts[3].view(np.uint64), pk.parts[4].view(np.float64)
    want = {}
    for r, n in ((refs[0], 2), (refs[1], 2)):
        for g in set(g for t in r for g in ngram_counts(t)):
            want[cider.pack_key(g)] = want.get(cider.pack_key(g), 0) + n
    assert keys.tolist() == sorted(want) and pk.L == math.log(4.0)
    assert all(v == math.log(4.0) - math.log(max(1.0, want[int(k)])) for k, v in zip(keys, vals))
    with pytest.raises(ValueError):
        cider.pack_host(refs, 5, 6, 2, None)                                  # 5 candidates are not 2 per image of 2 images
    with pytest.raises(ValueError):
        cider.pack_host([[[5, 0]], []], 2, 6, 1, None)                        # an image without references
    with pytest.raises(hip.BofiHipError, match="65534"):
        cider.pack_host([[[5, 65535, 0]]], 1, 6, 1, None)
    with pytest.raises(hip.BofiHipError, match="at most 64"):
        cider.pack_host([[[5, 0]]], 1, 65, 1, None)
    with pytest.raises(hip.BofiHipError, match="at most 64"):
        cider.pack_host([[[5] * 65]], 1, 6, 1, None)
