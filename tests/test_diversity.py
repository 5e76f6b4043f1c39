"""Diversity of an image's n sampled captions, host side: a float64 restatement of self-CIDEr (``Cider.my_self_cider`` of the pyciderevalcap
package with the ``get_div`` of captioning/utils/rewards.py:119-139), Div-1 / Div-2 and mBLEU-1..4, written here from the rules alone, with
examples worked by hand, and the declaration of ``bofi_diversity_score``.  tests/test_gpu_diversity.py holds the device side against the
same restatement."""
import math
import os
import re
import warnings

import numpy as np
import pytest

from test_cider import ngram_counts
from test_rouge import eval_ids, reward_ids

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY, SMALL = 1e-15, 1e-9

# ---------------------------------------------------------------- the float64 restatement (independent of boficap_amd)


def record(tokens, df, L):
    """Per order k = 0..3: {k-gram: tf * (L - log max(1, df))} and the vector's norm (sums exactly rounded: math.fsum)."""
    vec = [dict() for _ in range(4)]
    for g, tf in ngram_counts(tokens).items():
        vec[len(g) - 1][g] = float(tf) * (L - math.log(max(1.0, float(df.get(g, 0)))))
    return vec, [math.sqrt(math.fsum(w * w for w in v.values())) for v in vec]


def self_cider_matrix(samples, df, L):
    """M[i][j] = 1/4 sum_k cos_k(i, j) over the token lists of one image; plain CIDEr: no clipping, no length penalty."""
    recs = [record(s, df, L) for s in samples]
    n = len(samples)
    M = np.zeros((n, n), dtype=np.float64)
    for i in range(n):
        for j in range(n):
            (vi, ni), (vj, nj) = recs[i], recs[j]
            cos = []
            for k in range(4):
                dot = math.fsum(w * vj[k][g] for g, w in vi[k].items() if g in vj[k])
                cos.append(dot / (ni[k] * nj[k]) if ni[k] != 0.0 and nj[k] != 0.0 else 0.0)
            M[i, j] = (cos[0] + cos[1] + cos[2] + cos[3]) / 4.0
    return M


def div_of_eigenvalues(M):
    """rewards.py:132-135: eigenvalues clipped below at 0, -log(sqrt(l_max) / sum sqrt(l)) / log n; NaN where all clip to 0."""
    eig = np.clip(np.linalg.eigvalsh(np.asarray(M, dtype=np.float64)), 0, None)
    with np.errstate(invalid="ignore", divide="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return float(-np.log(np.sqrt(eig[-1]) / np.sqrt(eig).sum()) / np.log(len(eig)))


def div_counts(samples):
    """(distinct unigrams, distinct bigrams, tokens) over the token lists of one image."""
    uni = set(g for s in samples for g in ngram_counts(s, 1))
    both = set(g for s in samples for g in ngram_counts(s, 2))
    return len(uni), len(both) - len(uni), sum(len(s) for s in samples)


def bleu_comps(cand, refs):
    """(T, reflen, guess[4], correct[4]) of one candidate against its references: Bleu(4), option 'closest' (a tie goes to the shorter)."""
    T = len(cand)
    reflen = min((abs(len(r) - T), len(r)) for r in refs)[1]
    cc, rc = ngram_counts(cand), [ngram_counts(r) for r in refs]
    correct = [0] * 4
    for g, c in cc.items():
        correct[len(g) - 1] += min(c, max(r.get(g, 0) for r in rc))
    return [T, reflen] + [max(0, T - k) for k in range(4)] + correct


def bleu_of(testlen, reflen, guess, correct):
    """BLEU-1..4 of summed counts (bleu_scorer.py's compute_score)."""
    out, b = [], 1.0
    for k in range(4):
        b *= float(correct[k] + TINY) / (guess[k] + SMALL)
        out.append(b ** (1.0 / (k + 1)))
    ratio = (testlen + TINY) / (reflen + SMALL)
    if ratio < 1:
        out = [x * math.exp(1 - 1 / ratio) for x in out]
    return out


def restated_diversity(seq, n, df, L, rule="reward"):
    """Everything of rows seq [images * n, S]: M [images, n, n], score [images], div [images, 3], comps [images * n, 10] and the statistics."""
    ids = reward_ids if rule == "reward" else eval_ids
    if n < 2:
        raise ValueError("n >= 2")
    rows = [ids(r) for r in np.asarray(seq).tolist()]
    images = len(rows) // n
    M, score, div, comps = [], [], [], []
    for b in range(images):
        samples = rows[b * n:(b + 1) * n]
        M.append(self_cider_matrix(samples, df, L))
        score.append(div_of_eigenvalues(M[-1]))
        div.append(div_counts(samples))
        comps.extend(bleu_comps(samples[i], samples[:i] + samples[i + 1:]) for i in range(n))
    div, comps = np.array(div, dtype=np.int64).reshape(images, 3), np.array(comps, dtype=np.int64).reshape(images * n, 10)
    stats = {}
    for k in range(2):
        stats[f"Div-{k + 1}"] = float(np.mean([d[k] / d[2] if d[2] > 0 else 0.0 for d in div.tolist()]))
    runs = []
    for i in range(n):
        tot = comps.reshape(images, n, 10)[:, i, :].sum(0).tolist()
        runs.append(bleu_of(tot[0], tot[1], tot[2:6], tot[6:]))
    for k in range(4):
        stats[f"mBLEU_{k + 1}"] = float(np.mean(np.array([r[k] for r in runs])))
    sc = np.array(score, dtype=np.float64)
    stats["self_cider"] = float(np.mean(sc[~np.isnan(sc)])) if (~np.isnan(sc)).any() else float("nan")
    return {"M": np.array(M), "score": sc, "div": div, "comps": comps, "stats": stats}


# ---------------------------------------------------------------- worked examples

L16 = math.log(16.0)


def test_identical_captions_give_rank_one_and_score_zero():
    for n in (2, 5, 16):
        M = self_cider_matrix([[3, 4, 5, 6, 0]] * n, {(3,): 4, (4, 5): 2}, L16)
        assert np.abs(M - 1.0).max() <= 1e-15
        assert np.linalg.matrix_rank(M, tol=1e-12) == 1
        assert abs(div_of_eigenvalues(M)) <= 1e-6                     # exact arithmetic: eigenvalues (n, 0, ..), sqrt(n) / sqrt(n) -> 0


def test_disjoint_captions_give_the_identity_and_score_one():
    for n in (2, 5, 16):
        samples = [[10 * i + 1, 10 * i + 2, 10 * i + 3, 10 * i + 4] for i in range(n)]
        M = self_cider_matrix(samples, {}, L16)
        assert np.abs(M - np.eye(n)).max() <= 1e-15
        assert abs(div_of_eigenvalues(M) - 1.0) <= 1e-12              # n eigenvalues 1: -log(1 / n) / log n


def test_two_captions_with_one_shared_bigram():
    # A = 1 2 3 4, B = 5 1 2 6 share the unigrams 1, 2 and the bigram (1 2).  No df entry: every weight is L.
    #   order 1: 4 unigrams each, norm 2 L, dot 2 L^2 -> 1/2;  order 2: 3 bigrams each, norm sqrt(3) L, dot L^2 -> 1/3;  orders 3, 4: 0
    A, B = [1, 2, 3, 4], [5, 1, 2, 6]
    M = self_cider_matrix([A, B], {}, L16)
    a = (0.5 + 1.0 / 3.0) / 4.0
    assert abs(M[0, 1] - a) <= 1e-15 and M[0, 1] == M[1, 0] and abs(M[0, 0] - 1) <= 1e-15 and abs(M[1, 1] - 1) <= 1e-15
    # eigenvalues of [[1, a], [a, 1]]: 1 + a and 1 - a
    want = -math.log(math.sqrt(1 + a) / (math.sqrt(1 + a) + math.sqrt(1 - a))) / math.log(2.0)
    assert abs(div_of_eigenvalues(M) - want) <= 1e-14
    # the bigram (1 2) in 4 of 16 images: its weight is L - log 4 = L / 2;  order 2: norm^2 = (1/4 + 2) L^2, dot L^2 / 4 -> 1/9
    M = self_cider_matrix([A, B], {(1, 2): 4}, L16)
    assert abs(M[0, 1] - (0.5 + 1.0 / 9.0) / 4.0) <= 1e-15
    # a term frequency: C = 1 1 2 has the unigram 1 twice (weight 2 L) -> |C|_1 = sqrt(5) L; against D = 1 3: dot 2 L^2, |D|_1 = sqrt(2) L
    M = self_cider_matrix([[1, 1, 2], [1, 3]], {}, L16)
    assert abs(M[0, 1] - (2.0 / math.sqrt(10.0)) / 4.0) <= 1e-15
    # rows of one and of no token: the missing orders have norm 0 and add 0
    M = self_cider_matrix([[7], [7, 8], []], {}, L16)
    assert abs(M[0, 0] - 0.25) <= 1e-15 and abs(M[1, 1] - 0.5) <= 1e-15 and abs(M[0, 1] - 0.25 / math.sqrt(2.0)) <= 1e-15
    assert M[2].tolist() == [0.0, 0.0, 0.0]
    assert math.isnan(div_of_eigenvalues(np.zeros((3, 3))))          # every sample empty: 0 / 0


def test_div_and_mbleu_tables():
    assert div_counts([[1, 2, 3], [1, 2, 4], [5]]) == (5, 3, 7)        # {1 2 3 4 5}, {(1 2) (2 3) (2 4)}, 3 + 3 + 1 tokens
    assert div_counts([[1, 1, 1], [1, 1]]) == (1, 1, 5)
    assert div_counts([[], []]) == (0, 0, 0)
    A, B, C = [1, 2, 3, 4], [1, 2, 3, 5], [1, 2]
    assert bleu_comps(A, [B, C]) == [4, 4, 4, 3, 2, 1, 3, 2, 1, 0]
    assert bleu_comps(C, [A, B]) == [2, 4, 2, 1, 0, 0, 2, 1, 0, 0]
    assert bleu_comps([1, 2, 3], [[1, 2], [1, 2, 3, 4]])[1] == 2       # lengths 2 and 4 are equally close to 3: the shorter
    assert bleu_comps([1, 1, 1], [[1, 1], [1]])[6] == 2                # clipped at the largest count among the references
    assert bleu_comps([], [[1, 2]]) == [0, 2, 0, 0, 0, 0, 0, 0, 0, 0]
    seq = np.array([[1, 2, 3, 4, 0], [1, 2, 3, 5, 0], [1, 2, 0, 0, 0], [6, 7, 0, 0, 0], [6, 7, 0, 0, 0], [6, 8, 9, 0, 0]])
    out = restated_diversity(seq, 3, {}, L16, rule="eval")
    assert out["div"].tolist() == [[5, 4, 10], [4, 3, 7]]                # (1 2) (2 3) (3 4) (3 5);  (6 7) (6 8) (8 9)
    assert out["comps"][0].tolist() == [4, 4, 4, 3, 2, 1, 3, 2, 1, 0] and out["comps"][3].tolist() == [2, 2, 2, 1, 0, 0, 2, 1, 0, 0]
    assert out["stats"]["Div-1"] == (5 / 10 + 4 / 7) / 2 and out["stats"]["Div-2"] == (4 / 10 + 3 / 7) / 2
    # mBLEU-1: position 0 holds A (3 of 4 unigrams) and 6 7 (2 of 2), lengths 6 against closest lengths 4 + 2: no brevity penalty
    tot = (out["comps"][0] + out["comps"][3]).tolist()
    assert tot[:2] == [6, 6] and abs(bleu_of(tot[0], tot[1], tot[2:6], tot[6:])[0] - 5 / 6) <= 1e-9
    assert 0 < out["stats"]["mBLEU_4"] < out["stats"]["mBLEU_1"] < 1
    # the 'reward' rule keeps the terminating 0 as a token
    assert restated_diversity(seq, 3, {}, L16, rule="reward")["div"].tolist() == [[6, 7, 13], [5, 5, 10]]
    with pytest.raises(ValueError):
        restated_diversity(seq, 1, {}, L16)


# ---------------------------------------------------------------- boficap_amd.diversity, host side


def test_host_statistics_equal_the_restatement():
    from boficap_amd import diversity
    rng = np.random.default_rng(3)
    seq = rng.integers(1, 9, (12, 10))
    for row in seq:
        row[int(rng.integers(0, 11)):] = 0
    want = restated_diversity(seq, 4, {}, L16, rule="eval")
    stats, d1, d2 = diversity.stats_of_counts(want["div"], want["comps"], 4)
    for k in ("Div-1", "Div-2", "mBLEU_1", "mBLEU_2", "mBLEU_3", "mBLEU_4"):
        assert abs(stats[k] - want["stats"][k]) <= 1e-15, k
    assert d1.shape == (3,) and d2.shape == (3,)
    assert diversity.KEYS == ("Div-1", "Div-2", "mBLEU_1", "mBLEU_2", "mBLEU_3", "mBLEU_4", "self_cider")


def test_scorer_checks_its_arguments():
    from boficap_amd import diversity
    with pytest.raises(ValueError, match="corpus"):
        diversity.SelfCider("corpus", device="cuda")
    with pytest.raises(ValueError, match="corpus"):
        diversity.DiversityEval("corpus", device="cuda")
    with pytest.raises(ValueError):
        diversity.check_shape(10, 20, 1)                                # n >= 2
    with pytest.raises(ValueError):
        diversity.check_shape(34, 20, 17)                               # n <= 16
    with pytest.raises(ValueError):
        diversity.check_shape(10, 20, 3)                                # rows not n per image
    with pytest.raises(ValueError):
        diversity.check_shape(10, 65, 2)                                # rows of more than 64 ids
    assert diversity.check_shape(10, 20, 5) == 2


def test_structure_loss_takes_an_extra_advantage():
    import torch
    from boficap_amd import xe
    g = torch.Generator().manual_seed(0)
    lp = torch.log_softmax(torch.randn(6, 5, 11, generator=g), dim=2)
    seq = torch.randint(1, 11, (6, 5), generator=g)
    seq[1, 3:] = 0
    scores = torch.rand(6, generator=g)
    base, reward = xe.structure_loss("new_self_critical", lp, seq, scores, 3)
    same, _ = xe.structure_loss("new_self_critical", lp, seq, scores, 3, extra_advantage=None)
    assert torch.equal(base, same)
    extra = torch.tensor([[0.25], [0.75]]).expand(2, 3)
    got, reward2 = xe.structure_loss("new_self_critical", lp, seq, scores, 3, extra_advantage=extra)
    sc = scores.view(2, 3)
    adv = sc - (sc.sum(1, keepdim=True) - sc) / 2 + extra            # added after the baseline: it does not cancel
    mask = torch.cat([torch.ones(6, 1), (seq > 0).float()[:, :-1]], 1)
    want = (-lp.gather(2, seq.unsqueeze(2)).squeeze(2) * mask * adv.reshape(-1, 1)).sum() / mask.sum()
    assert abs(float(got) - float(want)) <= 1e-6 and abs(float(got) - float(base)) > 1e-3 and torch.equal(reward, reward2)
    other, _ = xe.structure_loss("seqnll", lp, seq, scores, 3, extra_advantage=extra)      # the other types ignore it (losses.py:157-171)
    assert torch.equal(other, xe.structure_loss("seqnll", lp, seq, scores, 3)[0])


def test_header_and_ctypes_table_declare_the_entry_point_alike():
    from boficap_amd import hip
    from boficap_amd.build import SOURCES
    header = open(os.path.join(ROOT, "include", "boficap_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    found = re.findall(r"\bint\s+bofi_diversity_score\s*\(([^;{]*?)\)\s*;", code, flags=re.S)
    assert len(found) == 1
    assert found[0].count(",") + 1 == len(hip.SIGNATURES["bofi_diversity_score"][1]) == 16
    found = re.findall(r"\bint64_t\s+bofi_diversity_workspace\s*\(([^;{]*?)\)\s*;", code, flags=re.S)
    assert len(found) == 1 and found[0].count(",") + 1 == len(hip.SIGNATURES["bofi_diversity_workspace"][1]) == 3
    assert "diversity.hip" in SOURCES and "cider.hip" in SOURCES and hip.ABI_VERSION == 5
    csrc = os.path.join(ROOT, "boficap_amd", "csrc")
    for src in ("cider.hip", "diversity.hip"):                          # both build their records with the one header
        assert '#include "bofi_record.h"' in open(os.path.join(csrc, src)).read()
    assert "build_record" in open(os.path.join(csrc, "bofi_record.h")).read()
