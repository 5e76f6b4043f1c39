"""Oracle and average language scores of an image's n sampled captions (the reference's ``--eval_oracle 1``), host side: a float64 restatement
built from the restatements of BLEU, ROUGE-L and CIDEr-D that the tree already has, a table worked by hand, the argument checks of
``LanguageEval.evaluate_n`` and the declaration of ``bofi_oracle_stats``.  tests/test_gpu_oracle_scores.py holds the device side against the
same restatement."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_bleu import bleu_comps, bleu_of
from test_cider import cider_d, corpus_df
from test_rouge import eval_ids, rouge_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L", "CIDEr")

# ---------------------------------------------------------------- the float64 restatement (independent of boficap_amd)


def restated_oracle(gts, seq, n):
    """Rows seq [images * n, S], row m * n + i = sample i of image m, against the references gts[m] (rows of ids), tokens by the 'eval' rule on
    both sides.  Round i of the reference evaluates "sample i of every image" as a corpus and keeps the sentence-level scores; none of them
    depends on another image's candidate, and CIDEr's document frequencies are those of the images' references with L = log(images).
    Returns sentence [images, n, 6] (KEYS order), oracle = the maximum over the samples, avg = the sum in index order / n, pick = the first
    index of the maximum, the 12 set-level means and the BLEU counts comps [images, n, 10]."""
    refs = [[eval_ids(r) for r in np.asarray(g).tolist()] for g in gts]
    images = len(refs)
    rows = [eval_ids(r) for r in np.asarray(seq).tolist()]
    assert len(rows) == images * n
    df, L = corpus_df(refs), math.log(float(images))
    sentence = np.zeros((images, n, 6), dtype=np.float64)
    comps = np.zeros((images, n, 10), dtype=np.int64)
    for m in range(images):
        for i in range(n):
            cand = rows[m * n + i]
            c = bleu_comps(cand, refs[m])
            comps[m, i] = [c[0], c[1], *c[2], *c[3]]
            sentence[m, i] = bleu_of(*c) + [rouge_of(cand, refs[m])[0], cider_d(cand, refs[m], df, L)]
    oracle = np.zeros((images, 6), dtype=np.float64)
    avg = np.zeros((images, 6), dtype=np.float64)
    pick = np.zeros((images, 6), dtype=np.int64)
    for m in range(images):
        for q in range(6):
            vals = sentence[m, :, q].tolist()
            oracle[m, q] = max(vals)
            s = 0.0
            for v in vals:
                s += v
            avg[m, q] = s / n
            pick[m, q] = vals.index(max(vals))
    stats = {f"oracle_{k}": float(np.mean(oracle[:, q])) for q, k in enumerate(KEYS)}
    stats.update({f"avg_{k}": float(np.mean(avg[:, q])) for q, k in enumerate(KEYS)})
    return {"sentence": sentence, "oracle": oracle, "avg": avg, "pick": pick, "stats": stats, "comps": comps}


# ---------------------------------------------------------------- a table worked by hand: 2 images x 2 samples, 2 references each

TABLE_GTS = [np.array([[1, 2, 3, 4, 0], [1, 2, 5, 0, 0]]),        # image 0: A = 1 2 3 4, B = 1 2 5
             np.array([[6, 7, 8, 9, 0], [6, 8, 7, 0, 0]])]        # image 1: C = 6 7 8 9, D = 6 8 7
TABLE_SEQ = np.array([[1, 2, 3, 4, 0],                            # image 0, sample 0: equal to A
                      [0, 0, 0, 0, 0],                            # image 0, sample 1: empty
                      [6, 7, 0, 0, 0],                            # image 1, sample 0: shorter than its closest reference
                      [9, 8, 0, 0, 0]])                           # image 1, sample 1: two words of C in the wrong order


def test_table_worked_by_hand():
    out = restated_oracle(TABLE_GTS, TABLE_SEQ, 2)
    s = out["sentence"]
    near = lambda got, want: abs(got - want) <= 1e-8 * want        # BLEU: the hand values leave out the 1e-15 / 1e-9 constants (~1e-9 relative)
    e18, e72, rt = math.exp(-1.0 / 18.0), math.exp(-1.0 / 72.0), math.sqrt
    # No n-gram occurs in both images' references, so every document frequency is 1 and every weight is tf * (log 2 - log 1) = log 2 =: L
    # (every tf here is 1): a vector of u unique k-grams has norm sqrt(u) L, and L cancels in every cosine.
    #
    # image 0, sample 0 = 1 2 3 4 = A.  BLEU: T 4, closest reference length 4, guess = correct = [4, 3, 2, 1]: every order is a product of
    #   (c + 1e-15) / (c + 1e-9) ~ 1, and ratio = (4 + 1e-15) / (4 + 1e-9) < 1 adds the factor exp(1 - 1 / ratio) ~ exp(-2.5e-10): 1 up to the constants.
    assert out["comps"][0, 0].tolist() == [4, 4, 4, 3, 2, 1, 4, 3, 2, 1]
    assert all(near(s[0, 0, k], 1.0) and s[0, 0, k] < 1.0 for k in range(4))
    #   ROUGE: lcs(A) = 4, lcs(B) = 2 (1 2); p = 4/4, r = max(4/4, 2/3) = 1; 2.44 * 1 * 1 / (1 + 1.44 * 1) = 1.
    assert s[0, 0, 4] == 1.0
    #   CIDEr: the sample has 4, 3, 2, 1 unique k-grams and 3 bigrams (its "length").  Against A: cosine 1 in all four orders, lengths equal.
    #   Against B (3, 2, 1, 0 unique k-grams, length 2): shared unigrams 1, 2 -> 2 / (sqrt 4 sqrt 3) = 1 / sqrt 3; shared bigram (1 2) -> 1 / (sqrt 3 sqrt 2)
    #   = 1 / sqrt 6; no shared trigram; each times exp(-(3 - 2)^2 / 72).  10 x the mean over the 4 orders / 2 references.
    want = 10.0 * ((1.0 + e72 / rt(3.0)) + (1.0 + e72 / rt(6.0)) + 1.0 + 1.0) / 4.0 / 2.0
    assert abs(s[0, 0, 5] - want) <= 1e-12 and abs(want - 6.2150) < 1e-4
    # image 0, sample 1 is empty.  BLEU: T 0, closest reference length 3 (B), every order (1e-15 / 1e-9)^k > 0, but ratio = 1e-15 / 3 and
    #   exp(1 - 3e15) = 0.  ROUGE: p = r = 0.  CIDEr: no n-gram.  All six are exactly 0.
    assert out["comps"][0, 1].tolist() == [0, 3, 0, 0, 0, 0, 0, 0, 0, 0]
    assert s[0, 1].tolist() == [0.0] * 6
    # image 1, sample 0 = 6 7.  BLEU: T 2; |D| = 3 is closer than |C| = 4; guess [2, 1, 0, 0]; 6 and 7 occur, (6 7) occurs in C: correct [2, 1, 0, 0].
    #   Products: ~1, ~1, 1e-15 / 1e-9 = 1e-6, 1e-12 -> roots 1, 1, 1e-2, 1e-3; ratio 2/3 < 1: the brevity factor exp(1 - 3/2) on every order.
    assert out["comps"][1, 0].tolist() == [2, 3, 2, 1, 0, 0, 2, 1, 0, 0]
    bp = math.exp(-0.5)
    assert near(s[1, 0, 0], bp) and near(s[1, 0, 1], bp) and near(s[1, 0, 2], 1e-2 * bp) and near(s[1, 0, 3], 1e-3 * bp)
    #   ROUGE: lcs(C) = 2, lcs(D) = 2 (6 . 7); p = 2/2, r = max(2/4, 2/3): 2.44 * (2/3) / (2/3 + 1.44).
    assert abs(s[1, 0, 4] - 2.44 * (2.0 / 3.0) / (2.0 / 3.0 + 1.44)) <= 1e-15
    #   CIDEr: the sample has 2 unigrams, 1 bigram (length 1).  C (4, 3, 2, 1 k-grams, length 3): unigrams 2 / (sqrt 2 sqrt 4) = 1 / sqrt 2, bigram (6 7)
    #   1 / sqrt 3, times exp(-(1 - 3)^2 / 72) = exp(-1/18).  D (3, 2, 1 k-grams, length 2): unigrams 2 / (sqrt 2 sqrt 3) = 2 / sqrt 6, no bigram, times exp(-1/72).
    want = 10.0 * ((e18 / rt(2.0) + 2.0 * e72 / rt(6.0)) + e18 / rt(3.0)) / 4.0 / 2.0
    assert abs(s[1, 0, 5] - want) <= 1e-12 and abs(want - 2.5254) < 1e-4
    # image 1, sample 1 = 9 8.  BLEU: T 2, reference length 3, correct [2, 0, 0, 0]: BLEU-1 is sample 0's to the bit (the same counts), the
    #   higher orders are roots of 1e-15, 1e-21, 1e-27: sqrt(1e-15), 1e-7, 1e-27^(1/4), times the brevity factor.
    assert out["comps"][1, 1].tolist() == [2, 3, 2, 1, 0, 0, 2, 0, 0, 0]
    assert s[1, 1, 0] == s[1, 0, 0] and near(s[1, 1, 1], rt(1e-15) * bp) and near(s[1, 1, 2], 1e-7 * bp) and near(s[1, 1, 3], 1e-27 ** 0.25 * bp)
    #   ROUGE: lcs 1 with either; p = 1/2, r = max(1/4, 1/3): 2.44 * (1/2) (1/3) / (1/3 + 1.44 / 2).
    assert abs(s[1, 1, 4] - 2.44 * (1.0 / 6.0) / (1.0 / 3.0 + 0.72)) <= 1e-15
    #   CIDEr: C shares the unigrams 9, 8: 1 / sqrt 2, exp(-1/18); D shares 8: 1 / (sqrt 2 sqrt 3), exp(-1/72); no bigram.
    want = 10.0 * (e18 / rt(2.0) + e72 / rt(6.0)) / 4.0 / 2.0
    assert abs(s[1, 1, 5] - want) <= 1e-12
    # the reduction: image 0's oracle is sample 0 and its average half of it; image 1's BLEU-1 is a tie, which goes to the lower index
    assert out["pick"].tolist() == [[0] * 6, [0] * 6]
    assert np.array_equal(out["oracle"], s[:, 0, :]) and np.array_equal(out["avg"][0], s[0, 0] / 2.0)
    assert np.array_equal(out["avg"][1], (s[1, 0] + s[1, 1]) / 2.0) and out["avg"][1, 0] == out["oracle"][1, 0]
    assert list(out["stats"]) == [f"oracle_{k}" for k in KEYS] + [f"avg_{k}" for k in KEYS]
    assert out["stats"]["oracle_ROUGE_L"] == (s[0, 0, 4] + s[1, 0, 4]) / 2.0
    # the samples swapped within each image: the same oracle, the pick moves, BLEU-1's tie stays at index 0
    swapped = restated_oracle(TABLE_GTS, TABLE_SEQ[[1, 0, 3, 2]], 2)
    assert np.array_equal(swapped["oracle"], out["oracle"]) and swapped["pick"].tolist() == [[1] * 6, [0] + [1] * 5]


def test_restatement_at_one_sample_is_the_sentence_scores():
    out = restated_oracle(TABLE_GTS, TABLE_SEQ[[0, 2]], 1)
    assert np.array_equal(out["oracle"], out["sentence"][:, 0]) and np.array_equal(out["avg"], out["oracle"]) and not out["pick"].any()


# ---------------------------------------------------------------- boficap_amd.lang_eval, host side


def test_evaluate_n_checks_its_arguments():
    """The checks run before any device work: an object without references on a device is enough."""
    from boficap_amd.lang_eval import MAX_SAMPLES, LanguageEval
    from boficap_amd.cider import MAX_TOKENS
    assert MAX_SAMPLES == 64 and MAX_TOKENS == 64
    ev = LanguageEval.__new__(LanguageEval)
    ev.images = 4
    with pytest.raises(ValueError, match="rows"):
        ev.evaluate_n(np.ones((10, 8), dtype=np.int64), 3)             # 10 rows are not 4 x 3
    with pytest.raises(ValueError, match="rows"):
        ev.evaluate_n(np.ones((4, 8), dtype=np.int64), 2)
    with pytest.raises(ValueError, match="samples"):
        ev.evaluate_n(np.ones((0, 8), dtype=np.int64), 0)
    with pytest.raises(ValueError, match="samples"):
        ev.evaluate_n(np.ones((260, 8), dtype=np.int64), 65)
    with pytest.raises(ValueError, match="samples"):
        ev.evaluate_n(np.ones((8, 8), dtype=np.int64), 2.5)
    with pytest.raises(ValueError, match="at most 64"):
        ev.evaluate_n(np.ones((8, 65), dtype=np.int64), 2)
    with pytest.raises(ValueError):
        ev.evaluate_n(np.ones(8, dtype=np.int64), 2)                   # not rows
    assert ev.check_n(256, 64, 64) == 64 and ev.check_n(4, 1, 1) == 1


def test_header_and_ctypes_table_declare_the_entry_point_alike():
    from boficap_amd import hip
    from boficap_amd.build import SOURCES
    header = open(os.path.join(ROOT, "include", "boficap_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    found = re.findall(r"\bint\s+bofi_oracle_stats\s*\(([^;{]*?)\)\s*;", code, flags=re.S)
    assert len(found) == 1
    assert found[0].count(",") + 1 == len(hip.SIGNATURES["bofi_oracle_stats"][1]) == 9
    assert "oracle.hip" in SOURCES and hip.ABI_VERSION == 5
    assert "#pragma clang fp contract(off)" in open(os.path.join(ROOT, "boficap_amd", "csrc", "oracle.hip")).read()


def test_tools_eval_names_the_options_the_oracle_needs():
    """--eval_oracle 1 without --language_eval 1 --sample_n N is an argument error, before any model or device work."""
    tool = os.path.join(ROOT, "tools", "eval.py")
    for extra in (["--sample_n", "3"], ["--language_eval", "1", "--input_label_npz", "labels.npz"]):
        out = subprocess.run([sys.executable, tool, "--eval_oracle", "1"] + extra, capture_output=True, text=True, timeout=120)
        assert out.returncode == 2 and "--language_eval 1" in out.stderr and "--sample_n" in out.stderr, out.stderr[-500:]
