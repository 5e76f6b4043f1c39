"""ROUGE-L, host side: a float64 restatement of the pycocoevalcap package's ``Rouge`` (beta = 1.2) on id token lists, written here from the
rules alone -- a plain dynamic-programming longest common subsequence and the formula in its stated order --, a worked table, both token
rules, and the declaration of ``bofi_rouge_score``.  tests/test_gpu_rouge.py holds the device side against the same restatement."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BETA = 1.2

# ---------------------------------------------------------------- the float64 restatement (independent of boficap_amd)


def lcs_len(a, b):
    """Length of the longest common subsequence of two token lists (the textbook table)."""
    prev = [0] * (len(b) + 1)
    for x in a:
        cur = [0]
        for j, y in enumerate(b):
            cur.append(prev[j] + 1 if x == y else max(prev[j + 1], cur[j]))
        prev = cur
    return prev[len(b)]


def rouge_of(cand, refs, beta=BETA):
    """(score, [lcs_i], index of the reference that gives p, index of the one that gives r) of one candidate token list."""
    lcs = [lcs_len(cand, r) for r in refs]
    ps = [float(l) / float(len(cand)) if len(cand) > 0 and len(r) > 0 else 0.0 for l, r in zip(lcs, refs)]
    rs = [float(l) / float(len(r)) if len(cand) > 0 and len(r) > 0 else 0.0 for l, r in zip(lcs, refs)]
    p, r = max(ps), max(rs)
    b2 = beta * beta
    score = (1.0 + b2) * p * r / (r + b2 * p) if p != 0.0 and r != 0.0 else 0.0
    return score, lcs, ps.index(p), rs.index(r)                  # (list.index: the lowest index on ties)


def reward_ids(row):
    """array_to_str's rule: the row up to and including its first 0, or the whole row."""
    row = [int(t) for t in row]
    return row[: row.index(0) + 1] if 0 in row else row


def eval_ids(row):
    """decode_sequence's rule: the ids before the first id <= 0."""
    out = []
    for t in row:
        if int(t) <= 0:
            break
        out.append(int(t))
    return out


def restated_rouge(data_gts, seq, seq_per_img, rule="reward", cand_len=None):
    """Every row of seq [N, S] against its image's references: (scores float64 [N], lcs of every pair in candidate order, best int [N, 2])."""
    ids = reward_ids if rule == "reward" else eval_ids
    refs = [[ids(r) for r in g] for g in data_gts]
    scores, pairs, best = [], [], []
    for j, row in enumerate(np.asarray(seq).tolist()):
        cand = [int(t) for t in row[: int(cand_len[j])]] if cand_len is not None else ids(row)
        s, l, bp, br = rouge_of(cand, refs[j // seq_per_img])
        scores.append(s); pairs.extend(l); best.append([bp, br])
    return np.array(scores, dtype=np.float64), np.array(pairs, dtype=np.int64), np.array(best, dtype=np.int64).reshape(-1, 2)


# candidate, references, lcs per reference, p, r
WORKED = [
    ([1, 2, 3, 4], [[1, 9, 2, 8, 3, 7]], [3], 0.75, 0.5),
    ([5, 6, 7], [[5, 6, 7]], [3], 1.0, 1.0),                                    # identical rows
    ([5, 6, 7], [[8, 9], [10]], [0, 0], 0.0, 0.0),                              # disjoint rows
    ([1, 2, 3, 4], [[1, 2, 3, 9, 9, 9, 9, 9], [1, 2]], [3, 2], 0.75, 1.0),      # p from the first reference, r from the second
    ([], [[1, 2]], [0], 0.0, 0.0),                                              # an empty candidate
    ([1, 2], [[], [2]], [0, 1], 0.5, 1.0),                                      # an empty reference
    ([4, 3, 2, 1], [[1, 2, 3, 4]], [1], 0.25, 0.25),                            # a reversed row
]


def test_restatement_reproduces_the_worked_table():
    for cand, refs, lcs, p, r in WORKED:
        s, got, bp, br = rouge_of(cand, refs)
        assert got == lcs, (cand, got)
        want = (1 + BETA * BETA) * p * r / (r + BETA * BETA * p) if p and r else 0.0
        assert s == want, (cand, s, want)
    assert rouge_of(*WORKED[0][:2])[0] == pytest.approx(2.44 * 0.375 / (0.5 + 1.44 * 0.75), abs=1e-15)
    assert rouge_of(*WORKED[1][:2])[0] == pytest.approx(1.0, abs=1e-15)
    assert rouge_of(*WORKED[3][:2])[2:] == (0, 1)
    assert rouge_of([1, 2], [[1, 2], [1, 2]])[2:] == (0, 0)                     # a tie goes to the lowest index
    assert rouge_of([1, 2], [[1, 2, 7, 7], [1, 7]])[3] == 0                      # 2/4 and 1/2: the same fraction, the lowest index


def test_both_token_rules_on_a_row_with_an_inner_zero():
    row = [5, 6, 0, 7, 8]
    assert reward_ids(row) == [5, 6, 0] and eval_ids(row) == [5, 6]
    assert reward_ids([5, 6, 7]) == [5, 6, 7] and eval_ids([5, 6, 7]) == [5, 6, 7]
    assert reward_ids([0, 5]) == [0] and eval_ids([0, 5]) == []
    assert eval_ids([5, -1, 6]) == [5]
    gts = [[[5, 6, 0, 9, 9]]]
    s_reward, l_reward, _ = restated_rouge(gts, [row], 1, "reward")
    s_eval, l_eval, _ = restated_rouge(gts, [row], 1, "eval")
    assert l_reward.tolist() == [3] and l_eval.tolist() == [2] and s_reward[0] == 1.0 and s_eval[0] == 1.0
    # the package's module agrees with the restatement's rules
    from boficap_amd.cider import token_list
    from boficap_amd.rouge import eval_token_list, rule_lists
    for r in (row, [5, 6, 7], [0, 5], [5, -1, 6]):
        assert eval_token_list(r) == eval_ids(r)
        if min(r) >= 0:
            assert token_list(r) == reward_ids(r)
    assert rule_lists([np.array([[5, 6, 0, 7]])], "eval") == [[[5, 6]]] and rule_lists([np.array([[5, 6, 0, 7]])], "reward") == [[[5, 6, 0]]]


def test_scorer_checks_its_arguments():
    from boficap_amd.rouge import Rouge
    with pytest.raises(ValueError):
        Rouge(rule="words", device="cuda")
    with pytest.raises(ValueError):
        Rouge(beta=0.0, device="cuda")
    sc = Rouge(device="cuda")
    assert sc.rule == "reward" and sc.beta == 1.2 and sc.on_device
    with pytest.raises(AssertionError):
        sc.compute_score({0: ["5 6"], 1: ["5"]}, {0: ["5 6"]})                  # key sets differ
    with pytest.raises(AssertionError):
        sc.compute_score({0: ["5 6"]}, {0: ["5 6", "5"]})                       # two hypotheses
    with pytest.raises(AssertionError):
        sc.compute_score({0: []}, {0: ["5 6"]})                                 # no reference


def test_header_and_ctypes_table_declare_the_entry_point_alike():
    from boficap_amd import hip
    from boficap_amd.build import SOURCES
    header = open(os.path.join(ROOT, "include", "boficap_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    found = re.findall(r"\bint\s+bofi_rouge_score\s*\(([^;{]*?)\)\s*;", code, flags=re.S)
    assert len(found) == 1
    assert found[0].count(",") + 1 == len(hip.SIGNATURES["bofi_rouge_score"][1]) == 15
    assert "rouge.hip" in SOURCES and hip.ABI_VERSION == 5


def test_language_eval_reads_rows_and_strings_alike():
    from boficap_amd.lang_eval import KEYS, eval_reference_lists
    rows = [np.array([[5, 6, 0, 0], [7, 8, 9, 0]]), np.array([[4, 0, 3, 0]])]
    assert eval_reference_lists(rows) == [[[5, 6], [7, 8, 9]], [[4]]]
    assert eval_reference_lists([["5 6", "7 8 9"], ["4 0 3"]]) == [[[5, 6], [7, 8, 9]], [[4]]]
    assert KEYS == ("Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L", "CIDEr")
