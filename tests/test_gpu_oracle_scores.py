"""Oracle and average language scores of sampled captions on the MI355X (boficap_amd/csrc/oracle.hip, ``LanguageEval.evaluate_n``) against the
one-candidate path the tree already has, against the host formula on the device's own counts, and against the float64 restatement of
tests/test_oracle_scores.py; ``eval_split`` with ``eval_oracle`` and ``tools/eval.py --eval_oracle 1``."""
import json
import math
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import record_parity
from test_cider import synthetic_corpus, write_df_pickle
from test_oracle_scores import KEYS, restated_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 16
SEEDS = {(5, 1): 0, (5, 2): 6, (7, 5): 12, (3, 64): 1, (130, 3): 0}      # chosen on the host with the restatement: see clear_winners and the (7, 5) conditions
CASES = [(5, 1), (5, 2), (7, 5), (3, 64), (130, 3)]               # (3, 64): the full wavefront; (130, 3): several workgroups and a tail
DIV_KEYS = ["Div-1", "Div-2", "mBLEU_1", "mBLEU_2", "mBLEU_3", "mBLEU_4", "self_cider"]
NEW_KEYS = [f"oracle_{k}" for k in KEYS] + [f"avg_{k}" for k in KEYS]
_CASE = {}


def build(images, n, seed=None):
    """1-7 references per image of 1-17 ids, rows of S = 16 ids, all ids out of 1..12 so that n-grams repeat.  An image's references leave two
    of the twelve ids out.  A sample is a reference of its image with some ids redrawn and a new length, or ids drawn afresh, then padding, and
    holds one of the two ids its references lack: with so few ids nearly every sample would otherwise match all its unigrams, and BLEU-1 would
    differ between samples only through the 1e-9 of its denominators.  From three samples per image on, one sample of every image is a copy of a
    reference, so that an image of many samples has one best caption and not several near-equal ones; in the (3, 64) batch it occurs twice (a
    tie between identical rows across the wavefront).  The (7, 5) batch holds the rows placed by hand instead."""
    seed = SEEDS[(images, n)] if seed is None else seed
    rng = np.random.default_rng(1000 * seed + 10 * images + n)
    gts, lacks = [], []
    for _ in range(images):
        out = rng.choice(np.arange(1, 13), 2, replace=False)
        ids = np.setdiff1d(np.arange(1, 13), out)
        g = ids[rng.integers(0, 10, (int(rng.integers(1, 8)), 18))]
        for row in g:
            row[int(rng.integers(1, 18)):] = 0
        gts.append(g)
        lacks.append(out)
    seq = rng.integers(1, 13, (images * n, S))
    for j, row in enumerate(seq):
        g = gts[j // n]
        if rng.random() < 0.6:
            row[:] = g[int(rng.integers(0, len(g))), :S]
            swap = (rng.random(S) < 0.3) | (row == 0)
            row[swap] = rng.integers(1, 13, int(swap.sum()))
        T = int(rng.integers(1, S + 1))
        row[T:] = 0
        row[int(rng.integers(0, T))] = lacks[j // n][int(rng.integers(0, 2))]
    if (images, n) == (7, 5):
        seq[0:5] = seq[0]                                          # image 0: five identical samples, a tie: every pick 0
        seq[5 + 2, 0] = 0                                          # image 1: one empty sample
        gts[2][0, 12:] = 0
        seq[10] = gts[2][0, :S]                                    # image 2: the first sample is a copy of a reference
        seq[15 + 1, 5:] = rng.integers(1, 13, S - 5)
        seq[15 + 1, 4] = 0                                         # image 3: a row with an inner 0; what follows it is not read
        seq[20] = np.arange(S) % 12 + 1                            # image 4: a row without any 0
    elif n >= 3:
        for m in range(images):
            g = gts[m]
            g[0, S:] = 0                                           # (a reference of 17 ids would not fit a row)
            at = rng.permutation(n)[:2]
            seq[m * n + at[0]] = g[0, :S]
            if n == 64:
                seq[m * n + at[1]] = g[0, :S]
    return gts, seq


def case(images, n):
    """(references, rows, restatement), computed once per shape, shared, left unchanged."""
    if (images, n) not in _CASE:
        gts, seq = build(images, n)
        _CASE[(images, n)] = (gts, seq, restated_oracle(gts, seq, n))
    return _CASE[(images, n)]


def clear_winners(seq, want, n):
    """True if no pick of the restatement can flip on a difference below the bars: for every image and metric, each sample either attains the
    maximum exactly and is the same row as the first that does, or lies more than 1e-6 below it."""
    sent = want["sentence"]
    for m in range(sent.shape[0]):
        for q in range(6):
            first = int(want["pick"][m, q])
            for i in range(n):
                if sent[m, i, q] == sent[m, first, q]:
                    if not np.array_equal(seq[m * n + i], seq[m * n + first]):
                        return False
                elif not sent[m, i, q] < sent[m, first, q] - 1e-6:
                    return False
    return True


def bits(t):
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


@pytest.mark.parametrize("images,n", CASES)
def test_kernel_and_reduction(images, n):
    """Bars: the project's bars for the same kernels -- BLEU and ROUGE-L 1e-15, CIDEr 1e-9.  Measured on the MI355X over the five shapes
    (profiles/r09_parity_errors.json): BLEU-1..4 against the host formula on the device's counts <= 1.1e-16 in every order (1, 2 and 3 go
    through pow with the exponents 1, 1/2, 1/3); against the restatement BLEU <= 1.1e-16, ROUGE-L 0, CIDEr <= 1.8e-15."""
    from boficap_amd.bleu import bleu_of_comps
    from boficap_amd.lang_eval import LanguageEval
    gts, seq_h, want = case(images, n)
    assert clear_winners(seq_h, want, n)
    if (images, n) == (7, 5):                                      # the data keeps exercising what it was chosen for
        assert any(len(set(want["pick"][m].tolist())) > 1 for m in range(images))                        # a pick that differs between two metrics
        assert any((want["oracle"][m] > want["avg"][m]).all() for m in range(images))                   # oracle > avg for all six metrics
        assert not want["pick"][0].any() and (want["sentence"][1, 2] == 0).all() and want["sentence"][2, 0, 4] == 1.0
    ev = LanguageEval(gts, "cuda")
    seq = torch.from_numpy(seq_h).cuda()
    sent_d, stats_d, pick_d, comps_d = ev._launch_n(seq, n)
    out = ev.evaluate_n(seq, n)
    per = out["per_image"]
    assert list(out) == NEW_KEYS + ["per_image"] and list(per) == ["sentence", "oracle", "avg", "pick"]
    assert per["sentence"].shape == (images, n, 6) and per["oracle"].shape == per["avg"].shape == per["pick"].shape == (images, 6)
    assert np.array_equal(per["sentence"].reshape(-1, 6), sent_d.cpu().numpy()) and np.array_equal(per["pick"], pick_d.cpu().numpy())
    # 1. the one-candidate path on the strided rows: the same blocks computing the same thing, bit for bit
    for i in range(n):
        rows = seq[i::n].contiguous()
        cl = ((rows <= 0).cumsum(1) == 0).sum(1).to(torch.int32)
        _, cider, comps = ev.reward._launch(None, rows, cl, 1, True, True, records=ev.records)
        rouge, _, _ = ev.rouge._launch(ev.pk, rows, cl, 1)
        assert torch.equal(comps, comps_d[i::n]), i
        assert torch.equal(bits(cider), bits(sent_d[i::n, 5])) and torch.equal(bits(rouge), bits(sent_d[i::n, 4])), i
    # 2. BLEU-1..4 against the host formula on the device's counts
    comps = comps_d.cpu().numpy()
    host = np.array([bleu_of_comps(int(c[0]), int(c[1]), [int(v) for v in c[2:6]], [int(v) for v in c[6:]]) for c in comps]).reshape(images, n, 4)
    err = np.abs(per["sentence"][:, :, :4] - host).reshape(-1, 4).max(0)
    print(f"images {images} n {n}: |BLEU-k - host formula| {err.tolist()}")
    record_parity(f"oracle_bleu_formula_i{images}_n{n}", float(err.max()), 1e-15)
    assert err.max() <= 1e-15, err
    # 3. the reduction, bit for bit, from the device's own sentence scores
    for m in range(images):
        for q in range(6):
            vals, total = per["sentence"][m, :, q].tolist(), 0.0
            for v in vals:                                         # left to right (the built-in sum of floats compensates its rounding)
                total += v
            assert per["oracle"][m, q] == max(vals) and per["avg"][m, q] == total / n and per["pick"][m, q] == vals.index(max(vals)), (m, q)
    for q, k in enumerate(KEYS):
        assert out[f"oracle_{k}"] == float(np.mean(per["oracle"][:, q])) and out[f"avg_{k}"] == float(np.mean(per["avg"][:, q])), k
    # 4. the restatement
    assert np.array_equal(comps.reshape(images, n, 10), want["comps"])
    for name, cols, bar in (("bleu", slice(0, 4), 1e-15), ("rouge", slice(4, 5), 1e-15), ("cider", slice(5, 6), 1e-9)):
        e = max(float(np.abs(per[a][..., cols] - want[a][..., cols]).max()) for a in ("sentence", "oracle", "avg"))
        print(f"images {images} n {n}: |{name} - restatement| {e:.3e}")
        record_parity(f"oracle_{name}_i{images}_n{n}", e, bar)
        assert e <= bar, (name, e)
    assert np.array_equal(per["pick"], want["pick"])
    for k in NEW_KEYS:
        assert abs(out[k] - want["stats"][k]) <= (1e-9 if k.endswith("CIDEr") else 1e-15), k
    again = ev._launch_n(seq, n)                                   # fixed orders: bit-identical run to run
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(again, (sent_d, stats_d, pick_d, comps_d)))
    host_ids = ev.evaluate_n(seq_h.astype(np.int32), n)            # ids from the host, another integer type
    assert all(host_ids[k] == out[k] for k in NEW_KEYS)


def test_nan_row():
    """An id above 65 534 has no key: that row's CIDEr is NaN, and so are its image's oracle and average; the set's means skip that image."""
    from boficap_amd.lang_eval import LanguageEval
    gts, seq_h, _ = case(5, 2)
    ev = LanguageEval(gts, "cuda")
    seq = torch.from_numpy(seq_h).cuda()
    clean = ev.evaluate_n(seq, 2)
    seq[3, 1] = 70000                                              # image 1, sample 1
    seq[3, 2] = 5                                                  # (read: no 0 before the id)
    out = ev.evaluate_n(seq, 2)
    per = out["per_image"]
    assert math.isnan(per["oracle"][1, 5]) and math.isnan(per["avg"][1, 5]) and per["pick"][1, 5] == -1 and math.isnan(per["sentence"][1, 1, 5])
    assert np.isfinite(per["oracle"][1, :5]).all() and np.isfinite(per["avg"][1, :5]).all() and (per["pick"][1, :5] >= 0).all()
    others = [0, 2, 3, 4]
    assert np.isfinite(per["oracle"][others]).all() and np.array_equal(per["oracle"][others], clean["per_image"]["oracle"][others])
    assert out["oracle_CIDEr"] == float(np.mean(per["oracle"][others, 5])) and out["avg_CIDEr"] == float(np.mean(per["avg"][others, 5]))
    assert out["oracle_ROUGE_L"] == float(np.mean(per["oracle"][:, 4]))


def test_one_sample_is_the_sentence_scores():
    from boficap_amd.lang_eval import LanguageEval
    gts, seq_h, _ = case(5, 1)
    ev = LanguageEval(gts, "cuda")
    out = ev.evaluate_n(seq_h, 1)
    per = out["per_image"]
    assert np.array_equal(per["oracle"], per["sentence"][:, 0]) and np.array_equal(per["avg"], per["oracle"]) and not per["pick"].any()
    one = ev.evaluate(seq_h)
    assert abs(out["oracle_CIDEr"] - one["CIDEr"]) <= 1e-15 and abs(out["avg_CIDEr"] - one["CIDEr"]) <= 1e-15
    assert abs(out["oracle_ROUGE_L"] - one["ROUGE_L"]) <= 1e-15 and abs(out["avg_ROUGE_L"] - one["ROUGE_L"]) <= 1e-15


def test_entry_point_checks_its_arguments():
    from boficap_amd import hip
    comps = torch.zeros(65 * 2, 10, dtype=torch.int32, device="cuda")
    cider = torch.zeros(65 * 2, dtype=torch.float64, device="cuda")
    rouge = torch.zeros(65 * 2, dtype=torch.float64, device="cuda")
    stats = torch.zeros(2, 6, 2, dtype=torch.float64, device="cuda")
    pick = torch.zeros(2, 6, dtype=torch.int32, device="cuda")
    fn, p, st = hip.lib().bofi_oracle_stats, hip.ptr, hip.stream_ptr()
    assert fn(p(comps), p(cider), p(rouge), 2, 65, None, p(stats), p(pick), st) == 1          # BOFI_ERR_ARG
    assert fn(p(comps), p(cider), p(rouge), 2, 0, None, p(stats), p(pick), st) == 1
    assert fn(p(comps), p(cider), p(rouge), 2, 2, None, None, p(pick), st) == 1
    assert fn(p(comps), p(cider), p(rouge), -1, 2, None, p(stats), p(pick), st) == 1
    assert fn(p(comps), p(cider), p(rouge), 0, 2, None, p(stats), p(pick), st) == 0           # no image: OK, no launch
    assert fn(p(comps), p(cider), p(rouge), 2, 2, None, p(stats), p(pick), st) == 0           # sent is optional
    torch.cuda.synchronize()
    assert pick.cpu().tolist() == [[0] * 6] * 2 and not stats.cpu().numpy().any()              # counts of 0: every score 0, a tie


def test_evaluate_n_does_not_synchronise_before_its_read_back():
    from boficap_amd.lang_eval import LanguageEval
    gts, seq_h, _ = case(7, 5)
    ev = LanguageEval(gts, "cuda")
    base = torch.from_numpy(seq_h).cuda()
    ev._launch_n(base, 5)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        seq = (base + 0) * (base >= 0)                             # produced on the device, still in flight
        sent, stats, pick, comps = ev._launch_n(seq, 5)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert sent.is_cuda and stats.shape == (7, 6, 2) and pick.dtype == torch.int32
    assert np.array_equal(sent.cpu().numpy().reshape(7, 5, 6), ev.evaluate_n(base, 5)["per_image"]["sentence"])


def test_eval_split_adds_the_oracle_scores(tmp_path):
    from boficap_amd import eval_utils
    from boficap_amd.config import TINY
    from test_gpu_lang_eval import LANG_KEYS, tiny_model
    path = str(tmp_path / "tiny-idxs.p")
    write_df_pickle(path, synthetic_corpus(200, seed=4, vocab=64, lengths=(3, 20)))
    labels = eval_utils.SyntheticLabels(TINY, 8, 5, seed=3)
    model = tiny_model()
    base = {"batch_size": 4, "language_eval": 1, "cached_tokens": path}
    kw = dict(base, sample_n=3, eval_oracle=1)
    _, predictions, stats = eval_utils.eval_split(model, labels.feats, labels, kw)
    assert list(stats) == LANG_KEYS + DIV_KEYS + NEW_KEYS
    per = kw["oracle_per_image"]
    assert per["sentence"].shape == (8, 3, 6) and per["oracle"].shape == (8, 6)
    assert all(stats[f"oracle_{k}"] >= stats[f"avg_{k}"] for k in KEYS)
    assert all(set(p) == {"image_id", "seq", "phrase_num", "phrase_length", "entropy", "perplexity"} for p in predictions)
    assert all(set(p) == {"image_id", "seq"} for p in kw["preds_n"])
    rows = np.zeros((24, TINY.seq_length), dtype=np.int64)         # the scores are those of the stored samples
    for j, p in enumerate(kw["preds_n"]):
        rows[j, :len(p["seq"])] = p["seq"]
    again = kw["lang_eval"].evaluate_n(rows, 3)
    assert all(again[k] == stats[k] for k in NEW_KEYS)
    kw0 = dict(base, sample_n=3, eval_oracle=0)
    stats0 = eval_utils.eval_split(model, labels.feats, labels, kw0)[2]
    assert list(stats0) == LANG_KEYS + DIV_KEYS and "oracle_per_image" not in kw0
    kw1 = dict(base, sample_n=1, eval_oracle=1)
    stats1 = eval_utils.eval_split(model, labels.feats, labels, kw1)[2]
    assert list(stats1) == LANG_KEYS and "oracle_per_image" not in kw1 and "preds_n" not in kw1
    kw2 = {"batch_size": 4, "cached_tokens": path, "sample_n": 3, "eval_oracle": 1}       # outside language_eval there is no oracle
    assert list(eval_utils.eval_split(model, labels.feats, labels, kw2)[2]) == DIV_KEYS and "oracle_per_image" not in kw2


def test_tools_eval_prints_the_oracle_scores(tmp_path):
    """tools/eval.py --language_eval 1 --sample_n 3 --eval_oracle 1 in a fresh process."""
    from boficap_amd import weights as W
    from boficap_amd.collate import synthetic_captions
    from boficap_amd.config import TINY
    Sq, n_img, per = TINY.seq_length, 8, 5
    labels, plen, psyn = synthetic_captions(TINY, n_img * per, seed=21)
    arrays = {"labels": labels[:, 1:Sq + 1].astype(np.uint32), "label_start_ix": (np.arange(n_img) * per + 1).astype(np.uint32),
              "label_end_ix": ((np.arange(n_img) + 1) * per).astype(np.uint32), "label_length": (labels[:, 1:Sq + 1] > 0).sum(1).astype(np.uint32),
              "phrase_num": (plen > 0).sum(1).astype(np.uint32), "phrase_length": plen.astype(np.uint32), "phrase_label": psyn.astype(np.uint32)}
    df, npz, pth, pkl, dump = (str(tmp_path / f) for f in ("tiny-idxs.p", "labels.npz", "model.pth", "infos.pkl", "out.json"))
    np.savez(npz, **arrays)
    write_df_pickle(df, synthetic_corpus(200, seed=4, vocab=64, lengths=(3, 20)))
    torch.save({k: torch.from_numpy(v) for k, v in W.make_state_dict(TINY, seed=0, gen_scale=6.0).items()}, pth)
    opt = TINY.to_opt()
    with open(pkl, "wb") as f:
        pickle.dump({"opt": opt, "vocab": opt.vocab}, f, protocol=2)
    cmd = [sys.executable, os.path.join(ROOT, "tools", "eval.py"), "--model", pth, "--infos_path", pkl, "--synthetic", str(n_img), "--batch_size", "4",
           "--dtype", "f32", "--input_label_npz", npz, "--cached_tokens", df, "--dump_json", dump, "--language_eval", "1", "--sample_n", "3",
           "--eval_oracle", "1"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    line = out.stdout.split("oracle scores ")[1].splitlines()[0]
    printed = dict(re.findall(r"(\w+) (-?[0-9.]+|nan)", line))
    assert list(printed) == NEW_KEYS
    assert all(float(printed[f"oracle_{k}"]) >= float(printed[f"avg_{k}"]) for k in KEYS)
    with open(dump) as f:
        dumped = json.load(f)
    assert set(dumped) == {"predictions", "preds_n", "lang_stats"} and len(dumped["preds_n"]) == 24
    assert [f"{dumped['lang_stats'][k]:.6f}" for k in NEW_KEYS] == [printed[k] for k in NEW_KEYS]
    assert "language scores " in out.stdout and "diversity scores " in out.stdout
