"""Diversity scores on the MI355X (boficap_amd/csrc/diversity.hip) against the float64 restatement of tests/test_diversity.py: the kernel's
matrix, counts and score, the self-CIDEr reward term of the 'new_self_critical' loss, and the evaluation with ``sample_n`` > 1."""
import math
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden, record_parity
from test_cider import synthetic_corpus, write_df_pickle
from test_diversity import div_of_eigenvalues, restated_diversity

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ["Div-1", "Div-2", "mBLEU_1", "mBLEU_2", "mBLEU_3", "mBLEU_4", "self_cider"]
CORPUS = dict(n_images=400, seed=6, vocab=30, lengths=(3, 20))
_WANT = {}


def batch(n, S, rule):
    """6 images of n samples over ~30 ids.  S = 20: image 0 all samples equal, image 1 two equal samples, image 2 rows of 1-3 tokens and a
    row that is [0] only, image 3 all samples empty under the 'eval' rule, images 4-5 random rows (some without a 0).  S = 64: no 0 at all,
    250 n-grams per row (image 0 all equal, image 1 two equal)."""
    rng = np.random.default_rng(10 * n + S)
    seq = rng.integers(1, 30, (6 * n, S)).astype(np.int64)
    if S == 64:
        seq[:n] = seq[0]
        seq[n + 1] = seq[n]
        return seq
    for j, row in enumerate(seq):
        if j % 4 != 3:
            row[int(rng.integers(4, S)):] = 0
    seq[0, 9:] = 0
    seq[:n] = seq[0]
    seq[n + 1] = seq[n]
    for k in range(n):
        seq[2 * n + k, 1 + k % 3:] = 0                                      # 1, 2, 3 tokens, then padding
    seq[2 * n + n - 1] = 0                                                  # [0] only
    seq[3 * n:4 * n, 0] = 0                                                 # nothing before the first 0
    if rule == "eval":
        seq[3 * n + 1, 0] = -1                                              # (an id below 0 ends a row under this rule only)
    return seq


def restated(n, S, rule, df):
    key = (n, S, rule)
    if key not in _WANT:                                                    # computed once, shared, left unchanged
        _WANT[key] = restated_diversity(batch(n, S, rule), n, df, math.log(float(CORPUS["n_images"])), rule)
    return _WANT[key]


@pytest.fixture(scope="module")
def df_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("df") / "div-idxs.p")
    return path, write_df_pickle(path, synthetic_corpus(**CORPUS))


@pytest.mark.parametrize("n,S,rule", [(2, 20, "reward"), (5, 20, "reward"), (16, 20, "reward"), (2, 20, "eval"), (5, 20, "eval"), (16, 20, "eval"),
                                      (5, 64, "reward")])
def test_kernel_against_the_restatement(df_file, n, S, rule):
    """Score bar 1e-6: an eigenvalue that is 0 in exact arithmetic comes out as +-eps ~ n 2^-53 |M|, its clipped square root as up to ~1e-7, and
    LAPACK and a Jacobi sweep differ by that much; with l_max >= trace / n the score moves by at most ~(n + 1) sqrt(eps) / log n < 1e-6.
    Measured on the MI355X over these seven cases: |M - restatement| <= 2.3e-16, |score - restatement| <= 6.5e-9 (the rank-deficient images)."""
    from boficap_amd import diversity
    path, df = df_file
    seq_h, want = batch(n, S, rule), restated(n, S, rule, df)
    sc = diversity.SelfCider(path)
    seq = torch.from_numpy(seq_h).cuda()
    score, mat, div, comps = sc._launch(seq, n, rule, want_mat=True, want_comps=True)
    M, got = mat.cpu().numpy(), score.cpu().numpy()
    err_m = float(np.abs(M - want["M"]).max())
    nan_w, nan_g = np.isnan(want["score"]), np.isnan(got)
    err_s = float(np.abs(got - want["score"])[~nan_w].max())
    own = np.array([div_of_eigenvalues(m) for m in M])                      # the formula by numpy on the device's own M
    err_own = float(np.abs(got - own)[~nan_w].max())
    print(f"n {n} S {S} {rule}: |M - restatement| {err_m:.3e}, |score - restatement| {err_s:.3e}, |score - numpy(device M)| {err_own:.3e}")
    record_parity(f"diversity_matrix_n{n}_S{S}_{rule}", err_m, 1e-15)
    record_parity(f"diversity_score_n{n}_S{S}_{rule}", max(err_s, err_own), 1e-6)
    assert err_m <= 1e-15
    assert np.array_equal(M, M.transpose(0, 2, 1))                          # exactly symmetric
    assert np.array_equal(nan_g, nan_w) and np.array_equal(np.isnan(own), nan_w)
    # image 3 of the S = 20 batches: no tokens ('eval'), or the token 0 alone ('reward'), which every image of the corpus holds: weight 0, M = 0
    assert bool(nan_w[3]) == (S == 20) and nan_w.sum() <= 1
    assert err_s <= 1e-6 and err_own <= 1e-6
    assert np.array_equal(div.cpu().numpy(), want["div"]) and np.array_equal(comps.cpu().numpy(), want["comps"])
    stats, _, _ = diversity.stats_of_counts(div.cpu().numpy(), comps.cpu().numpy(), n)
    for k in KEYS[:6]:
        assert abs(stats[k] - want["stats"][k]) <= 1e-15, (k, stats[k], want["stats"][k])
    assert torch.equal(sc.score(seq, n, rule)[~torch.from_numpy(nan_w).cuda()], score[~torch.from_numpy(nan_w).cuda()])
    assert torch.equal(sc.matrix(seq, n, rule), mat)
    again = sc._launch(seq, n, rule, want_mat=True, want_comps=True)        # fixed summation and rotation orders: bit-identical
    assert all(torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b)
               for a, b in zip(again, (score, mat, div, comps)))
    if S == 20:
        assert abs(got[0]) <= 1e-6                                          # all samples equal: rank 1, score 0
        assert (want["score"][~nan_w] >= -1e-9).all() and (want["score"][~nan_w] <= 1 + 1e-9).all()


def test_evaluate_is_the_restatement_and_does_not_synchronise_to_score(df_file):
    from boficap_amd import diversity
    path, df = df_file
    n, S = 5, 20
    want = restated(n, S, "eval", df)
    seq_h = batch(n, S, "eval")
    ev = diversity.DiversityEval(path, "cuda")
    stats = ev.evaluate(seq_h, n)
    assert list(stats) == KEYS + ["per_image"]
    for k in KEYS[:6]:
        assert abs(stats[k] - want["stats"][k]) <= 1e-15, k
    assert abs(stats["self_cider"] - want["stats"]["self_cider"]) <= 1e-6
    assert np.isnan(stats["per_image"]["self_cider"][3]) and stats["per_image"]["Div-1"].shape == (6,)
    sc = diversity.SelfCider(path)
    base = torch.from_numpy(batch(n, S, "reward")).cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        seq = (base + 0) * (base >= 0)                                      # produced on the device, still in flight
        out = sc.score(seq, n)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert out.is_cuda and out.dtype == torch.float64 and out.shape == (6,)
    with pytest.raises(ValueError):
        sc.score(seq[:5], 1)
    with pytest.raises(ValueError):
        sc.score(seq.repeat(4, 1)[:102], 17)
    opt = type("Opt", (), {"cached_tokens": path})()
    arr = diversity.get_self_cider_scores([None] * 6, seq, opt)             # the reference's contract: numpy out
    assert isinstance(arr, np.ndarray) and np.array_equal(arr, out.cpu().numpy(), equal_nan=True)


def test_self_cider_reward_term_in_the_structure_loss(weight_cache, manifest, tmp_path):
    """self_cider_reward_weight 0.5 with 'new_self_critical': the advantage gains 0.5 x the image's self-CIDEr after the baseline (this raised
    NotImplementedError before); weight 0 is the loss without the term, bit for bit; one LossWrapper RL step runs."""
    from boficap_amd import loss_wrapper as LW, xe
    from captioning.modules.loss_wrapper import LossWrapper
    from test_gpu_cider import _tiny, _tiny_refs
    path = str(tmp_path / "tiny-idxs.p")
    corpus = synthetic_corpus(500, seed=4, vocab=64, lengths=(3, 20))
    df = write_df_pickle(path, corpus)
    n = 3
    kw = dict(structure_loss_type="new_self_critical", train_sample_n=n, structure_loss_weight=1, train_sample_method="sample", train_beam_size=1,
              seed=5, cached_tokens=path)
    cfg, model = _tiny(weight_cache, manifest, self_cider_reward_weight=0.5, **kw)
    assert LW._SCORER["fn"] is None
    att = torch.from_numpy(load_golden("tiny_saic_multi")["att_feats"]).cuda()
    B = att.size(0)
    gts = _tiny_refs(cfg, B, seed=7)
    model.train()
    lw = LossWrapper(model, model.opt)
    seen = []
    crit = lw.struc_crit.forward

    def record(input, seq, data_gts, reduction="mean"):
        out = crit(input, seq, data_gts, reduction)
        seen.append((input.detach(), seq.detach(), out))
        return out
    lw.struc_crit.forward = record
    out = lw(torch.zeros(B, 0, device="cuda"), att, None, None, None, gts, torch.arange(B), False, True, False)      # one RL step
    assert torch.isfinite(out["loss"]) and len(seen) == 2
    out["loss"].backward()
    zero = LW.StructureLosses(type("Opt", (), dict(kw, self_cider_reward_weight=0))())
    other = LW.StructureLosses(type("Opt", (), dict(kw, self_cider_reward_weight=0.5, structure_loss_type="seqnll"))())
    for lp, seq, o in seen:
        reward = o["reward"].reshape(-1)                                    # the raw scores: the term does not enter the reported reward
        want = restated_diversity(seq.cpu().numpy(), n, df, math.log(500.0), "reward")["score"]
        assert not np.isnan(want).any() and (want > 0).any()
        sc = reward.view(-1, n)
        adv = sc - (sc.sum(1, keepdim=True) - sc) / (n - 1) + 0.5 * torch.from_numpy(want).float().cuda().view(-1, 1)
        mask = torch.cat([torch.ones(B * n, 1, device="cuda"), (seq > 0).float()[:, :-1]], 1)
        loss = (-lp.gather(2, seq.unsqueeze(2)).squeeze(2) * mask * adv.reshape(-1, 1)).sum() / mask.sum()
        plain, _ = xe.structure_loss("new_self_critical", lp, seq, reward, n)
        print(f"loss {float(o['loss'].detach())!r} restated {float(loss)!r} without the term {float(plain)!r}")
        assert abs(float(o["loss"]) - float(loss)) <= 1e-6 * max(1.0, abs(float(loss)))
        assert abs(float(o["loss"]) - float(plain)) > 1e-4                  # the term is there
        z = zero(lp, seq, gts)                                              # weight 0: the loss without the term, bit for bit
        assert torch.equal(z["loss"], plain) and torch.equal(z["reward"].reshape(-1), reward)
        a, b = other(lp, seq, gts)["loss"], xe.structure_loss("seqnll", lp, seq, reward, n)[0]
        assert torch.equal(a, b)                                            # the other types ignore the weight


def test_eval_split_samples_n_captions_and_scores_their_diversity(tmp_path):
    from boficap_amd import diversity, eval_utils
    from test_gpu_lang_eval import tiny_model
    from boficap_amd.config import TINY
    path = str(tmp_path / "tiny-idxs.p")
    write_df_pickle(path, synthetic_corpus(200, seed=4, vocab=64, lengths=(3, 20)))
    labels = eval_utils.SyntheticLabels(TINY, 8, 5, seed=3)
    model = tiny_model()
    for mode in ("NAIC", "SAIC"):
        plain = eval_utils.eval_split(model, labels.feats, labels, {"batch_size": 4, "language_eval": 1, "inference_mode": mode})
        kw = {"batch_size": 4, "language_eval": 1, "inference_mode": mode, "cached_tokens": path}
        val_loss, predictions, stats = eval_utils.eval_split(model, labels.feats, labels, kw, sample_n=3)
        assert val_loss == plain[0] and predictions == plain[1]             # the greedy pass is untouched
        assert list(stats) == list(plain[2]) + KEYS and all(stats[k] == plain[2][k] for k in plain[2])
        preds_n = kw["preds_n"]
        assert len(preds_n) == 24 and [p["image_id"] for p in preds_n] == [i // 3 for i in range(24)]
        rows = np.zeros((24, TINY.seq_length), dtype=np.int64)
        for j, p in enumerate(preds_n):
            rows[j, :len(p["seq"])] = p["seq"]
        want = diversity.DiversityEval(path, "cuda").evaluate(rows, 3)
        assert all(stats[k] == want[k] or (math.isnan(stats[k]) and math.isnan(want[k])) for k in KEYS), (stats, want)
        assert 0 <= stats["Div-1"] <= 1 and 0 <= stats["Div-2"] <= 1
        if mode == "NAIC":                                                  # (this seeded model's SAIC captions are empty, greedy and sampled alike)
            assert stats["Div-1"] > 0 and len({tuple(p["seq"]) for p in preds_n}) > 4          # the samples of an image differ
        # sample_n <= 1: exactly the outputs without it
        kw1 = {"batch_size": 4, "language_eval": 1, "inference_mode": mode, "sample_n": 1}
        again = eval_utils.eval_split(model, labels.feats, labels, kw1)
        assert again[0] == plain[0] and again[1] == plain[1] and again[2] == plain[2] and "preds_n" not in kw1


def test_tools_eval_prints_the_diversity_scores(tmp_path):
    """tools/eval.py --sample_n 3 in a fresh process."""
    from boficap_amd import weights as W
    from boficap_amd.config import TINY
    df, pth, pkl, dump = (str(tmp_path / f) for f in ("tiny-idxs.p", "model.pth", "infos.pkl", "out.json"))
    write_df_pickle(df, synthetic_corpus(200, seed=4, vocab=64, lengths=(3, 20)))
    torch.save({k: torch.from_numpy(v) for k, v in W.make_state_dict(TINY, seed=0, gen_scale=6.0).items()}, pth)
    opt = TINY.to_opt()
    with open(pkl, "wb") as f:
        pickle.dump({"opt": opt, "vocab": opt.vocab}, f, protocol=2)
    cmd = [sys.executable, os.path.join(ROOT, "tools", "eval.py"), "--model", pth, "--infos_path", pkl, "--synthetic", "8", "--batch_size", "4",
           "--dtype", "f32", "--sample_n", "3", "--cached_tokens", df, "--dump_json", dump]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    line = out.stdout.split("diversity scores ")[1].splitlines()[0]
    printed = dict(re.findall(r"([\w-]+) (-?[0-9.]+|nan)", line))
    assert list(printed) == KEYS and 0 < float(printed["Div-1"]) <= 1
    import json
    with open(dump) as f:
        dumped = json.load(f)
    assert set(dumped) == {"predictions", "preds_n", "lang_stats"} and len(dumped["preds_n"]) == 24 and len(dumped["predictions"]) == 8
    assert [f"{dumped['lang_stats'][k]:.6f}" for k in KEYS] == [printed[k] for k in KEYS]
