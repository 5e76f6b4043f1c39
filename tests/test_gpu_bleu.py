"""BLEU-4 term and the combined reward on the MI355X (bofi_reward_refs / bofi_reward_score of boficap_amd/csrc/cider.hip) against the float64
restatements of tests/test_bleu.py and tests/test_cider.py: the worked table, a random batch with its counts and corpus score, the
bit-identity of the combined kernel with the CIDEr-D one when the BLEU weight is 0, no host synchronisation, and the self-critical
paths that take the combined scorer (LossWrapper's RL branch, XETrainer.rl_step)."""
import math

import numpy as np
import pytest
import torch

from conftest import load_golden, record_parity
from test_bleu import WORKED, bleu_of, corpus_bleu, restated_bleu
from test_cider import restated_scores, synthetic_corpus, write_df_pickle
from test_gpu_cider import _random_batch, _tiny, _tiny_refs

pytestmark = pytest.mark.gpu


def _to_str(row):                                                           # array_to_str (rewards.py:33-39)
    out = []
    for t in row:
        out.append(str(int(t)))
        if t == 0:
            break
    return " ".join(out)


def _worked_batch():
    S = max(len(w[0]) for w in WORKED)
    W = max(len(r) for w in WORKED for r in w[1])
    seq = np.zeros((len(WORKED), S), dtype=np.int64)
    gts = []
    for i, (cand, refs, _, _) in enumerate(WORKED):
        seq[i, :len(cand)] = cand
        g = np.zeros((len(refs), W), dtype=np.int64)
        for j, r in enumerate(refs):
            g[j, :len(r)] = r
        gts.append(g)
    return gts, seq


def test_worked_table():
    from boficap_amd.bleu import Bleu
    gts, seq_h = _worked_batch()
    sc = Bleu(4)
    out, out64, comps = sc.score(gts, torch.from_numpy(seq_h).cuda(), 1, out64=True, comps=True)
    want = np.array([w[3] for w in WORKED])
    err = float(np.abs(out64.cpu().numpy() - want).max())
    record_parity("bleu_worked_table", err, 1e-15, "BLEU-4 of the four worked rows")
    assert err <= 1e-15, out64
    assert torch.equal(out.cpu(), out64.cpu().float())
    assert comps.cpu().tolist() == [[c[0], c[1], *c[2], *c[3]] for _, _, c, _ in WORKED]
    # the package's contract on the same rows
    res = {i: [_to_str(seq_h[i])] for i in range(len(WORKED))}
    refs = {i: [_to_str(r) for r in gts[i]] for i in range(len(WORKED))}
    corpus, per = sc.compute_score(refs, res)
    assert per[0][0] == bleu_of(*WORKED[0][2])[0] and abs(per[0][0] - 0.7999999996800004) <= 1e-16
    assert all(per[3][i] == bleu_of(*WORKED[i][2])[3] for i in range(len(WORKED)))
    assert corpus == corpus_bleu([w[2] for w in WORKED])
    # an id outside [0, 65534] has no key: NaN, as in the CIDEr-D kernel
    bad = seq_h.copy()
    bad[1, 1] = 70000
    assert torch.isnan(sc.score(gts, torch.from_numpy(bad).cuda(), 1).cpu()).tolist() == [False, True, False, False]


def test_random_batch_against_the_restatement():
    from boficap_amd.bleu import Bleu
    gts, seq_h = _random_batch(6)
    sc = Bleu(4)
    seq = torch.from_numpy(seq_h).cuda()
    out, out64, comps = sc.score(gts, seq, 5, out64=True, comps=True)
    want, want_comps, rows = restated_bleu(gts, seq_h, 5)
    err = float(np.abs(out64.cpu().numpy() - want).max())
    record_parity("bleu_random_batch", err, 1e-15, "64 images x 5 samples, 5-7 references, S = 20")
    assert err <= 1e-15, err
    assert np.array_equal(comps.cpu().numpy().astype(np.int64), want_comps)
    assert (want > 1e-3).sum() > 20 and (want < 1e-6).any()                 # the batch holds close copies and unrelated captions
    again = sc.score(gts, seq, 5, out64=True)[1]
    assert torch.equal(again, out64)
    # compute_score: per-sentence and corpus BLEU-1..4 bit-equal to the restatement's
    res = {j: [_to_str(seq_h[j])] for j in range(len(seq_h))}
    refs = {j: [_to_str(r) for r in gts[j // 5]] for j in range(len(seq_h))}
    corpus, per = sc.compute_score(refs, res)
    assert corpus == corpus_bleu(rows)
    assert [list(x) for x in zip(*per)] == [bleu_of(*c) for c in rows]


def test_combined_kernel(tmp_path):
    """bleu_weight 0: the combined kernel's CIDEr-D is bofi_cider_score's bit for bit; both weights: cw * CIDEr-D + bw * BLEU-4."""
    from boficap_amd.cider import CiderD
    from boficap_amd.rewards import RewardScorer
    path = str(tmp_path / "syn-idxs.p")
    df = write_df_pickle(path, synthetic_corpus(2000, seed=11, vocab=150, lengths=(3, 20)))
    gts, seq_h = _random_batch(7)
    seq = torch.from_numpy(seq_h).cuda()
    bleu = restated_bleu(gts, seq_h, 5)[0]
    errs = []
    for mode, dfa, cider in (("file", path, restated_scores(gts, seq_h, 5, df, math.log(2000.0))),
                             ("corpus", "corpus", restated_scores(gts, seq_h, 5))):
        for cw in (1.0, 0.7):
            o, o64 = CiderD(df=dfa).score(gts, seq, 5, weight=cw, out64=True)
            r, r64 = RewardScorer(df=dfa, cider_weight=cw, bleu_weight=0.0).score(gts, seq, 5, out64=True)
            assert torch.equal(r64, o64) and torch.equal(r, o), (mode, cw)
        cw, bw = 1.0, 0.5
        r, r64 = RewardScorer(df=dfa, cider_weight=cw, bleu_weight=bw).score(gts, seq, 5, out64=True)
        want = cw * cider + bw * bleu
        errs.append(float(np.abs(r64.cpu().numpy() - want).max()))
        assert errs[-1] <= 1e-14, (mode, errs[-1])
        assert torch.equal(r.cpu(), r64.cpu().float())
    record_parity("reward_cider_plus_bleu", max(errs), 1e-14, "1.0 x CIDEr-D + 0.5 x BLEU-4, both df modes")


def test_score_does_not_synchronise():
    from boficap_amd.rewards import RewardScorer
    gts, seq_h = _random_batch(3, n_img=16)
    sc = RewardScorer(df="corpus", cider_weight=1.0, bleu_weight=0.5)
    base = torch.from_numpy(seq_h).cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        seq = (base + 0) * (base >= 0)                                      # produced on the device, still in flight
        out = sc.score(gts, seq, 5)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert out.is_cuda and out.dtype == torch.float32
    want = restated_scores(gts, seq_h, 5) + 0.5 * restated_bleu(gts, seq_h, 5)[0]
    assert np.abs(out.cpu().numpy() - want).max() < 1e-5


@pytest.mark.parametrize("cider_weight", [1.0, 0.0])
def test_loss_wrapper_rl_branch_with_bleu(weight_cache, manifest, tmp_path, monkeypatch, cider_weight):
    """bleu_reward_weight 0.5, no scorer installed: the RL branch runs (it raised NotImplementedError before), with a df pickle for the
    CIDEr-D term or, at cider_reward_weight 0, with no df file at all; the scores reaching xe.structure_loss are the restatement's."""
    from boficap_amd import loss_wrapper as LW, xe
    from captioning.modules.loss_wrapper import LossWrapper
    n, bw = 3, 0.5
    if cider_weight > 0:
        path = str(tmp_path / "tiny-idxs.p")
        df = write_df_pickle(path, synthetic_corpus(500, seed=4, vocab=64, lengths=(3, 20)))
    else:
        path, df = str(tmp_path / "no-such-table.p"), None
    cfg, model = _tiny(weight_cache, manifest, structure_loss_type="new_self_critical", train_sample_n=n, structure_loss_weight=1,
                       train_sample_method="sample", train_beam_size=1, seed=5, cached_tokens=path, cider_reward_weight=cider_weight,
                       bleu_reward_weight=bw)
    assert LW._SCORER["fn"] is None
    att = torch.from_numpy(load_golden("tiny_saic_multi")["att_feats"]).cuda()
    B = att.size(0)
    gts = _tiny_refs(cfg, B, seed=7)
    seen = []
    structure_loss = xe.structure_loss

    def record(loss_type, input, seq, scores, *a, **kw):
        seen.append((seq.detach().cpu().numpy(), scores.detach().cpu().numpy()))
        return structure_loss(loss_type, input, seq, scores, *a, **kw)
    monkeypatch.setattr(xe, "structure_loss", record)
    model.train()
    lw = LossWrapper(model, model.opt)
    out = lw(torch.zeros(B, 0, device="cuda"), att, None, None, None, gts, torch.arange(B), False, True, False)
    assert torch.isfinite(out["loss"]) and len(seen) == 2
    for seq, scores in seen:
        want = bw * restated_bleu(gts, seq, n)[0]
        if cider_weight > 0:
            want = want + cider_weight * restated_scores(gts, seq, n, df, math.log(500.0))
        err = float(np.abs(scores - want).max())
        assert err <= 1e-6 * max(1.0, float(np.abs(want).max())), err
        assert (want > 0).any()
    out["loss"].backward()


def test_rl_step_with_the_combined_scorer_equals_a_host_scorer(weight_cache, manifest, tmp_path):
    """XETrainer.rl_step with RewardScorer.bind (device ids in, device scores out) against the same step with a host score_fn returning
    the restatements' weighted sum: same samples, same loss, same parameters after the step."""
    from boficap_amd.rewards import RewardScorer
    from boficap_amd.trainer import XETrainer
    path = str(tmp_path / "tiny-idxs.p")
    df = write_df_pickle(path, synthetic_corpus(500, seed=4, vocab=64, lengths=(3, 20)))
    n, cw, bw = 3, 1.0, 0.5
    att = torch.from_numpy(load_golden("tiny_saic_multi")["att_feats"]).cuda()
    results = []
    for device_scorer in (True, False):
        cfg, model = _tiny(weight_cache, manifest, seed=9)
        opt = model.opt
        opt.noamopt, opt.learning_rate = False, 1e-4
        tr = XETrainer(model, opt)
        gts = _tiny_refs(cfg, att.size(0), seed=8)
        if device_scorer:
            score = RewardScorer(df=path, cider_weight=cw, bleu_weight=bw).bind(gts, n)
        else:
            def score(seq):
                s = seq.numpy()
                return torch.from_numpy(cw * restated_scores(gts, s, n, df, math.log(500.0)) + bw * restated_bleu(gts, s, n)[0]).float()
        model.train()
        loss, rs, rn = tr.rl_step(att, None, score, sample_n=n, temperature=1.0)
        results.append((float(loss), float(rs), float(rn), tr.bucket.flat.detach().clone()))
        assert torch.isfinite(loss)
    (l0, s0, n0, w0), (l1, s1, n1, w1) = results
    assert abs(l0 - l1) <= 1e-6 and abs(s0 - s1) <= 1e-6 and abs(n0 - n1) <= 1e-6, results
    assert s1 > 0 or n1 > 0
    assert float((w0 - w1).abs().max()) <= 1e-6
