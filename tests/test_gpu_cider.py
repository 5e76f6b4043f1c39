"""CIDEr-D scorer on the MI355X (boficap_amd/csrc/cider.hip) against the float64 restatement of tests/test_cider.py: the worked example,
a random batch in both df modes, the package's compute_score contract, no host synchronisation, and the self-critical paths that take
it when no host scorer is installed (LossWrapper's RL branch, XETrainer.rl_step)."""
import math

import numpy as np
import pytest
import torch

from conftest import load_golden, record_parity
from test_cider import (WORKED_CANDS, WORKED_CORPUS, WORKED_REFS, WORKED_SCORES, restated_scores, synthetic_corpus,
                        write_df_pickle)

pytestmark = pytest.mark.gpu


def test_worked_example(tmp_path):
    from boficap_amd.cider import CiderD
    path = str(tmp_path / "worked-idxs.p")
    write_df_pickle(path, WORKED_CORPUS)
    sc = CiderD(df=path)
    seq = torch.from_numpy(WORKED_CANDS).cuda()
    out, out64 = sc.score([WORKED_REFS], seq, len(WORKED_CANDS), out64=True)
    err = float(np.abs(out64.cpu().numpy() - np.array(WORKED_SCORES)).max())
    record_parity("cider_worked_example", err, 1e-9)
    assert err <= 1e-9, out64
    assert torch.equal(out.cpu(), out64.cpu().float())


def _random_batch(seed, n_img=64, spi=5, S=20, vocab=150):
    """References 5-7 per image (some fill all S ids: no 0), candidates: copies and cuts of references, repeated n-grams (clipping),
    ids the df table never saw, rows without a 0, all-zero rows."""
    rng = np.random.default_rng(seed)
    gts = []
    for _ in range(n_img):
        rows = np.zeros((rng.integers(5, 8), S), dtype=np.int64)
        for r in rows:
            n = S if rng.random() < 0.15 else rng.integers(3, S)
            r[:n] = rng.integers(1, vocab, n)
        gts.append(rows)
    seq = np.zeros((n_img * spi, S), dtype=np.int64)
    for j in range(n_img * spi):
        refs, kind = gts[j // spi], j % spi
        src = refs[rng.integers(len(refs))]
        if kind == 0:                                                       # a reference, perhaps cut short
            cut = rng.integers(1, S + 1)
            seq[j, :cut] = src[:cut]
        elif kind == 1:                                                     # a repeated bigram / trigram
            g = rng.integers(1, vocab, rng.integers(2, 4))
            seq[j, :] = np.resize(g, S)
            seq[j, rng.integers(6, S):] = 0
        elif kind == 2:                                                     # no 0 at all, with unseen ids
            seq[j] = rng.integers(1, vocab, S)
            seq[j, rng.integers(0, S, 4)] = rng.integers(1000, 1100, 4)
        elif kind == 3:                                                     # a reference's words reshuffled
            toks = src[src > 0]
            seq[j, :len(toks)] = rng.permutation(toks)
        elif rng.random() < 0.5:                                            # all zeros, or random words
            seq[j, :rng.integers(1, S)] = rng.integers(1, vocab, 1)[0]
    return gts, seq


def test_random_batch_against_the_restatement(tmp_path):
    from boficap_amd.cider import CiderD
    corpus = synthetic_corpus(2000, seed=11, vocab=150, lengths=(3, 20))
    path = str(tmp_path / "syn-idxs.p")
    df = write_df_pickle(path, corpus)
    gts, seq_h = _random_batch(5)
    assert (seq_h == 0).all(1).any() and (seq_h != 0).all(1).any()
    seq = torch.from_numpy(seq_h).cuda()
    for mode, sc, want in (("file", CiderD(df=path), restated_scores(gts, seq_h, 5, df, math.log(2000.0))),
                           ("corpus", CiderD(df="corpus"), restated_scores(gts, seq_h, 5))):
        out, out64 = sc.score(gts, seq, 5, weight=1.0, out64=True)
        got = out64.cpu().numpy()
        err = float(np.abs(got - want).max())
        record_parity(f"cider_random_batch_{mode}", err, 1e-9, "64 images x 5 samples, 5-7 references, S = 20")
        assert err <= 1e-9, (mode, err)
        assert (want > 0).sum() > 100 and (want == 0).any()                # the batch exercises both overlapping and disjoint captions
        again, again64 = sc.score(gts, seq, 5, weight=1.0, out64=True)
        assert torch.equal(again64, out64) and torch.equal(again, out)      # fixed summation order: bit-identical
        w = sc.score(gts, seq, 5, weight=0.5)
        assert torch.equal(w.cpu(), (out64 * 0.5).float().cpu())


def test_compute_score_is_the_drop_in_form(tmp_path):
    from boficap_amd.cider import CiderD
    corpus = synthetic_corpus(300, seed=2, vocab=150, lengths=(3, 20))
    path = str(tmp_path / "syn-idxs.p")
    write_df_pickle(path, corpus)
    gts, seq_h = _random_batch(9, n_img=8)
    sc = CiderD(df=path)

    def to_str(row):                                                        # array_to_str (rewards.py:33-39)
        out = []
        for t in row:
            out.append(str(int(t)))
            if t == 0:
                break
        return " ".join(out)
    res = [{"image_id": j, "caption": [to_str(seq_h[j])]} for j in range(len(seq_h))]
    refs = {j: [to_str(r) for r in gts[j // 5]] for j in range(len(seq_h))}
    mean, arr = sc.compute_score(refs, res)
    _, o64 = sc.score(gts, torch.from_numpy(seq_h).cuda(), 5, out64=True)
    assert isinstance(mean, float) and isinstance(arr, np.ndarray) and arr.shape == (len(seq_h),)
    assert np.array_equal(arr, o64.cpu().numpy()) and mean == float(np.mean(arr))


def test_score_does_not_synchronise(tmp_path):
    from boficap_amd.cider import CiderD
    gts, seq_h = _random_batch(3, n_img=16)
    sc = CiderD(df="corpus")
    base = torch.from_numpy(seq_h).cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        seq = (base + 0) * (base >= 0)                                      # produced on the device, still in flight
        out = sc.score(gts, seq, 5)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert out.is_cuda and out.dtype == torch.float32
    assert np.abs(out.cpu().numpy() - restated_scores(gts, seq_h, 5)).max() < 1e-5


def _tiny(weight_cache, manifest, **opt_extra):
    import captioning.models as models
    m = manifest["tiny_saic_multi"]
    cfg, sd = weight_cache(m["config"], m["seed"], m["gen_scale"], m["digest"], m.get("patch"))
    model = models.setup(cfg.to_opt(**opt_extra))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return cfg, model.cuda()


def _tiny_refs(cfg, B, seed):
    rng = np.random.default_rng(seed)
    gts = []
    for _ in range(B):
        rows = np.zeros((rng.integers(3, 6), cfg.seq_length), dtype=np.int64)
        for r in rows:
            n = rng.integers(3, cfg.seq_length)
            r[:n] = rng.integers(1, cfg.vocab_size + 4, n)
        gts.append(rows)
    return gts


def test_loss_wrapper_rl_branch_scores_with_cider_d(weight_cache, manifest, tmp_path):
    """No scorer installed, opt.cached_tokens = a df pickle: the RL branch runs (it raised before) and its reward is CIDEr-D."""
    from boficap_amd import loss_wrapper as LW, xe
    from captioning.modules.loss_wrapper import LossWrapper
    path = str(tmp_path / "tiny-idxs.p")
    df = write_df_pickle(path, synthetic_corpus(500, seed=4, vocab=64, lengths=(3, 20)))
    n = 3
    cfg, model = _tiny(weight_cache, manifest, structure_loss_type="new_self_critical", train_sample_n=n, structure_loss_weight=1,
                       train_sample_method="sample", train_beam_size=1, seed=5, cached_tokens=path)
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
        seen.append((input.detach(), seq.detach().cpu().numpy(), out))
        return out
    lw.struc_crit.forward = record
    out = lw(torch.zeros(B, 0, device="cuda"), att, None, None, None, gts, torch.arange(B), False, True, False)
    assert torch.isfinite(out["loss"]) and len(seen) == 2
    total = 0
    for lp, seq, o in seen:
        want = restated_scores(gts, seq, n, df, math.log(500.0))
        err = float(np.abs(o["reward"].reshape(-1).detach().cpu().numpy() - want).max())
        assert err <= 1e-6, err
        loss, _ = xe.structure_loss("new_self_critical", lp, torch.from_numpy(seq).cuda(), torch.from_numpy(want).float(), n)
        assert abs(float(o["loss"]) - float(loss)) <= 1e-6 * max(1.0, abs(float(loss)))
        total = total + want
    assert np.abs(out["reward"].reshape(-1).detach().cpu().numpy() - total).max() <= 2e-6
    assert (total > 0).any()
    out["loss"].backward()


def test_rl_step_with_cider_d_equals_a_host_scorer(weight_cache, manifest, tmp_path):
    """XETrainer.rl_step with CiderD.bind (device ids in, device scores out) against the same step with a host score_fn returning the
    restatement's scores: same samples, same loss, same parameters after the step."""
    from boficap_amd.cider import CiderD
    from boficap_amd.trainer import XETrainer
    path = str(tmp_path / "tiny-idxs.p")
    df = write_df_pickle(path, synthetic_corpus(500, seed=4, vocab=64, lengths=(3, 20)))
    n = 3
    att = torch.from_numpy(load_golden("tiny_saic_multi")["att_feats"]).cuda()
    results = []
    for device_scorer in (True, False):
        cfg, model = _tiny(weight_cache, manifest, seed=9)
        opt = model.opt
        opt.noamopt, opt.learning_rate = False, 1e-4
        tr = XETrainer(model, opt)
        gts = _tiny_refs(cfg, att.size(0), seed=8)
        if device_scorer:
            score = CiderD(df=path).bind(gts, n)
        else:
            def score(seq):
                return torch.from_numpy(restated_scores(gts, seq.numpy(), n, df, math.log(500.0))).float()
        model.train()
        loss, rs, rn = tr.rl_step(att, None, score, sample_n=n, temperature=1.0)
        results.append((float(loss), float(rs), float(rn), tr.bucket.flat.detach().clone()))
        assert torch.isfinite(loss)
    (l0, s0, n0, w0), (l1, s1, n1, w1) = results
    assert abs(l0 - l1) <= 1e-6 and abs(s0 - s1) <= 1e-6 and abs(n0 - n1) <= 1e-6, results
    assert s1 > 0 or n1 > 0                                                 # the samples share words with the references
    assert float((w0 - w1).abs().max()) <= 1e-6
