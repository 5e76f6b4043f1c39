#!/usr/bin/env python3
"""Time the device reward scorers at 64 images x 5 samples x 5 references, S = 20: CIDEr-D alone (boficap_amd.cider.CiderD), BLEU-4 alone
(boficap_amd.bleu.Bleu) and both in one pass (boficap_amd.rewards.RewardScorer, 1.0 x CIDEr-D + 0.5 x BLEU-4), and the float64 host
restatement of BLEU in tests/test_bleu.py on the same batch for comparison.  usage: python dev/time_bleu.py [iters]"""
import math, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch
from boficap_amd.bleu import Bleu
from boficap_amd.cider import CiderD
from boficap_amd.rewards import RewardScorer
from test_bleu import restated_bleu
from test_cider import restated_scores, synthetic_corpus, write_df_pickle

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 50
rng = np.random.default_rng(0)
n_img, spi, S = 64, 5, 20
with tempfile.TemporaryDirectory() as d:
    path = os.path.join(d, "syn-idxs.p")
    df = write_df_pickle(path, synthetic_corpus(5000, seed=1, vocab=2000, refs=(5, 6), lengths=(6, 16)))
    scorers = [("CIDEr-D", CiderD(df=path)), ("BLEU-4", Bleu(4)), ("CIDEr-D + BLEU-4", RewardScorer(df=path, cider_weight=1.0, bleu_weight=0.5))]
gts = [np.pad(rng.integers(1, 2000, (5, 12)), ((0, 0), (0, S - 12))) for _ in range(n_img)]
seq_h = np.pad(rng.integers(1, 2000, (n_img * spi, 14)), ((0, 0), (0, S - 14)))
seq = torch.from_numpy(seq_h).cuda()
for name, sc in scorers:
    sc.score(gts, seq, spi); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        sc.score(gts, seq, spi)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / iters * 1e3
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(iters):
        sc.score(gts, seq, spi)
    ev[1].record(); torch.cuda.synchronize()
    print(f"{name}: {n_img} images x {spi} samples x 5 references, S = {S}: score() {wall:.3f} ms per call (wall, incl. host packing), "
          f"stream time {ev[0].elapsed_time(ev[1]) / iters:.3f} ms per call", flush=True)
t0 = time.perf_counter()
want_b = restated_bleu(gts, seq_h, spi)[0]
host_ms = (time.perf_counter() - t0) * 1e3
want_c = restated_scores(gts, seq_h, spi, df, math.log(5000.0))
err_b = float(np.abs(scorers[1][1].score(gts, seq, spi, out64=True)[1].cpu().numpy() - want_b).max())
err_r = float(np.abs(scorers[2][1].score(gts, seq, spi, out64=True)[1].cpu().numpy() - (want_c + 0.5 * want_b)).max())
print(f"float64 host restatement of BLEU {host_ms:.1f} ms; max |device - host| BLEU-4 {err_b:.2e}, combined {err_r:.2e}")
