#!/usr/bin/env python3
"""Time the device CIDEr-D scorer (boficap_amd.cider.CiderD.score) at 64 images x 5 samples x 5 references, S = 20, and the float64 host
restatement of tests/test_cider.py on the same batch for comparison.  usage: python dev/time_cider.py [iters]"""
import math, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch
from boficap_amd.cider import CiderD
from test_cider import restated_scores, synthetic_corpus, write_df_pickle

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 50
rng = np.random.default_rng(0)
n_img, spi, S, vocab = 64, 5, 20, 9487
with tempfile.TemporaryDirectory() as d:
    path = os.path.join(d, "syn-idxs.p")
    df = write_df_pickle(path, synthetic_corpus(5000, seed=1, vocab=2000, refs=(5, 6), lengths=(6, 16)))
    sc = CiderD(df=path)
gts = [np.pad(rng.integers(1, 2000, (5, 12)), ((0, 0), (0, S - 12))) for _ in range(n_img)]
seq_h = np.pad(rng.integers(1, 2000, (n_img * spi, 14)), ((0, 0), (0, S - 14)))
seq = torch.from_numpy(seq_h).cuda()
out = sc.score(gts, seq, spi); torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(iters):
    out = sc.score(gts, seq, spi)
torch.cuda.synchronize()
dev_ms = (time.perf_counter() - t0) / iters * 1e3
# the kernels alone (host packing excluded): events around the two launches of one call
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
ev[0].record()
for _ in range(iters):
    sc.score(gts, seq, spi)
ev[1].record(); torch.cuda.synchronize()
t0 = time.perf_counter()
want = restated_scores(gts, seq_h, spi, df, math.log(5000.0))
host_ms = (time.perf_counter() - t0) * 1e3
err = float(np.abs(sc.score(gts, seq, spi, out64=True)[1].cpu().numpy() - want).max())
print(f"CIDEr-D {n_img} images x {spi} samples x 5 references, S = {S}: device score() {dev_ms:.3f} ms per call (wall, incl. host packing), "
      f"stream time {ev[0].elapsed_time(ev[1]) / iters:.3f} ms per call; float64 host restatement {host_ms:.1f} ms; max |device - host| {err:.2e}")
