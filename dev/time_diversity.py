#!/usr/bin/env python3
"""Time the device self-CIDEr score (boficap_amd.diversity.SelfCider.score) at 64 images x 5 samples, S = 20, and DiversityEval.evaluate at the
same size, against the float64 host restatement of tests/test_diversity.py on the same batch.  usage: python dev/time_diversity.py [iters] [out file]"""
import math, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch
from boficap_amd.diversity import DiversityEval, SelfCider
from test_cider import synthetic_corpus, write_df_pickle
from test_diversity import restated_diversity

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 200
rng = np.random.default_rng(0)
n_img, n, S = 64, 5, 20
with tempfile.TemporaryDirectory() as d:
    path = os.path.join(d, "syn-idxs.p")
    df = write_df_pickle(path, synthetic_corpus(5000, seed=1, vocab=2000, refs=(5, 6), lengths=(6, 16)))
    sc, ev = SelfCider(path), DiversityEval(path)
base = rng.integers(1, 2000, (n_img, 14))                        # the samples of an image: one caption with about a third of its words redrawn
seq_h = np.repeat(base, n, axis=0)
swap = rng.random(seq_h.shape) < 0.35
seq_h[swap] = rng.integers(1, 2000, int(swap.sum()))
seq_h = np.pad(seq_h, ((0, 0), (0, S - 14)))
seq = torch.from_numpy(seq_h).cuda()


def timed(fn):
    fn(); torch.cuda.synchronize()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t0 = time.perf_counter()
    marks[0].record()
    for _ in range(iters):
        fn()
    marks[1].record(); torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3, marks[0].elapsed_time(marks[1]) / iters


score_ms, score_stream = timed(lambda: sc.score(seq, n))
eval_ms, _ = timed(lambda: ev.evaluate(seq, n, "reward"))
t0 = time.perf_counter()
want = restated_diversity(seq_h, n, df, math.log(5000.0), "reward")
host_ms = (time.perf_counter() - t0) * 1e3
err = float(np.abs(sc.score(seq, n).cpu().numpy() - want["score"]).max())
line = (f"self-CIDEr {n_img} images x {n} samples, S = {S}: device score() {score_ms:.3f} ms per call (wall), stream time {score_stream:.3f} ms per call; "
        f"DiversityEval.evaluate (launch + read-back + host statistics) {eval_ms:.3f} ms per call; float64 host restatement {host_ms:.1f} ms; "
        f"max |device - host| on the score {err:.2e}")
print(line)
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        f.write(line + "\n")
