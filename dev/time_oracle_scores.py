#!/usr/bin/env python3
"""Time the oracle scores of sampled captions (boficap_amd.lang_eval.LanguageEval.evaluate_n) at 5 000 images x 5 references, n = 5 samples per
image, S = 20: one ``evaluate_n`` as wall time and as stream time over back-to-back calls, against (a) n calls of ``LanguageEval.evaluate`` on
the strided rows -- what the tree could do before, without sentence-level BLEU -- and (b) the float64 host restatement of
tests/test_oracle_scores.py on the same batch.  usage: python dev/time_oracle_scores.py [iters] [out file] [images]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch
from boficap_amd.lang_eval import LanguageEval
from test_oracle_scores import restated_oracle

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 50
n_img = int(sys.argv[3]) if len(sys.argv) > 3 else 5000
n, S, vocab = 5, 20, 9487
rng = np.random.default_rng(0)
gts = []
for _ in range(n_img):
    g = rng.integers(7, vocab, (5, S))
    for row in g:
        row[int(rng.integers(6, 17)):] = 0
    gts.append(g)
seq_h = rng.integers(7, vocab, (n_img * n, S))
for j, row in enumerate(seq_h):                                  # a sample: the start of one of its image's references, then other words
    m = j // n
    keep = int(rng.integers(2, 10))
    row[:keep] = gts[m][j % 5][:keep]
    row[int(rng.integers(6, 17)):] = 0
seq = torch.from_numpy(seq_h).cuda()
ev = LanguageEval(gts, "cuda")
strided = [seq[i::n].contiguous() for i in range(n)]
torch.cuda.synchronize()


def timed(fn):
    fn(); torch.cuda.synchronize()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t0 = time.perf_counter()
    marks[0].record()
    for _ in range(iters):
        fn()
    marks[1].record(); torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3, marks[0].elapsed_time(marks[1]) / iters


def n_evaluates():
    return [ev.evaluate(rows) for rows in strided]


one_ms, _ = timed(lambda: ev.evaluate_n(seq, n))
_, one_stream = timed(lambda: ev._launch_n(seq, n))
many_ms, _ = timed(n_evaluates)
out = ev.evaluate_n(seq, n)
t0 = time.perf_counter()
want = restated_oracle(gts, seq_h, n)
host_ms = (time.perf_counter() - t0) * 1e3
err = {k: abs(out[k] - want["stats"][k]) for k in out if k != "per_image"}
rounds = n_evaluates()
d_avg = max(abs(float(np.mean([r[k] for r in rounds])) - out[f"avg_{k}"]) for k in ("ROUGE_L", "CIDEr"))
lines = [f"oracle scores, {n_img} images x 5 references, n = {n} samples, S = {S} ({iters} back-to-back calls each):",
         f"  evaluate_n (three launches, one read-back, host means): {one_ms:.3f} ms per call (wall); its launches alone {one_stream:.3f} ms of stream time per call",
         f"  {n} x LanguageEval.evaluate on the strided rows (2 launches and a read-back each; corpus BLEU only, no per-image reduction): {many_ms:.3f} ms (wall)",
         f"  float64 host restatement: {host_ms:.0f} ms",
         f"  one evaluate_n costs no more than the {n} evaluate calls: {'confirmed' if one_ms <= many_ms else 'REFUTED'} ({one_ms / many_ms:.2f} x)",
         f"  max |device - restatement| over the 12 set-level values: BLEU and ROUGE-L {max(v for k, v in err.items() if 'CIDEr' not in k):.2e}, "
         f"CIDEr {max(v for k, v in err.items() if 'CIDEr' in k):.2e}; |avg_M - mean of the {n} evaluate calls| (ROUGE_L, CIDEr) {d_avg:.2e}",
         "  " + " ".join(f"{k} {v:.4f}" for k, v in out.items() if k != "per_image")]
print("\n".join(lines))
if len(sys.argv) > 2 and sys.argv[2]:
    with open(sys.argv[2], "w") as f:
        f.write("\n".join(lines) + "\n")
