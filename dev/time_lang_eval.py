#!/usr/bin/env python3
"""Time the validation pass's language scores at 5 000 images x 5 references (boficap_amd.lang_eval.LanguageEval): the construction (host packing of
the references with their corpus document frequencies, upload, records: once per run), one ``evaluate`` (two launches and a read-back), the same scores
with the references packed again on every call (what the scorers cost on their own: Bleu / CiderD('corpus') / Rouge ``compute_score``), and one whole
validation pass of the full-size model (``eval_split``, NAIC through ``decode_many`` and SAIC per batch) with synthetic weights and features.
usage: python dev/time_lang_eval.py [images] [out.txt]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np
import torch

n_img = int(sys.argv[1]) if len(sys.argv) > 1 else 5000
out_path = sys.argv[2] if len(sys.argv) > 2 else ""
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


from boficap_amd.bleu import Bleu
from boficap_amd.cider import CiderD
from boficap_amd.lang_eval import LanguageEval
from boficap_amd.rouge import Rouge, eval_token_list

rng = np.random.default_rng(0)
S, vocab = 20, 9487
gts = []
for _ in range(n_img):
    g = rng.integers(7, vocab, (5, S))
    for row in g:
        row[int(rng.integers(6, 17)):] = 0
    gts.append(g)
seq_h = rng.integers(7, vocab, (n_img, S))
for j, row in enumerate(seq_h):
    row[:6] = gts[j][j % 5][:6]                               # (some overlap with a reference, as a trained model's captions have)
    row[int(rng.integers(6, 17)):] = 0
seq = torch.from_numpy(seq_h).cuda()
torch.cuda.synchronize()

t0 = time.perf_counter()
ev = LanguageEval(gts, "cuda")
torch.cuda.synchronize()
say(f"LanguageEval({n_img} images x 5 references): construction {time.perf_counter() - t0:.3f} s (host packing + corpus df + upload + records; once per run)")
stats = ev.evaluate(seq)
iters = 20
t0 = time.perf_counter()
for _ in range(iters):
    stats = ev.evaluate(seq)
say(f"evaluate(): {(time.perf_counter() - t0) / iters * 1e3:.3f} ms per call (wall: token-rule expression, two launches, read-back, host means)")
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
cl = ((seq <= 0).cumsum(1) == 0).sum(1).to(torch.int32)
e0.record()
for _ in range(iters):
    ev.reward._launch(None, seq, cl, 1, True, True, records=ev.records)
    ev.rouge._launch(ev.pk, seq, cl, 1)
e1.record(); torch.cuda.synchronize()
say(f"  its two launches (bofi_reward_score + bofi_rouge_score): {e0.elapsed_time(e1) / iters:.3f} ms of stream time per call")
say("  " + " ".join(f"{k} {v:.4f}" for k, v in stats.items()))

strs = lambda rows: [" ".join(map(str, eval_token_list(r))) for r in rows]
t0 = time.perf_counter()
g = {i: strs(rows) for i, rows in enumerate(gts)}
r = {i: strs([seq_h[i]]) for i in range(n_img)}
t_str = time.perf_counter() - t0
t0 = time.perf_counter()
b, _ = Bleu(4, device="cuda").compute_score(g, r)
t_b = time.perf_counter() - t0
t0 = time.perf_counter()
c, _ = CiderD("corpus", device="cuda").compute_score(g, [{"image_id": i, "caption": r[i]} for i in range(n_img)])
t_c = time.perf_counter() - t0
t0 = time.perf_counter()
l, _ = Rouge(device="cuda").compute_score(g, r)
t_l = time.perf_counter() - t0
say(f"packing per call (the scorers on their own, each packs the references again): Bleu.compute_score {t_b:.3f} s, CiderD('corpus').compute_score {t_c:.3f} s, "
    f"Rouge.compute_score {t_l:.3f} s (+ {t_str:.3f} s for the id strings); same scores: BLEU {b == [stats[f'Bleu_{k}'] for k in range(1, 5)]}, "
    f"|dCIDEr| {abs(c - stats['CIDEr']):.1e}, |dROUGE_L| {abs(l - stats['ROUGE_L']):.1e}")

# one whole validation pass of the full-size model
import captioning.models as models
from boficap_amd import eval_utils, weights as W
from boficap_amd.config import FULL
opt = FULL.to_opt()
opt.bofi_compute_dtype, opt.bofi_max_batch = torch.bfloat16, 64
model = models.setup(opt)
model.load_state_dict({k: torch.from_numpy(v) for k, v in W.make_state_dict(FULL, 0).items()}, strict=True)
model.cuda().eval()
uniq = W.synthetic_att_feats(min(n_img, 1024), 36, FULL.att_feat_size, seed=1235)
feats = np.concatenate([uniq] * (-(-n_img // len(uniq))))[:n_img]
kw = {"batch_size": 64, "language_eval": 1, "lang_eval": ev}
for mode in ("NAIC", "SAIC"):
    for rep in ("first (graph captures, forks)", "second"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, pred, st = eval_utils.eval_split(model, feats, gts, dict(kw, inference_mode=mode))
        say(f"eval_split {mode}, {n_img} images, no loss pass, {rep}: {time.perf_counter() - t0:.3f} s ({len(pred)} predictions, CIDEr {st['CIDEr']:.4f})")
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
