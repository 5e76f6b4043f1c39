#!/usr/bin/env python3
"""Time one NAIC decode plain, with nbest = 5 and with nbest = 8 (bofi_vocab_nbest's two launches behind the replayed graph, and the small reduction that hands them the
live counts), on the full-size bf16 engine with the log-prob tensor kept, at 64 images per launch and at 1 024 (16 batches of 64, q1_group = 64), 36 regions, synthetic
features, seeded weights: HIP events around back-to-back calls, the forms interleaved block by block on the same device.  Then bofi_vocab_nbest alone on the decode's own
tensor, HIP events around 20 calls.  Then what five captions per image cost through ``mode='sample'`` at 64 images: ``sample_n = 5`` sampled captions against one greedy
decode with ``opt['nbest'] = 5`` (wall clock around the synchronised calls).  ``--tree DIR --plain-only`` times the plain decode alone on another checkout (the parent's
baseline; alternate the two in one session).  The sibling of dev/time_required_words.py.
usage: python dev/time_nbest.py [out file] [blocks] [--tree DIR] [--plain-only]"""
import os, sys, time
argv = sys.argv[1:]
tree = argv[argv.index("--tree") + 1] if "--tree" in argv else None
plain_only = "--plain-only" in argv
args = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] != "--tree")]
ROOT = os.path.abspath(tree) if tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from boficap_amd import hip, weights as W
from boficap_amd.config import FULL as cfg
from boficap_amd.engine import BofiEngine

blocks = int(args[1]) if len(args) > 1 else 10
per_block = 5
eng = BofiEngine(cfg, torch.bfloat16, max_batch=1024, max_regions=36)
sd = W.make_state_dict(cfg, 0)
eng.load_state_dict(sd)
feats = torch.from_numpy(W.synthetic_att_feats(1024, 36, cfg.att_feat_size, seed=1235)).cuda().to(torch.bfloat16)
S, V = cfg.seq_length, cfg.tgt_vocab
lines = [f"one NAIC decode (log-probs kept, row statistics), full-size bf16 engine, 36 regions, tree {os.path.basename(ROOT) if tree else 'this one'}; {blocks} interleaved blocks of {per_block} back-to-back "
         "calls per form (graph replay + what follows it), HIP events; ms per decode: median of the blocks (min .. max)"]
for B, hint in ((64, 1), (1024, 0)):
    att = feats[:B].contiguous()
    eng.set_decodes_in_flight(hint)                              # (64 images: a decode running alone; 1 024: the throughput forms)
    common = dict(want_logprob=True, row_stats=True, graph=True, q1_group=64 if B > 64 else 0)
    forms = {"plain": {}}
    if not plain_only:
        forms.update({"nbest=5": {"nbest": 5}, "nbest=8": {"nbest": 8}})
    outs = {k: None for k in forms}
    for k, kw in forms.items():                                  # warm-up, graph capture
        for _ in range(3):
            outs[k] = eng.decode_naic(att, out=outs[k], **common, **kw)
    torch.cuda.synchronize()
    ms = {k: [] for k in forms}
    for _ in range(blocks):
        for k, kw in forms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(per_block):
                outs[k] = eng.decode_naic(att, out=outs[k], **common, **kw)
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / per_block)
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    live = int(outs["plain"]["phrase_length"].sum())
    lines.append(f"  B = {B:4d} (bound_loop_active {eng.bound_loop_active(36)}; {live} live positions of {B * S}): " +
                 "; ".join(f"{k} {med[k]:.4f} ({min(ms[k]):.4f} .. {max(ms[k]):.4f})" for k in forms))
    if plain_only:
        continue
    r = outs["nbest=8"]
    lines.append(f"      lists of 8: {int((r['nbest_count'] == 8).sum())} of {B} images full, entry 0 equals the caption on {int((r['nbest_seq'][:, 0] == r['seq']).all(1).sum())} images; "
                 f"mean log-prob gap from entry 0 to entry 7: {float((r['nbest_logp'][:, 0] - r['nbest_logp'][:, 7])[r['nbest_count'] == 8].mean()):.4f}")
    lines.append("      " + "; ".join(f"{k} - plain {(med[k] - med['plain']) * 1e3:+.1f} us per decode ({(med[k] / med['plain'] - 1) * 100:+.2f} %)" for k in forms if k != "plain"))
    # the two launches alone on this decode's tensor, and the reduction that makes its live counts
    plain = outs["plain"]
    lpf = plain["seq_logprob"].view(B * S, V)
    ntok = plain["phrase_length"].sum(1).to(torch.int32)
    bufs = {N: (torch.empty(B, N, S, dtype=torch.int64, device="cuda"), torch.empty(B, N, dtype=torch.float64, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda"))
            for N in (5, 8)}
    work = torch.empty(B * S * 8, dtype=torch.int32, device="cuda")

    def nbest(N):
        hip.vocab_nbest(lpf, V, S, N, ntok=ntok, pad_idx=cfg.pad_idx, seq_n=bufs[N][0], total=bufs[N][1], count=bufs[N][2], work=work)

    def counts():
        torch.sum(plain["phrase_length"], 1, dtype=torch.int32)

    us = {}
    for name, fn in (("bofi_vocab_nbest N = 5", lambda: nbest(5)), ("bofi_vocab_nbest N = 8", lambda: nbest(8)), ("live counts (one torch reduction)", counts)):
        for _ in range(3):
            fn()
        t = []
        for _ in range(blocks):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(20):
                fn()
            b.record()
            b.synchronize()
            t.append(a.elapsed_time(b) / 20 * 1e3)
        us[name] = (sorted(t)[len(t) // 2], min(t), max(t))
    lines.append(f"      alone on the [{B * S}, {V}] tensor (candidates launch + a wavefront per image), us per call incl. the launch gaps: " +
                 "; ".join(f"{k} {v[0]:.1f} ({v[1]:.1f} .. {v[2]:.1f})" for k, v in us.items()))
if not plain_only:
    # five captions per image through mode='sample', 64 images: sample_n = 5 draws against one decode with the list
    import captioning.models as models
    opt = cfg.to_opt()
    opt.bofi_compute_dtype, opt.bofi_max_batch, opt.bofi_max_regions = torch.bfloat16, 320, 36
    model = models.setup(opt)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    model.cuda().eval()
    att, fc = feats[:64].contiguous(), torch.zeros(64, 0, device="cuda")
    forms = {"greedy": {"train_mode": "NAIC"}, "greedy + nbest=5": {"train_mode": "NAIC", "nbest": 5},
             "sample_method='sample', sample_n=5": {"train_mode": "NAIC", "sample_method": "sample", "sample_n": 5}}
    wall = {k: [] for k in forms}
    with torch.no_grad():
        for k, o in forms.items():
            for _ in range(3):
                model(fc, att, None, opt=o, mode="sample")
        for _ in range(blocks):
            for k, o in forms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(per_block):
                    model(fc, att, None, opt=o, mode="sample")
                torch.cuda.synchronize()
                wall[k].append((time.perf_counter() - t0) / per_block * 1e3)
    lines.append("  five captions per image through mode='sample', 64 images (wall clock around the synchronised calls, ms per call: median (min .. max)): " +
                 "; ".join(f"{k} {sorted(v)[len(v) // 2]:.4f} ({min(v):.4f} .. {max(v):.4f})" for k, v in wall.items()))
print("\n".join(lines))
if args and args[0]:
    os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
    with open(args[0], "w") as f:
        f.write("\n".join(lines) + "\n")
