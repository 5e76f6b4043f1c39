#!/usr/bin/env python3
"""Time one NAIC decode with T = 3 refinement rounds in both methods -- feed-back and mask-predict -- on the full-size bf16 engine at B = 64 and B = 256
(36 regions, synthetic features, seeded weights): HIP events around back-to-back decodes, the two methods interleaved block by block on the same device,
eager launches and replayed graphs, plus the plain decode (T = 0) for scale.  Expectation: a mask-predict round costs a feed-back round plus one step launch.
usage: python dev/time_mask_predict.py [out file] [blocks] [--tree DIR] [--feed-back-only]
  --tree DIR          import boficap_amd from DIR instead of this checkout (a checkout of the parent commit: the feed-back baseline)
  --feed-back-only    only what a tree without mask-predict can run"""
import os, sys
args = [a for a in sys.argv[1:] if not a.startswith("--")]
tree = sys.argv[sys.argv.index("--tree") + 1] if "--tree" in sys.argv else None
if tree:
    args.remove(tree)
ROOT = os.path.abspath(tree) if tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from boficap_amd import weights as W
from boficap_amd.config import FULL as cfg
from boficap_amd.engine import BofiEngine

blocks = int(args[1]) if len(args) > 1 else 10
per_block, T = 5, 3
fb_only = "--feed-back-only" in sys.argv
eng = BofiEngine(cfg, torch.bfloat16, max_batch=256, max_regions=36)
eng.load_state_dict(W.make_state_dict(cfg, 0))
eng.set_decodes_in_flight(1)
feats = torch.from_numpy(W.synthetic_att_feats(256, 36, cfg.att_feat_size, seed=1235)).cuda().to(torch.bfloat16)
forms = {"plain (T = 0)": {}, "feed-back": {"refine_rounds": T}}
if not fb_only:
    forms["mask-predict"] = {"refine_rounds": T, "refine_method": "mask_predict"}
lines = [f"one NAIC decode, full-size bf16 engine, 36 regions, T = {T}; {blocks} interleaved blocks of {per_block} back-to-back decodes per form, HIP events; ms per decode: median of the blocks (min .. max)"
         + (f"  [tree: {ROOT}]" if tree else "")]
for B in (64, 256):
    att = feats[:B].contiguous()
    for graph in (False, True):
        outs = {k: None for k in forms}
        for k, kw in forms.items():                              # warm-up, graph capture
            for _ in range(3):
                outs[k] = eng.decode_naic(att, want_logprob=False, graph=graph, out=outs[k], **kw)
        torch.cuda.synchronize()
        ms = {k: [] for k in forms}
        for _ in range(blocks):
            for k, kw in forms.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(per_block):
                    outs[k] = eng.decode_naic(att, want_logprob=False, graph=graph, out=outs[k], **kw)
                b.record()
                b.synchronize()
                ms[k].append(a.elapsed_time(b) / per_block)
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        lines.append(f"  B = {B:3d}, {'replayed graph' if graph else 'eager launches'}: " + "; ".join(f"{k} {med[k]:.3f} ({min(ms[k]):.3f} .. {max(ms[k]):.3f})" for k in forms))
        if not fb_only:
            per_round_fb = (med["feed-back"] - med["plain (T = 0)"]) / T
            lines.append(f"      per extra round: feed-back {per_round_fb * 1e3:.1f} us, mask-predict {(med['mask-predict'] - med['plain (T = 0)']) / T * 1e3:.1f} us; "
                         f"mask-predict - feed-back per decode {(med['mask-predict'] - med['feed-back']) * 1e3:+.1f} us ({T + 1} step launches)")
print("\n".join(lines))
if args and args[0]:
    os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
    with open(args[0], "w") as f:
        f.write("\n".join(lines) + "\n")
