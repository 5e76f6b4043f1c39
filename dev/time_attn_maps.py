#!/usr/bin/env python3
"""Time one NAIC decode with and without the word-to-region attention output (attn_topk = 3: one extra launch of attn_maps.hip's kernel in the filling pass) on the
full-size bf16 engine at 64 images per launch and at 1 024 (16 batches of 64, q1_group = 64), 36 regions, synthetic features, seeded weights: HIP events around
back-to-back replays of the captured graphs, the forms interleaved block by block on the same device (ids-only decodes, as the pipeline's launches).  Also the whole
map (attn_maps=True, [B, 20, 36] float32 written) beside the top-3.
usage: python dev/time_attn_maps.py [out file] [blocks]"""
import os, sys
args = [a for a in sys.argv[1:] if not a.startswith("--")]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from boficap_amd import weights as W
from boficap_amd.config import FULL as cfg
from boficap_amd.engine import BofiEngine

blocks = int(args[1]) if len(args) > 1 else 10
per_block = 5
eng = BofiEngine(cfg, torch.bfloat16, max_batch=1024, max_regions=36)
eng.load_state_dict(W.make_state_dict(cfg, 0))
feats = torch.from_numpy(W.synthetic_att_feats(1024, 36, cfg.att_feat_size, seed=1235)).cuda().to(torch.bfloat16)
forms = {"plain": {}, "attn_topk=3": {"attn_topk": 3}, "attn_topk=3 + map": {"attn_topk": 3, "attn_maps": True}}
lines = [f"one NAIC decode (ids only, row statistics), full-size bf16 engine, 36 regions; {blocks} interleaved blocks of {per_block} back-to-back graph replays per form, "
         "HIP events; ms per decode: median of the blocks (min .. max)"]
for B, hint in ((64, 1), (1024, 0)):
    att = feats[:B].contiguous()
    eng.set_decodes_in_flight(hint)                              # (64 images: a decode running alone; 1 024: the throughput forms)
    common = dict(want_logprob=False, ids_only=True, row_stats=True, graph=True, q1_group=64 if B > 64 else 0)
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
    lines.append(f"  B = {B:4d} (ids_only_fused {eng.ids_only_fused(B)}, bound_loop_active {eng.bound_loop_active(36)}): " +
                 "; ".join(f"{k} {med[k]:.4f} ({min(ms[k]):.4f} .. {max(ms[k]):.4f})" for k in forms))
    lines.append(f"      attn_topk=3 - plain {(med['attn_topk=3'] - med['plain']) * 1e3:+.1f} us per decode ({(med['attn_topk=3'] / med['plain'] - 1) * 100:+.2f} %); "
                 f"with the map {(med['attn_topk=3 + map'] - med['plain']) * 1e3:+.1f} us ({(med['attn_topk=3 + map'] / med['plain'] - 1) * 100:+.2f} %)")
print("\n".join(lines))
if args and args[0]:
    os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
    with open(args[0], "w") as f:
        f.write("\n".join(lines) + "\n")
