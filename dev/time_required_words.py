#!/usr/bin/env python3
"""Time one NAIC decode plain, with no_repeat (bofi_vocab_constrain's two launches) and with require_ids (K = 4 words per image: bofi_vocab_require's one launch behind the
replayed graph, and the small reduction that hands it the live counts), on the full-size bf16 engine with the log-prob tensor kept, at 64 images per launch and at 1 024
(16 batches of 64, q1_group = 64), 36 regions, synthetic features, seeded weights: HIP events around back-to-back calls (the captured graph replayed, the post-pass
enqueued behind it), the forms interleaved block by block on the same device.  Then bofi_vocab_require alone on the decode's own tensor and ids, HIP events around 20
launches.  ``--tree DIR --plain-only`` times the plain decode alone on another checkout (the parent's baseline; alternate the two in one session).  The sibling of
dev/time_trigram_pick.py.
usage: python dev/time_required_words.py [out file] [blocks] [--tree DIR] [--plain-only]"""
import os, sys
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
eng.load_state_dict(W.make_state_dict(cfg, 0))
feats = torch.from_numpy(W.synthetic_att_feats(1024, 36, cfg.att_feat_size, seed=1235)).cuda().to(torch.bfloat16)
S, V, K = cfg.seq_length, cfg.tgt_vocab, 4
lines = [f"one NAIC decode (log-probs kept, row statistics), full-size bf16 engine, 36 regions, tree {os.path.basename(ROOT) if tree else 'this one'}; {blocks} interleaved blocks of {per_block} back-to-back "
         "calls per form (graph replay + what follows it), HIP events; ms per decode: median of the blocks (min .. max)"]
for B, hint in ((64, 1), (1024, 0)):
    att = feats[:B].contiguous()
    eng.set_decodes_in_flight(hint)                              # (64 images: a decode running alone; 1 024: the throughput forms)
    common = dict(want_logprob=True, row_stats=True, graph=True, q1_group=64 if B > 64 else 0)
    forms = {"plain": {}}
    if not plain_only:
        first = eng.decode_naic(att, **common)
        torch.cuda.synchronize()
        # K = 4 words per image: the runner-up ids of four of its live positions (words the decode nearly said), by one rule for every image
        n = first["phrase_length"].sum(1)
        lp = first["seq_logprob"]
        table = torch.full((B, K), -1, dtype=torch.int32, device="cuda")
        for j in range(K):
            p = (n * (2 * j + 1) // (2 * K)).clamp(max=S - 1)
            table[:, j] = lp[torch.arange(B, device="cuda"), p].topk(2, dim=1).indices[:, 1].to(torch.int32)
        table[n == 0] = -1
        forms.update({"no_repeat": {"no_repeat": True}, "require_ids": {"require_ids": table}, "require_ids + no_repeat": {"require_ids": table, "no_repeat": True}})
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
    r = outs["require_ids"]
    lines.append(f"      required words: {int((r['required_pos'] >= 0).sum())} of {int((table >= 0).sum())} placed, {int(r['required_moved'].sum())} positions changed")
    lines.append("      " + "; ".join(f"{k} - plain {(med[k] - med['plain']) * 1e3:+.1f} us per decode ({(med[k] / med['plain'] - 1) * 100:+.2f} %)" for k in forms if k != "plain"))
    # the launch alone on this decode's tensor, and the reduction that makes its live counts
    plain = outs["plain"]
    lpf, seq0 = plain["seq_logprob"].view(B * S, V), plain["seq"].clone().view(-1)
    seq = seq0.clone()
    ntok = plain["phrase_length"].sum(1).to(torch.int32)
    chosen, pos, moved = torch.empty(B * S, device="cuda"), torch.empty(B, K, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")

    def require():
        hip.vocab_require(lpf, V, S, seq, table, pos, ntok=ntok, no_repeat=True, row_chosen=chosen, moved=moved)

    def counts():
        torch.sum(plain["phrase_length"], 1, dtype=torch.int32)

    us = {}
    for name, fn in (("bofi_vocab_require (K = 4, no_repeat)", require), ("live counts (one torch reduction)", counts)):
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
    lines.append(f"      alone on the [{B * S}, {V}] tensor (a wavefront per image, {B * K} words), us per launch incl. the launch gap: " +
                 "; ".join(f"{k} {v[0]:.1f} ({v[1]:.1f} .. {v[2]:.1f})" for k, v in us.items()))
print("\n".join(lines))
if args and args[0]:
    os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
    with open(args[0], "w") as f:
        f.write("\n".join(lines) + "\n")
