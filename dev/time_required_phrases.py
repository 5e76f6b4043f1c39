#!/usr/bin/env python3
"""Time one NAIC decode plain, with require_ids (bofi_vocab_require, K = 4 and K = 8 words per image) and with require_phrases (bofi_vocab_require_units: K = 4 units of 2
ids, K = 8 units of 4 ids), on the full-size bf16 engine with the log-prob tensor kept, at 64 images per launch and at 1 024 (16 batches of 64, q1_group = 64), 36
regions, synthetic features, seeded weights: HIP events around back-to-back calls (the captured graph replayed, the post-pass enqueued behind it), the forms interleaved
block by block in ONE process.  Then the two kernels alone on the decode's own tensor and ids, HIP events around 20 launches.  The sibling of dev/time_required_words.py.
usage: python dev/time_required_phrases.py [out file] [blocks]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from boficap_amd import hip, weights as W
from boficap_amd.config import FULL as cfg
from boficap_amd.engine import BofiEngine

args = sys.argv[1:]
blocks = int(args[1]) if len(args) > 1 else 8
per_block = 5
eng = BofiEngine(cfg, torch.bfloat16, max_batch=1024, max_regions=36)
eng.load_state_dict(W.make_state_dict(cfg, 0))
feats = torch.from_numpy(W.synthetic_att_feats(1024, 36, cfg.att_feat_size, seed=1235)).cuda().to(torch.bfloat16)
S, V = cfg.seq_length, cfg.tgt_vocab
SHAPES = ((4, 2), (8, 4))                                        # (K units, ids per unit)
lines = [f"one NAIC decode (log-probs kept, row statistics), full-size bf16 engine, 36 regions; {blocks} interleaved blocks of {per_block} back-to-back calls per form "
         "(graph replay + what follows it), HIP events, one process; ms per decode: median of the blocks (min .. max)"]
for B, hint in ((64, 1), (1024, 0)):
    att = feats[:B].contiguous()
    eng.set_decodes_in_flight(hint)                              # (64 images: a decode running alone; 1 024: the throughput forms)
    common = dict(want_logprob=True, row_stats=True, graph=True, q1_group=64 if B > 64 else 0)
    first = eng.decode_naic(att, **common)
    torch.cuda.synchronize()
    n, lp = first["phrase_length"].sum(1), first["seq_logprob"]
    runner = lp.topk(2, dim=2).indices[:, :, 1].to(torch.int32)  # [B, S]: the id every position nearly said
    forms, tables = {"plain": {}}, {}
    for K, L in SHAPES:                                          # unit j: the runner-up ids of L neighbouring positions from n (2j + 1) / 2K on; require_ids: their first ids
        units = torch.full((B, K, L), -1, dtype=torch.int32, device="cuda")
        for j in range(K):
            p = n * (2 * j + 1) // (2 * K)
            for i in range(L):
                units[:, j, i] = runner[torch.arange(B, device="cuda"), (p + i).clamp(max=S - 1)]
        units[n == 0] = -1
        tables[(K, L)] = units
        forms[f"require_ids K={K}"] = {"require_ids": units[:, :, 0].contiguous()}
        forms[f"require_phrases K={K} L={L}"] = {"require_phrases": units}
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
    for K, L in SHAPES:
        r, w = outs[f"require_phrases K={K} L={L}"], outs[f"require_ids K={K}"]
        lines.append(f"      K={K} L={L}: {int((r['required_pos'] >= 0).sum())} of {B * K} units placed, {int(r['required_moved'].sum())} positions changed "
                     f"(require_ids K={K}: {int((w['required_pos'] >= 0).sum())} words placed, {int(w['required_moved'].sum())} changed)")
    lines.append("      " + "; ".join(f"{k} - plain {(med[k] - med['plain']) * 1e3:+.1f} us per decode ({(med[k] / med['plain'] - 1) * 100:+.2f} %)" for k in forms if k != "plain"))
    lines.append("      " + "; ".join(f"require_phrases K={K} L={L} - require_ids K={K} {(med[f'require_phrases K={K} L={L}'] - med[f'require_ids K={K}']) * 1e3:+.1f} us" for K, L in SHAPES))
    # the launches alone on this decode's tensor
    plain = outs["plain"]
    lpf, seq = plain["seq_logprob"].view(B * S, V), plain["seq"].clone().view(-1)
    ntok = plain["phrase_length"].sum(1).to(torch.int32)
    chosen, moved = torch.empty(B * S, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
    calls = []
    for K, L in SHAPES:
        units, pos = tables[(K, L)], torch.empty(B, K, dtype=torch.int32, device="cuda")
        words = units[:, :, 0].contiguous()
        calls.append((f"bofi_vocab_require K={K}", lambda words=words, pos=pos: hip.vocab_require(lpf, V, S, seq, words, pos, ntok=ntok, row_chosen=chosen, moved=moved)))
        calls.append((f"bofi_vocab_require_units K={K} L={L}", lambda units=units, pos=pos: hip.vocab_require_units(lpf, V, S, seq, units, pos, ntok=ntok, row_chosen=chosen, moved=moved)))
    calls.append(("live counts (one torch reduction)", lambda: torch.sum(plain["phrase_length"], 1, dtype=torch.int32)))
    us = {}
    for name, fn in calls:
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
    lines.append(f"      alone on the [{B * S}, {V}] tensor (a wavefront per image), us per launch incl. the launch gap: " + "; ".join(f"{k} {v[0]:.1f} ({v[1]:.1f} .. {v[2]:.1f})" for k, v in us.items()))
print("\n".join(lines))
if args and args[0]:
    os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
    with open(args[0], "w") as f:
        f.write("\n".join(lines) + "\n")
