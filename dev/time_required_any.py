#!/usr/bin/env python3
"""Time bofi_vocab_require_any (required alternatives) against bofi_vocab_require_units (required phrases) and the plain decode, on the full-size bf16 engine with the
log-prob tensor kept, at 64 images per launch and at 1 024 (16 batches of 64, q1_group = 64), 36 regions, synthetic features, seeded weights, ONE process.
  the launch alone   on the decode's own tensor and ids, HIP events around 20 launches, for (K, A, L) = (4, 1, 2), (4, 2, 2), (8, 1, 4), (8, 4, 4), with
                     bofi_vocab_require_units at the same K, L beside it (at A = 1 the two do the same work)
  the decode         plain, require_phrases (the first alternatives only) and require_any for (K, A, L) = (4, 2, 2) and (8, 4, 4): HIP events around back-to-back calls
                     (the captured graph replayed, the post-pass enqueued behind it), the forms interleaved block by block
The sibling of dev/time_required_phrases.py.
usage: python dev/time_required_any.py [out file] [blocks]"""
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
ALONE = ((4, 1, 2), (4, 2, 2), (8, 1, 4), (8, 4, 4))             # (K groups, alternatives per group, ids per alternative)
DECODE = ((4, 2, 2), (8, 4, 4))
lines = [f"required alternatives, full-size bf16 engine, 36 regions, log-probs kept, row statistics; {blocks} blocks, HIP events, one process; median of the blocks (min .. max)"]
for B, hint in ((64, 1), (1024, 0)):
    att = feats[:B].contiguous()
    eng.set_decodes_in_flight(hint)                              # (64 images: a decode running alone; 1 024: the throughput forms)
    common = dict(want_logprob=True, row_stats=True, graph=True, q1_group=64 if B > 64 else 0)
    first = eng.decode_naic(att, **common)
    torch.cuda.synchronize()
    n, lp = first["phrase_length"].sum(1), first["seq_logprob"]
    best = lp.topk(5, dim=2).indices.to(torch.int32)             # [B, S, 5]: alternative a of a group holds the (a + 2)-th best ids of L neighbouring positions
    tables = {}
    for K, A, L in ALONE:                                        # group j starts at position n (2j + 1) / 2K
        t = torch.full((B, K, A, L), -1, dtype=torch.int32, device="cuda")
        for j in range(K):
            p = n * (2 * j + 1) // (2 * K)
            for a in range(A):
                for i in range(L):
                    t[:, j, a, i] = best[torch.arange(B, device="cuda"), (p + i).clamp(max=S - 1), a + 1]
        t[n == 0] = -1
        tables[(K, A, L)] = t
    forms = {"plain": {}}
    for K, A, L in DECODE:
        forms[f"require_phrases K={K} L={L}"] = {"require_phrases": tables[(K, A, L)][:, :, 0].contiguous()}
        forms[f"require_any K={K} A={A} L={L}"] = {"require_any": tables[(K, A, L)]}
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
    lines.append(f"  B = {B:4d} (bound_loop_active {eng.bound_loop_active(36)}; {live} live positions of {B * S}), ms per decode: " +
                 "; ".join(f"{k} {med[k]:.4f} ({min(ms[k]):.4f} .. {max(ms[k]):.4f})" for k in forms))
    for K, A, L in DECODE:
        r, u = outs[f"require_any K={K} A={A} L={L}"], outs[f"require_phrases K={K} L={L}"]
        alt = r["required_alt"]
        lines.append(f"      K={K} A={A} L={L}: {int((r['required_pos'] >= 0).sum())} of {B * K} groups placed, by alternative {[int((alt == a).sum()) for a in range(A)]}, "
                     f"{int(r['required_moved'].sum())} positions changed (require_phrases, first alternatives only: {int((u['required_pos'] >= 0).sum())} units placed, "
                     f"{int(u['required_moved'].sum())} changed)")
    lines.append("      " + "; ".join(f"{k} - plain {(med[k] - med['plain']) * 1e3:+.1f} us per decode ({(med[k] / med['plain'] - 1) * 100:+.2f} %)" for k in forms if k != "plain"))
    lines.append("      " + "; ".join(f"require_any K={K} A={A} L={L} - require_phrases K={K} L={L} {(med[f'require_any K={K} A={A} L={L}'] - med[f'require_phrases K={K} L={L}']) * 1e3:+.1f} us"
                                      for K, A, L in DECODE))
    # the launches alone on this decode's tensor
    plain = outs["plain"]
    lpf, seq = plain["seq_logprob"].view(B * S, V), plain["seq"].clone().view(-1)
    ntok = plain["phrase_length"].sum(1).to(torch.int32)
    chosen, moved = torch.empty(B * S, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
    calls = []
    for K, A, L in ALONE:
        t, pos, which = tables[(K, A, L)], torch.empty(B, K, dtype=torch.int32, device="cuda"), torch.empty(B, K, dtype=torch.int32, device="cuda")
        units = t[:, :, 0].contiguous()
        if A == 1:
            calls.append((f"bofi_vocab_require_units K={K} L={L}", lambda units=units, pos=pos: hip.vocab_require_units(lpf, V, S, seq, units, pos, ntok=ntok, row_chosen=chosen, moved=moved)))
        calls.append((f"bofi_vocab_require_any K={K} A={A} L={L}", lambda t=t, pos=pos, which=which: hip.vocab_require_any(lpf, V, S, seq, t, pos, which, ntok=ntok, row_chosen=chosen, moved=moved)))
    us = {}
    for rnd in range(2):                                         # two rounds over all calls: the second is reported, the first shows the run-to-run spread
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
            us.setdefault(name, []).append((sorted(t)[len(t) // 2], min(t), max(t)))
    lines.append(f"      alone on the [{B * S}, {V}] tensor, us per launch incl. the launch gap, second round (first round's median in brackets):")
    for k, v in us.items():
        lines.append(f"        {k}: {v[1][0]:.1f} ({v[1][1]:.1f} .. {v[1][2]:.1f}) [{v[0][0]:.1f}]")
print("\n".join(lines))
if args and args[0]:
    os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
    with open(args[0], "w") as f:
        f.write("\n".join(lines) + "\n")
