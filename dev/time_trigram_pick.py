#!/usr/bin/env python3
"""Time one NAIC decode plain, with no_repeat (bofi_vocab_constrain's two launches), with no_repeat + block_trigrams and with block_trigrams alone (bofi_vocab_pick's two
launches: K candidates per row, the scan with the trigram rule), on the full-size bf16 engine with the log-prob tensor kept, at 64 images per launch and at 1 024 (16 batches
of 64, q1_group = 64), 36 regions, synthetic features, seeded weights: HIP events around back-to-back replays of the captured graphs, the forms interleaved block by block on
the same device.  Then the two picks alone on the decode's own tensor and ids: bofi_vocab_pick (no_repeat + block_trigrams, and block_trigrams = 0) against
bofi_vocab_constrain (no_repeat), HIP events around 20 calls each.  The sibling of dev/time_constrained_pick.py.
usage: python dev/time_trigram_pick.py [out file] [blocks]"""
import os, sys
args = [a for a in sys.argv[1:] if not a.startswith("--")]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
S, V = cfg.seq_length, cfg.tgt_vocab
K = hip.lib().bofi_vocab_pick_workspace(1) // 4
lines = [f"one NAIC decode (log-probs kept, row statistics), full-size bf16 engine, 36 regions, K = {K} candidates per row; {blocks} interleaved blocks of {per_block} back-to-back "
         "graph replays per form, HIP events; ms per decode: median of the blocks (min .. max)"]
for B, hint in ((64, 1), (1024, 0)):
    att = feats[:B].contiguous()
    eng.set_decodes_in_flight(hint)                              # (64 images: a decode running alone; 1 024: the throughput forms)
    common = dict(want_logprob=True, row_stats=True, graph=True, q1_group=64 if B > 64 else 0)
    forms = {"plain": {}, "no_repeat": {"no_repeat": True}, "no_repeat + trigrams": {"no_repeat": True, "block_trigrams": True}, "trigrams": {"block_trigrams": True}}
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
    n = int(outs["plain"]["phrase_length"].sum())
    # how deep the rule reaches: the place of every emitted id in its row's order (ties by id), on the host
    lp = outs["no_repeat + trigrams"]["seq_logprob"]
    ids = outs["no_repeat + trigrams"]["seq"]
    v = lp.gather(2, ids.unsqueeze(2))
    col = torch.arange(V, device="cuda").view(1, 1, V)
    rank = 1 + ((lp > v) | ((lp == v) & (col < ids.unsqueeze(2)))).sum(2)
    live = torch.arange(S, device="cuda")[None, :] < outs["plain"]["phrase_length"].sum(1)[:, None]
    rank = rank[live]
    lines.append(f"  B = {B:4d} (bound_loop_active {eng.bound_loop_active(36)}; {n} live positions of {B * S}; re-picked: " +
                 ", ".join(f"{k} {int(outs[k]['constrained'].sum())}" for k in forms if k != "plain") +
                 f"; under no_repeat + trigrams {int((rank > 2).sum())} picks lie behind the row's 2nd best, {int((rank > K).sum())} behind its {K}th (rows read again), deepest {int(rank.max())}): " +
                 "; ".join(f"{k} {med[k]:.4f} ({min(ms[k]):.4f} .. {max(ms[k]):.4f})" for k in forms))
    lines.append("      " + "; ".join(f"{k} - plain {(med[k] - med['plain']) * 1e3:+.1f} us per decode ({(med[k] / med['plain'] - 1) * 100:+.2f} %)" for k in forms if k != "plain"))
    lines.append(f"      increment of no_repeat + trigrams over that of no_repeat: {(med['no_repeat + trigrams'] - med['plain']) / (med['no_repeat'] - med['plain']):.2f} x; "
                 f"of trigrams alone: {(med['trigrams'] - med['plain']) / (med['no_repeat'] - med['plain']):.2f} x")
    # the picks alone on this decode's tensor
    plain = outs["plain"]
    lpf, seq0 = plain["seq_logprob"].view(B * S, V), plain["seq"].clone().view(-1)
    seq = seq0.clone()
    ntok = (plain["phrase_length"].sum(1) + 1).to(torch.int32)
    chosen = torch.empty(B * S, device="cuda")
    changed_d = torch.empty(B, dtype=torch.int32, device="cuda")
    work = torch.empty(hip.lib().bofi_vocab_pick_workspace(B * S) // 4, dtype=torch.int32, device="cuda")
    kw = dict(ntok=ntok, ntok_bias=-1, pad_idx=cfg.pad_idx, row_chosen=chosen, changed=changed_d)

    def constrain():
        hip.vocab_constrain(lpf, V, S, seq, no_repeat=True, **kw)

    def pick_off():
        hip.vocab_pick(lpf, V, S, seq, no_repeat=True, block_trigrams=False, work=work, **kw)

    def pick_on():
        hip.vocab_pick(lpf, V, S, seq, no_repeat=True, block_trigrams=True, work=work, **kw)

    us = {}
    for name, fn in (("bofi_vocab_constrain (no_repeat)", constrain), (f"bofi_vocab_pick (no_repeat, K = {K})", pick_off), (f"bofi_vocab_pick (no_repeat + trigrams, K = {K})", pick_on)):
        for _ in range(3):
            seq.copy_(seq0)
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
    lines.append(f"      alone on the [{B * S}, {V}] tensor (the {n} live rows, {n * V * 4 / 1e6:.1f} MB, a workgroup each; the scan a wavefront per image), us per call of two launches incl. "
                 "the launch gaps: " + "; ".join(f"{k} {v[0]:.1f} ({v[1]:.1f} .. {v[2]:.1f})" for k, v in us.items()))
print("\n".join(lines))
if args and args[0]:
    os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
    with open(args[0], "w") as f:
        f.write("\n".join(lines) + "\n")
