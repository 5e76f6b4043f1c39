#!/usr/bin/env python3
"""Time one NAIC decode with and without the constrained pick (ban_ids = one id, no_repeat: constrain.hip's two launches behind the vocabulary epilogue)
on the full-size bf16 engine with the log-prob tensor kept (want_logprob), at 64 images per launch and at 1 024 (16 batches of 64, q1_group = 64), 36 regions,
synthetic features, seeded weights: HIP events around back-to-back replays of the captured graphs, the forms interleaved block by block on the same device.  Then the
two kernels that stream that tensor once, alone on the decode's own tensor and ids: bofi_vocab_constrain against bofi_vocab_stats, HIP events around 20 launches each.
A kernel-stats profile of this script gives the kernels' own durations.
usage: python dev/time_constrained_pick.py [out file] [blocks]"""
import os, sys
args = [a for a in sys.argv[1:] if not a.startswith("--")]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
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
lines = [f"one NAIC decode (log-probs kept, row statistics), full-size bf16 engine, 36 regions; {blocks} interleaved blocks of {per_block} back-to-back graph replays per form, "
         "HIP events; ms per decode: median of the blocks (min .. max)"]
for B, hint in ((64, 1), (1024, 0)):
    att = feats[:B].contiguous()
    eng.set_decodes_in_flight(hint)                              # (64 images: a decode running alone; 1 024: the throughput forms)
    common = dict(want_logprob=True, row_stats=True, graph=True, q1_group=64 if B > 64 else 0)
    plain = eng.decode_naic(att, **common)
    torch.cuda.synchronize()
    live = plain["seq"][plain["seq"] >= 7]
    ids, counts = torch.unique(live, return_counts=True)
    top = int(ids[counts.argmax()])
    forms = {"plain": {}, "no_repeat": {"no_repeat": True}, "ban + no_repeat": {"ban_ids": [top], "no_repeat": True}}
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
    n = int(plain["phrase_length"].sum())
    changed = int(outs["ban + no_repeat"]["constrained"].sum())
    lines.append(f"  B = {B:4d} (bound_loop_active {eng.bound_loop_active(36)}; {n} live positions of {B * S}, {changed} re-picked under ban + no_repeat): " +
                 "; ".join(f"{k} {med[k]:.4f} ({min(ms[k]):.4f} .. {max(ms[k]):.4f})" for k in forms))
    lines.append("      " + "; ".join(f"{k} - plain {(med[k] - med['plain']) * 1e3:+.1f} us per decode ({(med[k] / med['plain'] - 1) * 100:+.2f} %), "
                                      f"{B / med[k] * 1e3:.0f} against {B / med['plain'] * 1e3:.0f} images/s" for k in forms if k != "plain"))
    # the two kernels alone on this decode's tensor
    lp, seq = outs["plain"]["seq_logprob"].view(B * S, V), outs["plain"]["seq"].clone().view(-1)
    ntok = (plain["phrase_length"].sum(1) + 1).to(torch.int32)
    ban = hip.ban_bits([top], V, "cuda")
    plogp, chosen = torch.empty(B * S, device="cuda"), torch.empty(B * S, device="cuda")
    changed_d = torch.empty(B, dtype=torch.int32, device="cuda")

    def stats():
        hip.check(hip.lib().bofi_vocab_stats(hip.ptr(lp), hip.ptr(seq), B * S, V, hip.ptr(plogp), hip.ptr(chosen), hip.stream_ptr()))

    def constrain():
        hip.vocab_constrain(lp, V, S, seq, ntok=ntok, ntok_bias=-1, pad_idx=cfg.pad_idx, ban=ban, no_repeat=True, row_chosen=chosen, changed=changed_d)

    us = {}
    for name, fn in (("bofi_vocab_stats", stats), ("bofi_vocab_constrain", constrain)):
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
    lines.append(f"      alone on the [{B * S}, {V}] tensor ({B * S * V * 4 / 1e6:.1f} MB; the pick reads the {n} live rows, {n * V * 4 / 1e6:.1f} MB, a workgroup each), us per call incl. "
                 "the launch gaps: " + "; ".join(f"{k} {v[0]:.1f} ({v[1]:.1f} .. {v[2]:.1f})" for k, v in us.items()))
print("\n".join(lines))
if args and args[0]:
    os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
    with open(args[0], "w") as f:
        f.write("\n".join(lines) + "\n")
