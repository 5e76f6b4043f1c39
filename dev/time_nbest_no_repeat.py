#!/usr/bin/env python3
"""Time one NAIC decode plain, with nbest = 5, and with nbest = 5 / 6 under nbest_no_repeat (bofi_vocab_nbest_norepeat's two launches behind the replayed graph in place
of bofi_vocab_nbest's), on the full-size bf16 engine with the log-prob tensor kept, at 64 images per launch and at 1 024 (16 batches of 64, q1_group = 64), 36 regions,
synthetic features, seeded weights: HIP events around back-to-back calls, the forms interleaved block by block in one process.  Then the two entry points alone on the
decode's own tensor, HIP events around 20 calls, and the candidates launch's share (bofi_vocab_pick with nothing to block: that launch plus a light scan).  The sibling
of dev/time_nbest.py.
usage: python dev/time_nbest_no_repeat.py [out file] [blocks]"""
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
lines = [f"one NAIC decode (log-probs kept, row statistics), full-size bf16 engine, 36 regions; {blocks} interleaved blocks of {per_block} back-to-back calls per form "
         "(graph replay + what follows it), HIP events; ms per decode: median of the blocks (min .. max)"]
for B, hint in ((64, 1), (1024, 0)):
    att = feats[:B].contiguous()
    eng.set_decodes_in_flight(hint)                              # (64 images: a decode running alone; 1 024: the throughput forms)
    common = dict(want_logprob=True, row_stats=True, graph=True, q1_group=64 if B > 64 else 0)
    forms = {"plain": {}, "nbest=5": {"nbest": 5}, "nbest=5 no_repeat": {"nbest": 5, "nbest_no_repeat": True}, "nbest=6 no_repeat": {"nbest": 6, "nbest_no_repeat": True}}
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
    lines.append("      " + "; ".join(f"{k} - plain {(med[k] - med['plain']) * 1e3:+.1f} us per decode ({(med[k] / med['plain'] - 1) * 100:+.2f} %)" for k in forms if k != "plain"))
    p5, r5 = outs["nbest=5"], outs["nbest=5 no_repeat"]
    seq, n = p5["nbest_seq"][:, 0], p5["phrase_length"].sum(1)
    pos = torch.arange(1, S, device="cuda")[None, :]
    rep = ((seq[:, 1:] == seq[:, :-1]) & (seq[:, 1:] >= 7) & (pos < n[:, None])).any(1)
    lines.append(f"      the plain list's entry 0 repeats a word on {int(rep.sum())} of {B} images; the no-repeat list differs from the plain list on "
                 f"{int((r5['nbest_seq'] != p5['nbest_seq']).any(2).any(1).sum())}; lists of 5 full on {int((r5['nbest_count'] == 5).sum())}")
    # the entry points alone on this decode's tensor
    plain = outs["plain"]
    lpf = plain["seq_logprob"].view(B * S, V)
    ntok = plain["phrase_length"].sum(1).to(torch.int32)
    bufs = {N: (torch.empty(B, N, S, dtype=torch.int64, device="cuda"), torch.empty(B, N, dtype=torch.float64, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda"))
            for N in (5, 6)}
    work = torch.empty(B * S * 8, dtype=torch.int32, device="cuda")
    seq_pick = plain["seq"].clone()

    def plain_list(N):
        hip.vocab_nbest(lpf, V, S, N, ntok=ntok, pad_idx=cfg.pad_idx, seq_n=bufs[N][0], total=bufs[N][1], count=bufs[N][2], work=work)

    def nr_list(N):
        hip.vocab_nbest_norepeat(lpf, V, S, N, ntok=ntok, pad_idx=cfg.pad_idx, seq_n=bufs[N][0], total=bufs[N][1], count=bufs[N][2], work=work)

    def pick():
        hip.check(hip.lib().bofi_vocab_pick(hip.ptr(lpf), V, B * S, V, S, hip.ptr(ntok), 0, cfg.pad_idx, None, 0, 0, 7, hip.ptr(seq_pick), None, None, hip.ptr(work),
                                            work.numel() * 4, hip.stream_ptr()), "bofi_vocab_pick")

    us = {}
    for name, fn in (("bofi_vocab_nbest N = 5", lambda: plain_list(5)), ("bofi_vocab_nbest_norepeat N = 5", lambda: nr_list(5)),
                     ("bofi_vocab_nbest_norepeat N = 6", lambda: nr_list(6)), ("candidates launch + plain scan (bofi_vocab_pick, nothing blocked)", pick)):
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
    lines.append(f"      alone on the [{B * S}, {V}] tensor, us per call incl. the launch gaps: " + "; ".join(f"{k} {v[0]:.1f} ({v[1]:.1f} .. {v[2]:.1f})" for k, v in us.items()))
print("\n".join(lines))
if args and args[0]:
    os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
    with open(args[0], "w") as f:
        f.write("\n".join(lines) + "\n")
