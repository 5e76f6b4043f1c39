#!/usr/bin/env python3
"""Time one NAIC decode plain, with nbest = N / nbest_no_repeat, and with diverse = N / diverse_no_repeat (bofi_vocab_diverse's two launches behind the replayed graph),
N = 5 and N = 6, on the full-size bf16 engine with the log-prob tensor kept, at 64 images per launch and at 1 024 (16 batches of 64, q1_group = 64), 36 regions, synthetic
features, seeded weights: HIP events around back-to-back calls, the forms interleaved block by block in one process.  Then the entry points alone on the decode's own
tensor, HIP events around 20 calls, beside the two lists' and the candidates launch's share (bofi_vocab_pick with nothing to block).  With ``--parent DIR`` (a built
checkout of the parent commit) bench.py -- the option off: nothing new may be launched -- runs on that tree and on this one alternately, three runs each, every run a
fresh process.  The sibling of dev/time_nbest_no_repeat.py.
usage: python dev/time_diverse_set.py [out file] [blocks] [--parent DIR]"""
import json, os, subprocess, sys
argv = sys.argv[1:]
parent = argv[argv.index("--parent") + 1] if "--parent" in argv else ""
args = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] != "--parent")]
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
         "(graph replay + what follows it), HIP events; ms per decode: median of the blocks (min .. max); lambda = 0.5"]
for B, hint in ((64, 1), (1024, 0)):
    att = feats[:B].contiguous()
    eng.set_decodes_in_flight(hint)                              # (64 images: a decode running alone; 1 024: the throughput forms)
    common = dict(want_logprob=True, row_stats=True, graph=True, q1_group=64 if B > 64 else 0)
    forms = {"plain": {}}
    for N in (5, 6):
        forms[f"nbest={N}"] = {"nbest": N}
        forms[f"nbest={N} no_repeat"] = {"nbest": N, "nbest_no_repeat": True}
        forms[f"diverse={N}"] = {"diverse": N}
        forms[f"diverse={N} no_repeat"] = {"diverse": N, "diverse_no_repeat": True}
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
    d5, r5, n5 = outs["diverse=5"], outs["diverse=5 no_repeat"], outs["nbest=5"]
    n = d5["phrase_length"].sum(1)
    pos = torch.arange(S, device="cuda")[None, None, :] < n[:, None, None]

    def hamming(seq):                                            # mean share of live positions at which two captions of a set differ, over the pairs and the images
        diff = ((seq[:, :, None, :] != seq[:, None, :, :]) & pos[:, None]).sum(3).float() / n.clamp(min=1)[:, None, None]
        N = seq.size(1)
        return float((diff.sum((1, 2)) / (N * (N - 1)))[n > 0].mean())

    lines.append(f"      the sets on these weights (no trained checkpoint: no quality claim): mean pairwise Hamming distance per live position nbest=5 {hamming(n5['nbest_seq']):.3f}, "
                 f"diverse=5 {hamming(d5['diverse_seq']):.3f}, diverse=5 no_repeat {hamming(r5['diverse_seq']):.3f}; mean log-prob of captions 1..4 against caption 0: nbest "
                 f"{float((n5['nbest_logp'][:, 1:].clamp(min=-1e30).mean(1) - n5['nbest_logp'][:, 0])[n > 0].mean()):+.3f}, diverse "
                 f"{float((d5['diverse_logp'][:, 1:].mean(1) - d5['diverse_logp'][:, 0])[n > 0].mean()):+.3f}")
    # the entry points alone on this decode's tensor
    plain = outs["plain"]
    lpf = plain["seq_logprob"].view(B * S, V)
    ntok = plain["phrase_length"].sum(1).to(torch.int32)
    bufs = {N: (torch.empty(B, N, S, dtype=torch.int64, device="cuda"), torch.empty(B, N, dtype=torch.float64, device="cuda"),
                torch.empty(B, N, dtype=torch.float64, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")) for N in (5, 6)}
    work = torch.empty(B * S * 8, dtype=torch.int32, device="cuda")
    seq_pick = plain["seq"].clone()

    def diverse(N, nr):
        hip.vocab_diverse(lpf, V, S, N, lam=0.5, no_repeat=nr, ntok=ntok, pad_idx=cfg.pad_idx, seq_n=bufs[N][0], total=bufs[N][1], aug=bufs[N][2], count=bufs[N][3], work=work)

    def plain_list(N):
        hip.vocab_nbest(lpf, V, S, N, ntok=ntok, pad_idx=cfg.pad_idx, seq_n=bufs[N][0], total=bufs[N][1], count=bufs[N][3], work=work)

    def nr_list(N):
        hip.vocab_nbest_norepeat(lpf, V, S, N, ntok=ntok, pad_idx=cfg.pad_idx, seq_n=bufs[N][0], total=bufs[N][1], count=bufs[N][3], work=work)

    def pick():
        hip.check(hip.lib().bofi_vocab_pick(hip.ptr(lpf), V, B * S, V, S, hip.ptr(ntok), 0, cfg.pad_idx, None, 0, 0, 7, hip.ptr(seq_pick), None, None, hip.ptr(work),
                                            work.numel() * 4, hip.stream_ptr()), "bofi_vocab_pick")

    us = {}
    calls = [("candidates launch + plain scan (bofi_vocab_pick, nothing blocked)", pick)]
    for N in (5, 6):
        calls += [(f"bofi_vocab_diverse N = {N}", lambda N=N: diverse(N, False)), (f"bofi_vocab_diverse N = {N} no_repeat", lambda N=N: diverse(N, True)),
                  (f"bofi_vocab_nbest N = {N}", lambda N=N: plain_list(N)), (f"bofi_vocab_nbest_norepeat N = {N}", lambda N=N: nr_list(N))]
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
    lines.append(f"      alone on the [{B * S}, {V}] tensor, us per call incl. the launch gaps: " + "; ".join(f"{k} {v[0]:.1f} ({v[1]:.1f} .. {v[2]:.1f})" for k, v in us.items()))
del eng, feats
torch.cuda.empty_cache()
if parent:                                                       # bench.py, the option off, the two trees alternating; each run a fresh process
    runs = {"parent": [], "this tree": []}
    for _ in range(3):
        for name, tree in (("parent", parent), ("this tree", ROOT)):
            r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "64", "--warmup", "16"], cwd=tree, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise SystemExit(f"bench.py failed in {tree}: {r.stderr[-2000:]}")
            res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
            runs[name].append(float(res["value"]))
            print(name, res, flush=True)
    lines.append("")
    lines.append("bench.py (the option off: nothing new is launched), parent's tree and this tree alternating, three runs each, python bench.py --gpus 1 --steps 64 --warmup 16")
    meds = {}
    for name, v in runs.items():
        meds[name] = sorted(v)[1]
        lines.append(f"  {name}: {', '.join(f'{x:.1f}' for x in v)}; median {meds[name]:.1f}; span {(max(v) - min(v)) / meds[name] * 100:.2f} %")
    diff = abs(meds["this tree"] - meds["parent"]) / meds["parent"] * 100
    span = max((max(v) - min(v)) / meds[k] * 100 for k, v in runs.items())
    lines.append(f"  medians differ by {diff:.2f} % (this tree {'above' if meds['this tree'] >= meds['parent'] else 'below'}); the larger of the two sides' own spans is {span:.2f} %: "
                 + ("no difference shown" if diff <= span else "A DIFFERENCE ABOVE THE RUN-TO-RUN SPAN"))
print("\n".join(lines))
if args and args[0]:
    os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
    with open(args[0], "w") as f:
        f.write("\n".join(lines) + "\n")
