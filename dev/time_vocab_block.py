#!/usr/bin/env python3
"""Time bofi_vocab_block (the generator with the vocabulary epilogue inside) against the two launches it replaces -- bofi_linear_block(y_f32 = 1) into a
[rows, 9600] buffer + bofi_vocab_finalize reading it back (log-softmax in place) -- at the model's vocabulary, 6 400 and 20 480 rows, interleaved, one launch
at a time on the current stream.  usage: python dev/time_vocab_block.py [iters]"""
import math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from boficap_amd import hip as H

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 50
V, Npad, D, S = 9491, 9600, 512, 20
lib = H.lib()
g = torch.Generator().manual_seed(0)
w = torch.zeros(Npad, D)
w[:V] = torch.randn(V, D, generator=g) / math.sqrt(D)
c, cs = torch.zeros(Npad), torch.zeros(Npad)
c[:V] = torch.randn(V, generator=g) * 0.1
cs[:V] = w[:V].to(torch.bfloat16).double().sum(1).float()
wp = torch.empty(Npad * D, dtype=torch.bfloat16, device="cuda")
H.check(lib.bofi_pack_frag(H.ptr(w.to(torch.bfloat16).cuda()), H.ptr(wp), Npad, D, H.stream_ptr()))
cc, csc = c.cuda(), cs.cuda()


def timed(fn):
    for _ in range(5):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(iters):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / iters * 1e3


for M in (6400, 20480):
    x = (torch.randn(M, D, generator=g) * 2.0 - 0.3).cuda()
    y = torch.empty(M, Npad, device="cuda")
    lp = torch.randn(M, V, device="cuda")                      # (the epilogue's time does not depend on the values: it finalises a tensor of its own, in place at pitch V)
    seq = torch.empty(M, dtype=torch.int64, device="cuda")
    plogp, chosen = torch.empty(M, device="cuda"), torch.empty(M, device="cuda")

    def gen_only():
        H.check(lib.bofi_linear_block(H.ptr(x), D, H.ptr(wp), H.ptr(cc), H.ptr(csc), H.ptr(y), Npad, 1, M, Npad, 0, H.stream_ptr()))

    def fin_only():
        H.check(lib.bofi_vocab_finalize(H.ptr(lp), M, V, S, 1, None, 0, H.ptr(seq), H.stream_ptr()))

    def fused():
        H.vocab_block(x, wp, cc, csc, V, S, seq, row_plogp=plogp, row_chosen=chosen)

    rows = []
    for rep in range(3):                                        # interleaved: the spread is part of the answer
        rows.append((timed(gen_only), timed(fin_only), timed(fused)))
    for rep, (a, b, f) in enumerate(rows):
        print(f"rows {M:6d} rep {rep}: generator {a:8.1f} us + vocab_finalize {b:8.1f} us = {a + b:8.1f} us;  bofi_vocab_block {f:8.1f} us  ({(a + b) / f:.2f}x)", flush=True)
