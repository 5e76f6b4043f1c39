#!/usr/bin/env python3
"""Time the two launches of boficap_amd.surface at the sizes of a COCO validation: ``bofi_caption_trim`` on 5 000 x 20 ids, and
``bofi_sentence_lookup`` of 25 000 rows (5 000 images x 5 samples) in a table of 600 000 training sentences -- device-event times, the median of 20
windows of back-to-back launches each -- beside the host loops they replace on the same ids (``trim_host``, ``lookup_host``), copies included.
The device results are compared with the host's at these sizes first.  usage: python dev/time_surface.py [out file] [table rows]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np
import torch
from boficap_amd import hip
from boficap_amd.surface import CaptionSurface, TrainSentences, lookup_host, trim_host

M = int(sys.argv[2]) if len(sys.argv) > 2 else 600_000
V, S, WINDOWS, PER_WINDOW = 9495, 20, 20, 50
rng = np.random.default_rng(0)


def captions(rows, bad_ids, tail):
    """Rows of S ids over the vocabulary, 6..16 long, ``tail``: ending in 0..3 ids of ``bad_ids``."""
    seq = rng.integers(7, V, (rows, S))
    length = rng.integers(6, 17, rows)
    if tail:
        for r in range(rows):
            k = int(rng.integers(0, 4))
            seq[r, length[r] - k:length[r]] = rng.choice(bad_ids, k)
    seq[np.arange(S)[None, :] >= length[:, None]] = 0
    return seq


def device_median(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(WINDOWS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(PER_WINDOW):
            fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / PER_WINDOW * 1e3)
    return float(np.median(times)), float(min(times)), float(max(times))


trim_ids, count_ids = list(range(7, 21)), list(range(14, 31))            # 14 and 17 ids, as the reference's two lists
surface = CaptionSurface(V, trim_ids, count_ids, "cuda")
greedy = captions(5000, trim_ids, tail=True)
dev = torch.from_numpy(greedy).cuda()
out, length, bad = (torch.empty_like(dev), torch.empty(5000, dtype=torch.int32, device="cuda"), torch.empty(5000, dtype=torch.int32, device="cuda"))
lib = hip.lib()


def launch_trim():
    hip.check(lib.bofi_caption_trim(hip.ptr(dev), 5000, S, 0, hip.ptr(surface.trim_bits), hip.ptr(surface.count_bits), V, 0, hip.ptr(out), hip.ptr(length), hip.ptr(bad),
                                    hip.stream_ptr()), "bofi_caption_trim")


launch_trim()
want = trim_host(greedy, trim_ids, count_ids)
assert np.array_equal(out.cpu().numpy(), want[0]) and np.array_equal(length.cpu().numpy(), want[1]) and np.array_equal(bad.cpu().numpy(), want[2])
trim_us = device_median(launch_trim)
t0 = time.perf_counter()
h = trim_host(dev.cpu().numpy(), trim_ids, count_ids)
back = torch.from_numpy(h[0]).cuda(); torch.cuda.synchronize()
trim_host_ms = (time.perf_counter() - t0) * 1e3

table = captions(M, trim_ids, tail=False)                             # (distinct but for a chance duplicate: TrainSentences reports the count)
t0 = time.perf_counter()
train = TrainSentences(table, "cuda")
build_ms = (time.perf_counter() - t0) * 1e3
sampled = captions(25000, trim_ids, tail=False)
sampled[::2] = train.host[rng.integers(0, train.M, 12500)]                # every other sample is a training sentence
canon, kept, _ = surface.trim(sampled, remove=False)
novel, seen = torch.empty(25000, dtype=torch.int32, device="cuda"), torch.zeros(V, dtype=torch.int32, device="cuda")


def launch_lookup():
    hip.check(lib.bofi_sentence_lookup(hip.ptr(canon), hip.ptr(kept), 25000, S, hip.ptr(train.rows), train.M, train.St, V, hip.ptr(novel), hip.ptr(seen), hip.stream_ptr()),
              "bofi_sentence_lookup")


launch_lookup()
torch.cuda.synchronize()
t0 = time.perf_counter()
rows_h, kept_h = canon.cpu().numpy(), kept.cpu().numpy()
want_novel, want_seen = lookup_host(rows_h, kept_h, train.host, V)
lookup_host_ms = (time.perf_counter() - t0) * 1e3
assert np.array_equal(novel.cpu().numpy(), want_novel) and np.array_equal(seen.cpu().numpy(), want_seen)
lookup_us = device_median(launch_lookup)
lines = [f"caption surface ({WINDOWS} windows of {PER_WINDOW} back-to-back launches, device events; median [min .. max] per launch):",
         f"  bofi_caption_trim, 5 000 x {S} ids, V = {V}: {trim_us[0]:.1f} us [{trim_us[1]:.1f} .. {trim_us[2]:.1f}]; trim_host on the same ids with the copies both ways: {trim_host_ms:.1f} ms",
         f"  bofi_sentence_lookup, 25 000 x {S} ids in {train.M} training rows x {train.St}: {lookup_us[0]:.1f} us [{lookup_us[1]:.1f} .. {lookup_us[2]:.1f}]; lookup_host (a set of the "
         f"table's rows, then one probe per row) with the copy: {lookup_host_ms:.0f} ms; TrainSentences (canonical form, np.unique, upload; once per run): {build_ms:.0f} ms",
         f"  device = host on every row at these sizes; novel {int(want_novel.sum())} of 25 000, {int(want_seen.sum())} distinct words"]
print("\n".join(lines))
if len(sys.argv) > 1 and sys.argv[1]:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
