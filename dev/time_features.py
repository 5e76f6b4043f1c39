#!/usr/bin/env python3
"""Measurements of the feature side of the loader (boficap_amd/features.py, csrc/regions.hip); the output is kept as profiles/r10_region_features.txt.

    python dev/time_features.py

Stream time of ``bofi_pack_regions`` (HIP events around 200 back-to-back calls after warm-up, median of 5 such regions) and the bytes it moves, for 64
images of F = 2048 with 10..100 regions (fixed seed) and with 36 each, float32 and float16 files, bfloat16 output, with and without the norm -- against
the other way to the same tensors: ``data.collate_regions`` on the host, one copy of the padded float32 array, ``.to(bfloat16)`` [+ the torch norm].
The end-to-end figures (``tools/eval.py`` images/s from feature files, ``tools/train.py`` s/it with the feeder) are not measured here.
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

F = 2048


def lengths(kind, n, seed=0):
    return [36] * n if kind == "36" else [int(v) for v in np.random.default_rng(seed).integers(10, 101, n)]


def stream_ms(fn, calls=200, regions=5):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(regions):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / calls)
    return statistics.median(out), min(out), max(out)


def part1():
    from boficap_amd import hip
    from boficap_amd.data import collate_regions
    from boficap_amd.features import RaggedBatch
    print("== bofi_pack_regions: 64 images, F = 2048, bf16 output; stream time per call (median [min, max] of 5 regions of 200 back-to-back calls)")
    for kind in ("10..100", "36"):
        lens = lengths(kind, 64)
        rng = np.random.default_rng(1)
        R = max(lens)
        for file_dtype in (np.float32, np.float16):
            images = [np.abs(rng.standard_normal((l, F))).astype(file_dtype) for l in lens]
            rb = RaggedBatch.from_arrays(images)
            rows, offs = rb.rows.cuda(), rb.offsets.cuda()
            out = torch.empty(64, R, F, dtype=torch.bfloat16, device="cuda")
            att_len = torch.empty(64, dtype=torch.int32, device="cuda")
            feats, _ = collate_regions([a.astype(np.float32) for a in images])
            dense = torch.from_numpy(feats).cuda()
            h2d_ragged = rb.rows.numel() * rb.rows.element_size() + rb.offsets.numel() * 4
            h2d_dense = dense.numel() * 4
            print(f"-- regions {kind} (sum {sum(lens)}, longest {R}), files {np.dtype(file_dtype).name}: host -> device bytes ragged {h2d_ragged / 1e6:.2f} MB, "
                  f"padded float32 (collate_regions) {h2d_dense / 1e6:.2f} MB (x{h2d_dense / h2d_ragged:.2f})")
            for norm in (False, True):
                moved = rb.rows.numel() * rb.rows.element_size() * (2 if norm else 1) + out.numel() * 2
                med, lo, hi = stream_ms(lambda: hip.pack_regions(rows, offs, rb.offsets, out, norm=norm, att_len=att_len))

                def torch_way():
                    x = dense / dense.norm(2, 2, keepdim=True) if norm else dense
                    return x.to(torch.bfloat16)
                tmed, tlo, thi = stream_ms(torch_way)
                launches = 1, (4 if norm else 1)
                print(f"   norm {int(norm)}: pack_regions {med * 1e3:8.1f} us [{lo * 1e3:.1f}, {hi * 1e3:.1f}]  {moved / 1e6:6.2f} MB moved = {moved / med / 1e6:7.1f} GB/s, 1 launch | "
                      f"torch on the padded array {tmed * 1e3:8.1f} us [{tlo * 1e3:.1f}, {thi * 1e3:.1f}], >= {launches[1]} launch(es)")
            # the copies themselves, pinned host memory -> device (stream time of one copy)
            pin_dense = torch.from_numpy(feats).pin_memory()
            dst_d, dst_r = torch.empty_like(dense), torch.empty_like(rows)
            cd = stream_ms(lambda: dst_d.copy_(pin_dense, non_blocking=True), calls=20)
            cr = stream_ms(lambda: dst_r.copy_(rb.rows, non_blocking=True), calls=20)
            print(f"   copy: ragged {cr[0] * 1e3:8.1f} us ({h2d_ragged / cr[0] / 1e6:.1f} GB/s) | padded float32 {cd[0] * 1e3:8.1f} us ({h2d_dense / cd[0] / 1e6:.1f} GB/s)")


def main():
    print(f"{torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    part1()


if __name__ == "__main__":
    main()
