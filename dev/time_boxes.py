#!/usr/bin/env python3
"""Measurement of the box launch of the loader's use_box mode (``bofi_pack_regions_box``, csrc/regions.hip) beside the plain launch on the same build; the
output is kept under profiles/.

    python dev/time_boxes.py [out.txt]

Stream time (HIP events around 200 back-to-back calls after warm-up, median of 5 such regions) for 64 images of F = 2048 with 36 and with 100 regions each,
float16 rows -> bfloat16 output: ``bofi_pack_regions`` into [64, R, 2048] against ``bofi_pack_regions_box`` into [64, R, 2112] -- 3 % more output bytes and
16 bytes of box per row, plus what the plain launch has no counterpart for: every workgroup computes its image's R keys, one barrier, a rank per row.
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

F, F_OUT, B = 2048, 2112, 64


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


def main():
    from boficap_amd import hip
    from boficap_amd.features import BoxRaggedBatch
    lines = [f"{torch.cuda.get_device_name(0)}; torch {torch.__version__}",
             f"== {B} images, F = {F}, float16 rows -> bfloat16; stream time per call (median [min, max] of 5 regions of 200 back-to-back calls)"]
    rng = np.random.default_rng(1)
    for R in (36, 100):
        images = [np.abs(rng.standard_normal((R, F))).astype(np.float16) for _ in range(B)]
        sizes = np.stack([rng.integers(200, 641, B), rng.integers(150, 481, B)], 1).astype(np.int32)
        boxes = []
        for w, h in sizes:
            x1, y1 = rng.uniform(0, w - 2, R), rng.uniform(0, h - 2, R)
            boxes.append(np.stack([x1, y1, x1 + rng.uniform(1, w - x1), y1 + rng.uniform(1, h - y1)], 1).astype(np.float32))
        rb = BoxRaggedBatch.from_arrays(images, boxes, sizes)
        rows, offs, dboxes, wh = rb.rows.cuda(), rb.offsets.cuda(), rb.boxes.cuda(), rb.wh.cuda()
        plain = torch.empty(B, R, F, dtype=torch.bfloat16, device="cuda")
        wide = torch.empty(B, R, F_OUT, dtype=torch.bfloat16, device="cuda")
        att_len = torch.empty(B, dtype=torch.int32, device="cuda")
        for norm_att, norm_box in ((False, False), (False, True), (True, True)):
            p = stream_ms(lambda: hip.pack_regions(rows, offs, rb.offsets, plain, norm=norm_att, att_len=att_len))
            q = stream_ms(lambda: hip.pack_regions_box(rows, dboxes, wh, rb.wh, offs, rb.offsets, wide, norm_att=norm_att, norm_box=norm_box, att_len=att_len))
            read = rows.numel() * 2 * (2 if norm_att else 1)
            moved_p, moved_q = read + plain.numel() * 2, read + wide.numel() * 2 + dboxes.numel() * 4
            lines.append(f"R = {R:3d} norm_att {int(norm_att)} norm_box {int(norm_box)}: pack_regions {p[0] * 1e3:7.1f} us [{p[1] * 1e3:.1f}, {p[2] * 1e3:.1f}] {moved_p / 1e6:6.2f} MB = "
                         f"{moved_p / p[0] / 1e6:7.1f} GB/s | pack_regions_box {q[0] * 1e3:7.1f} us [{q[1] * 1e3:.1f}, {q[2] * 1e3:.1f}] {moved_q / 1e6:6.2f} MB = "
                         f"{moved_q / q[0] / 1e6:7.1f} GB/s | x{q[0] / p[0]:.2f}")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
