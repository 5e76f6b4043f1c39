"""Word-to-region attention maps, host side (no GPU): the declarations agree, bofi_attn_maps refuses bad arguments before anything touches a device, the command
line refuses the option outside NAIC mode, the 'regions' field of a prediction entry -- and the float64 RESTATEMENT of the maps that tests/test_gpu_attn_maps.py
holds the kernel to (include/boficap_hip.h states the same rules in words at bofi_attn_maps)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

from conftest import ROOT

NAN = float("nan")


# ----------------------------------------------------------------------------- the maps, restated
def maps_np(q, k, B, H, Lq, Lk, scale, klen=None):
    """A [B, H, Lq, Lk] and M [B, Lq, Lk] in float64 from q [B * Lq, >= 64 H] and k [B * Lk, >= 64 H] (the values as stored, whatever their dtype was):
    softmax over r < len_b of q . k * scale per head, zeros beyond, a row whose sum of exponentials is NaN (a NaN or +inf score) NaN in all its Lk entries; M the
    heads' mean."""
    q, k = np.asarray(q, np.float64), np.asarray(k, np.float64)
    A = np.zeros((B, H, Lq, Lk))
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            n = Lk if klen is None else min(max(int(klen[b]), 0), Lk)
            for h in range(H):
                qs = q[b * Lq:(b + 1) * Lq, 64 * h:64 * h + 64]
                ks = k[b * Lk:b * Lk + n, 64 * h:64 * h + 64]
                s = np.einsum("td,rd->tr", qs, ks) * scale
                if n:
                    e = np.exp(s - s.max(1, keepdims=True))      # (numpy's max hands a NaN on; inf - inf is NaN)
                    A[b, h, :, :n] = e / e.sum(1, keepdims=True)
                    A[b, h, np.isnan(e.sum(1)), :] = NAN
    return A, A.sum(1) / H


def topk_np(mean, K, klen=None, qlen=None):
    """top_idx int32 / top_w float32 [B, Lq, K] of a float32 ``mean`` [B, Lq, Lk]: the K largest of mean[b, t, :len_b] in stable descending order (equal weights: lower
    index first) with mean's own floats; (-1, 0) in slots past len_b and on rows t >= qlen[b]; (-1, NaN) everywhere on a row that holds a NaN."""
    B, Lq, Lk = mean.shape
    idx, w = np.full((B, Lq, K), -1, np.int32), np.zeros((B, Lq, K), np.float32)
    for b in range(B):
        n = Lk if klen is None else min(max(int(klen[b]), 0), Lk)
        nq = Lq if qlen is None else min(max(int(qlen[b]), 0), Lq)
        for t in range(nq):
            row = mean[b, t, :n]
            if np.isnan(row).any():
                w[b, t] = NAN
                continue
            order = np.argsort(-row, kind="stable")[:K]
            idx[b, t, :len(order)], w[b, t, :len(order)] = order, row[order]
    return idx, w


# ----------------------------------------------------------------------------- tests
def _lib():
    from boficap_amd import hip
    assert os.path.exists(hip.LIB_PATH), "build the library first (python -m boficap_amd.build)"
    return hip, hip.lib()


def test_declarations_agree():
    """The kernel's entry point and the per-call record that carries the engine's attention outputs: header, ctypes table, build list, ABI version."""
    from boficap_amd import build, hip
    header = open(os.path.join(ROOT, "include", "boficap_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, arity in (("bofi_attn_maps", 19),):
        found = re.findall(r"\b" + name + r"\s*\(([^;{]*?)\)\s*;", code, flags=re.S)
        assert len(found) == 1 and found[0].count(",") + 1 == len(hip.SIGNATURES[name][1]) == arity, name
    # the per-call record: the header's field list is the ctypes mirror's, in order, and its size is the one the engine's graph key asserts
    body = re.search(r"typedef\s+struct\s+bofi_call_opts\s*\{(.*?)\}\s*bofi_call_opts_t\s*;", code, flags=re.S).group(1)
    assert re.findall(r"(\w+)\s*;", body) == [n for n, _ in hip.BofiCallOpts._fields_]
    pinned = re.findall(r"static_assert\(sizeof\(bofi_call_opts_t\) == (\d+)", open(os.path.join(build.CSRC, "engine.hip")).read())
    assert len(pinned) == 1 and C.sizeof(hip.BofiCallOpts) == int(pinned[0])
    assert {"attn_layer", "attn_topk", "attn_mean", "attn_heads", "attn_top_idx", "attn_top_w"} <= set(dict(hip.BofiCallOpts._fields_))
    assert "attn_maps.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "attn_maps.hip"))
    assert "launch_attn_maps" in open(os.path.join(build.CSRC, "bofi_kernels.h")).read()
    assert hip.ABI_VERSION == 5
    _, lib = _lib()
    assert hasattr(lib, "bofi_attn_maps") and callable(hip.attn_maps)


def test_attn_maps_refuses_bad_arguments_without_a_device():
    """Every one of these returns BOFI_ERR_ARG (1) from the argument check, with a message: the pointers are never read, no launch, no allocation."""
    hip, lib = _lib()
    p = C.c_void_p(0x1000)              # (any non-null value: validation comes first)
    good = dict(q=p, ldq=512, k=p, ldk=3072, dtype=hip.DT_BF16, B=2, H=8, Lq=20, Lk=36, scale=0.125, klen=None, qlen=None, qlen_bias=0, mean=p, heads=None, K=3, top_idx=p,
                top_w=p, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.bofi_attn_maps(a["q"], a["ldq"], a["k"], a["ldk"], a["dtype"], a["B"], a["H"], a["Lq"], a["Lk"], a["scale"], a["klen"], a["qlen"], a["qlen_bias"], a["mean"],
                                a["heads"], a["K"], a["top_idx"], a["top_w"], a["stream"])
        if rc == 1:
            assert b"attn_maps" in lib.bofi_last_error(), kw
        return rc

    assert call(B=0) == 1 and call(H=0) == 1
    assert call(Lq=0) == 1 and call(Lq=65) == 1 and call(Lk=0) == 1 and call(Lk=129) == 1
    assert call(K=-1) == 1 and call(K=9) == 1
    assert call(dtype=hip.DT_F16) == 1 and call(dtype=7) == 1
    assert call(q=None) == 1 and call(k=None) == 1
    assert call(mean=None, heads=None, K=0, top_idx=None, top_w=None) == 1                     # no output buffer at all
    assert call(top_idx=None) == 1 and call(top_w=None) == 1 and call(top_idx=None, top_w=None) == 1      # K > 0 needs both
    assert call(K=0, top_idx=None) == 1                                                        # one of the two without the other
    assert call(ldq=511) == 1 and call(ldk=500) == 1                                           # a pitch below 64 H: rows would overlap
    assert call(H=300, ldq=19200, ldk=19200) == 1                                              # one query row's share of LDS beyond the budget


def test_eval_tool_refuses_attn_topk_outside_naic():
    """An unknown option exits 2 as well: the message is the test."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval.py"), "--attn_topk", "3", "--inference_mode", "SAIC", "--synthetic", "8"],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 2 and "--attn_topk" in r.stderr and "NAIC" in r.stderr, r.stderr[-400:]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval.py"), "--attn_topk", "9", "--synthetic", "8"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 2 and "0..8" in r.stderr, r.stderr[-400:]


def test_regions_of_an_entry():
    """One list per id of the entry's 'seq' (the positions whose id is > 0), [region, weight] pairs heaviest first, -1 slots skipped."""
    import torch
    from boficap_amd import eval_utils
    seq = torch.tensor([[11, 7, 0, 9, 0], [0, 0, 0, 0, 0]])
    top = torch.tensor([[[4, 2, -1], [0, -1, -1], [-1, -1, -1], [5, 6, 7], [-1, -1, -1]], [[-1, -1, -1]] * 5], dtype=torch.int32)
    w = torch.tensor([[[.5, .25, 0.], [1., 0., 0.], [0., 0., 0.], [.5, .25, .125], [0., 0., 0.]], [[0., 0., 0.]] * 5])
    assert eval_utils.regions_of(seq[0], top[0], w[0]) == [[[4, .5], [2, .25]], [[0, 1.]], [[5, .5], [6, .25], [7, .125]]]
    assert eval_utils.regions_of(seq[1], top[1], w[1]) == []
    r = {"seq": seq, "attn_top": top, "attn_top_w": w}
    e = eval_utils.with_regions(eval_utils.entry_of(0, 0, seq, torch.tensor([1, 0]), torch.tensor([[2, 1, 0, 0, 0]] * 2), torch.zeros(2), torch.zeros(2)), r, 0)
    assert len(e["regions"]) == len(e["seq"]) == 3 and all(isinstance(p[0], int) and isinstance(p[1], float) for word in e["regions"] for p in word)
    plain = eval_utils.with_regions({"seq": [1]}, {"seq": seq}, 0)
    assert "regions" not in plain                                # (a decode without the option: the entry stays as it was)


def test_the_restatement_on_a_hand_made_case():
    """Two keys, one head: softmax of (0, ln 3) = (1/4, 3/4); a masked key is 0; a NaN query row is NaN everywhere; the top-K rules."""
    q = np.zeros((2, 64)); k = np.zeros((2, 64))
    q[0, 0], k[1, 0] = 1.0, np.log(3.0) * 8
    q[1, 3] = NAN
    A, M = maps_np(q, k, 1, 1, 2, 2, 0.125)
    assert np.allclose(A[0, 0, 0], [0.25, 0.75]) and np.isnan(A[0, 0, 1]).all() and np.array_equal(np.isnan(M), np.isnan(A[:, 0]))
    A1, _ = maps_np(q, k, 1, 1, 2, 2, 0.125, klen=[1])
    assert A1[0, 0, 0].tolist() == [1.0, 0.0] and np.isnan(A1[0, 0, 1]).all()
    mean = np.array([[[.25, .5, .25, .9], [NAN, .1, .2, .3], [.4, .3, .2, .1]]], np.float32)
    idx, w = topk_np(mean, 3, klen=[3], qlen=[2])
    assert idx[0, 0].tolist() == [1, 0, 2] and w[0, 0].tolist() == [.5, .25, .25]             # the tie goes to the lower index; column 3 is past len
    assert idx[0, 1].tolist() == [-1] * 3 and np.isnan(w[0, 1]).all()
    assert idx[0, 2].tolist() == [-1] * 3 and w[0, 2].tolist() == [0.] * 3                    # a row past qlen
    idx, w = topk_np(mean[:, 2:], 3, klen=[2])
    assert idx[0, 0].tolist() == [0, 1, -1] and w[0, 0].tolist() == [np.float32(.4), np.float32(.3), 0.]
