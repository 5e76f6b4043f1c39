"""ctypes binding of libboficap_hip.so (C ABI: include/boficap_hip.h).

The HIP library is the product path.  There is no CPU fallback: importing this module without the
built library raises, and every non-zero status from the library raises ``BofiHipError``.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BOFI_LIB_PATH") or os.path.join(HERE, "libboficap_hip.so")     # (the override is a developer knob for A/B runs)

DT_F32, DT_BF16 = 0, 1
DT_F16 = 2                          # bofi_pack_regions' input only
FLAG_STRICT_Q1, FLAG_RAW_LOGITS, FLAG_GRAPH = 1, 2, 4
FLAG_REFINE_SHIFT = 8
FLAG_SAMPLE = 16
FLAG_PHASE_ENCODE, FLAG_PHASE_BOUND, FLAG_PHASE_FILL = 32, 64, 128
FLAG_SAIC_LAYOUT_ONLY = 4096
FLAG_IDS_ONLY = 8192
FLAG_MASK_PREDICT = 16384
FLAG_PICK_TRIGRAMS = 32768
FORK_IDS_ONLY = 1
ABI_VERSION = 5
REQUIRE_MAX = 8                     # BOFI_REQUIRE_MAX: required words per image (bofi_vocab_require)
REQUIRE_UNIT_MAX = 4                # BOFI_REQUIRE_UNIT_MAX: ids per required unit (bofi_vocab_require_units)
REQUIRE_ALT_MAX = 4                 # BOFI_REQUIRE_ALT_MAX: alternatives per required group (bofi_vocab_require_any)
NBEST_MAX = 8                       # BOFI_NBEST_MAX: captions per image of bofi_vocab_nbest
DIVERSE_MAX = 8                     # BOFI_DIVERSE_MAX: groups (captions per image) of bofi_vocab_diverse
DIVERSE_NR_MAX = 6                  # BOFI_DIVERSE_NR_MAX: ... under its repeat rule (N + 2 candidates per row are the candidates launch's 8)
NBEST_NR_MAX = 6                    # BOFI_NBEST_NR_MAX: ... of bofi_vocab_nbest_norepeat (its N + 2 candidates per row are the candidates launch's 8)


class BofiHipError(RuntimeError):
    pass


class BofiConfigC(C.Structure):
    _fields_ = [(n, C.c_int) for n in (
        "vocab", "feat", "d_model", "d_ff", "heads", "n_enc", "n_dec", "seq_length",
        "pad_idx", "bos_idx", "eos_idx", "len_idx", "head_hidden", "max_batch", "max_regions", "dtype", "n_len")]


_P, _I, _I64 = C.c_void_p, C.c_int, C.c_int64


class BofiCallOpts(C.Structure):
    """bofi_call_opts_t: the options of one decode_naic / decode_saic / fill_naic call (the header states each field); zero-filled = the defaults."""
    _fields_ = [("q1_group", _I), ("bound_iter_cap", _I), ("saic_it_begin", _I), ("saic_it_end", _I), ("sample_temperature", C.c_float), ("sample_seed", C.c_uint64),
                ("live_max", _P), ("sat_out", _P), ("row_plogp", _P), ("row_chosen", _P), ("refine_round", _P), ("attn_layer", _I), ("attn_topk", _I),
                ("attn_mean", _P), ("attn_heads", _P), ("attn_top_idx", _P), ("attn_top_w", _P),
                ("pick_ban", _P), ("pick_no_repeat", _I), ("pick_repeat_min_id", _I)]


_OPTS = C.POINTER(BofiCallOpts)

# name -> (restype, argtypes); mirrors include/boficap_hip.h one to one
SIGNATURES = {
    "bofi_abi_version": (_I, []),
    "bofi_last_error": (C.c_char_p, []),
    "bofi_layernorm": (_I, [_P, _P, _P, _P, _I, _I, _I, _P]),
    "bofi_linear": (_I, [_P, _I, _I, _P, _I, _P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _P, _I, _P]),
    "bofi_attention": (_I, [_P, _I, _P, _I, _P, _I, _P, _I, _I, _I, _I, _I, _I, _P, _I, _I, _P]),
    "bofi_vocab_finalize": (_I, [_P, _I, _I, _I, _I, _P, _I, _P, _P]),
    "bofi_attention_ex": (_I, [_P, _I, _P, _I, _P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _P, _I, _I, _I, C.c_float, C.c_uint64, _P, _P, _P, _I, _I, _P]),
    "bofi_layernorm_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "bofi_linear_rows": (_I, [_P, _I, _I, _P, _I, _P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P]),
    "bofi_rowgemm": (_I, [_P, _I, _P, _P, _P, _I, _P, _P, _I, _P, _I, _P, _I, _P, _I, _I, _I, _I, _I, _P, _I, _P, _P, _P]),
    "bofi_bound_qattn": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _I, _I, _P, _I, _P, _P, _I, _P]),
    "bofi_layernorm_bwd_ex": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _P, C.c_float, C.c_uint64, _P, _P]),
    "bofi_attention_bwd": (_I, [_P, _I, _P, _I, _P, _I, _P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _P, _I, _I, _I, _P, _P, _I, _P]),
    "bofi_attention_bwd_mfma": (_I, [_P, _I, _P, _I, _P, _I, _I, _P, _I, _P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _I, _I, _I, C.c_float, C.c_uint64,
                                     _P, _P, _P, _I, _I, _P]),
    "bofi_logsoftmax_bwd": (_I, [_P, _P, _P, _I, _I, _P]),
    "bofi_rl_take_draws": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "bofi_saic_collate": (_I, [_P, _P, _P, _I, _I, _I, _P, _P, _P, _P]),
    "bofi_nll_bwd": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "bofi_uic_criterion": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _I, _P, _P, _P, _I, _P, _P]),
    "bofi_uic_criterion_bwd": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _I, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P]),
    "bofi_colsum_add": (_I, [_P, _P, _I, _I, _P]),
    "bofi_embed_rows": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P]),
    "bofi_embed_bwd": (_I, [_P, _P, _P, _I, _I, C.c_float, _P]),
    "bofi_transpose_pad": (_I, [_P, _I, _P, _I, _I, _I, _I, _P, _P]),
    "bofi_transpose_many": (_I, [_P, _P, _P, _P, _I, _I, _P]),
    "bofi_gemm_tn_acc": (_I, [_P, _I, _I, _P, _I, _I, _P, _I, _I, _I, _I, _P, _P]),
    "bofi_gemm_tn_grouped": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "bofi_cast_bf16": (_I, [_P, _I, _P, _I, _I, _I, _P, _P, C.c_float, C.c_uint64, _P, _P]),
    "bofi_reload_env": (None, []),
    "bofi_linear_fused": (_I, [_P, _I, _P, _P, _P, _I, _P, _I, _I, _P, _I, _P, _P, _I, _P, _I, _I, _I, _I, _P]),
    "bofi_linear_ex": (_I, [_P, _I, _I, _P, _I, _P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _P, _I, C.c_float, C.c_uint64, _P, _P, _I, _P]),
    "bofi_linear_masked": (_I, [_P, _I, _I, _P, _I, _P, _I, C.c_float, _P, _I, _I, _I, _I, _I, _P]),
    "bofi_dropout": (_I, [_P, _P, _P, _I64, C.c_float, C.c_uint64, _P, _P]),
    "bofi_adam_step": (_I, [_P, _P, _P, _P, _P, _I64, C.c_float, C.c_float, C.c_float, C.c_float, _I, C.c_float, C.c_float, _P]),
    "bofi_relu_bwd": (_I, [_P, _P, _P, _I64, _P]),
    "bofi_vocab_stats": (_I, [_P, _P, _I, _I, _P, _P, _P]),
    "bofi_vocab_sample": (_I, [_P, _I, _I, _I, _I, C.c_float, C.c_uint64, _P, _I, _P, _P]),
    "bofi_engine_logprob": (_P, [_P]),
    "bofi_engine_refresh_device": (_I, [_P, _I, C.POINTER(C.c_char_p), C.POINTER(_P), C.POINTER(_I64), _P]),
    "bofi_engine_set_decodes_in_flight": (_I, [_P, _I]),
    "bofi_engine_bound_loop_active": (_I, [_P, _I]),
    "bofi_engine_saic_put_words": (_I, [_P, _P, _I, _P]),
    "bofi_engine_set_bound_loop": (_I, [_P, _I]),
    "bofi_engine_set_bound_kv_beside": (_I, [_P, _I]),
    "bofi_engine_bound_kv_beside_active": (_I, [_P, _I, _I, _I]),
    "bofi_engine_create": (_I, [C.POINTER(BofiConfigC), C.POINTER(_P)]),
    "bofi_engine_destroy": (None, [_P]),
    "bofi_engine_fork": (_I, [_P, C.POINTER(_P)]),
    "bofi_engine_fork_sized": (_I, [_P, _I, C.POINTER(_P)]),
    "bofi_engine_fork_ex": (_I, [_P, _I, _I, C.POINTER(_P)]),
    "bofi_engine_ids_only_fused": (_I, [_P, _I]),
    "bofi_engine_stream": (_P, [_P]),
    "bofi_engine_set_weight": (_I, [_P, C.c_char_p, _P, _I64]),
    "bofi_engine_finalize": (_I, [_P]),
    "bofi_engine_decode_naic": (_I, [_P, _P, _I, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _OPTS, _P]),
    "bofi_engine_decode_saic": (_I, [_P, _P, _I, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _OPTS, _P]),
    "bofi_engine_encode": (_I, [_P, _P, _I, _P, _I, _I, _P, _P]),
    "bofi_engine_bound_step": (_I, [_P, _P, _P, _I, _I, _P, _P, _P, _P]),
    "bofi_engine_debug_copy": (_I, [_P, C.c_char_p, _P, _I64, _P]),
    "bofi_gemm_flops": (C.c_double, [_I, _P]),
    "bofi_pack_frag": (_I, [_P, _P, _I, _I, _P]),
    "bofi_attn_block": (_I, [_P, _I, _P, _I, _P, _I, _I, _I, _I, _P, _I, _I, _I, _I, _P, _P, _P, _I, _P, _I, _P, _P, _P]),
    "bofi_linear_block": (_I, [_P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "bofi_vocab_block": (_I, [_P, _I, _P, _P, _P, _I, _I, _I, _I, _P, _I, _I, _P, _P, _P, _P, _I, _P]),
    "bofi_attn_linear_block": (_I, [_P, _I, _P, _I, _P, _I, _I, _I, _I, _P, _I, _I, _I, _P, _P, _P, _I, _P, _P, _P, _P, _I, _P]),
    "bofi_ffn_block": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _I, _P, _P, _I, _I, _P]),
    "bofi_ffn_linear_block": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _I, _I, _P]),
    "bofi_engine_fill_naic": (_I, [_P, _P, _P, _I, _I, _P, _I, _P, _P, _OPTS, _P]),
    "bofi_attn_out_ffn_block": (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _I, _I, _P]),
    "bofi_cider_refs": (_I, [_P, _P, _I, _I, _P, _P, _I, C.c_double, _P, _P, _P, _P, _I, _P]),
    "bofi_cider_score": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _I, C.c_double, C.c_double, C.c_double, _P, _P, _P, _P, _I, _P, _P, _P]),
    "bofi_reward_refs": (_I, [_P, _P, _I, _I, _P, _P, _I, C.c_double, _P, _P, _P, _P, _P, _P, _I, _P]),
    "bofi_reward_score": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _I, C.c_double, C.c_double, C.c_double, C.c_double, _P, _P, _P, _P, _P, _P, _I,
                               _P, _P, _P, _P]),
    "bofi_rouge_score": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _I, _I, C.c_double, _P, _P, _P, _P]),
    "bofi_diversity_workspace": (_I64, [_I, _I, _I]),
    "bofi_diversity_score": (_I, [_P, _I, _I, _I, _I, _P, _P, _I, C.c_double, _P, _I64, _P, _P, _P, _P, _P]),
    "bofi_oracle_stats": (_I, [_P, _P, _P, _I, _I, _P, _P, _P, _P]),
    "bofi_pack_regions": (_I, [_P, _I, _P, _P, _I, _I, _P, _I, _I, _I, _P, _P]),
    "bofi_pack_regions_box": (_I, [_P, _I, _P, _P, _P, _P, _P, _I, _I, _P, _I, _I, _I, _I, _I, _P, _P]),
    "bofi_mask_predict_step": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "bofi_attn_maps": (_I, [_P, _I, _P, _I, _I, _I, _I, _I, _I, C.c_float, _P, _P, _I, _P, _P, _I, _P, _P, _P]),
    "bofi_vocab_constrain": (_I, [_P, _I, _I, _I, _I, _P, _I, _I, _P, _I, _I, _P, _P, _P, _P]),
    "bofi_engine_pick_changed": (_I, [_P, _P, _I, _P]),
    "bofi_vocab_pick_workspace": (_I64, [_I]),
    "bofi_vocab_pick": (_I, [_P, _I, _I, _I, _I, _P, _I, _I, _P, _I, _I, _I, _P, _P, _P, _P, _I64, _P]),
    "bofi_vocab_require": (_I, [_P, _I, _I, _I, _I, _P, _I, _P, _I, _P, _I, _I, _P, _P, _P, _P, _P]),
    "bofi_vocab_require_units": (_I, [_P, _I, _I, _I, _I, _P, _I, _P, _I, _I, _P, _I, _I, _P, _P, _P, _P, _P]),
    "bofi_vocab_require_any": (_I, [_P, _I, _I, _I, _I, _P, _I, _P, _I, _I, _I, _P, _I, _I, _P, _P, _P, _P, _P, _P]),
    "bofi_vocab_nbest_workspace": (_I64, [_I]),
    "bofi_vocab_nbest": (_I, [_P, _I, _I, _I, _I, _P, _I, _I, _P, _I, _P, _P, _P, _P, _I64, _P]),
    "bofi_vocab_nbest_norepeat": (_I, [_P, _I, _I, _I, _I, _P, _I, _I, _P, _I, _I, _P, _P, _P, _P, _I64, _P]),
    "bofi_vocab_diverse": (_I, [_P, _I, _I, _I, _I, _P, _I, _I, _P, _I, C.c_double, _I, _I, _P, _P, _P, _P, _P, _I64, _P]),
    "bofi_caption_trim": (_I, [_P, _I, _I, _I, _P, _P, _I, _I, _P, _P, _P, _P]),
    "bofi_sentence_lookup": (_I, [_P, _P, _I, _I, _P, _I, _I, _I, _P, _P, _P]),
}

_lib = None


def lib():
    """The loaded library; raises if it has not been built (python -m boficap_amd.build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise BofiHipError(
                f"{LIB_PATH} is missing: build it with `python -m boficap_amd.build` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the decode path.")
        # torch bundles its own libamdhip64 (SONAME libamdhip64.so.7).  It must be loaded BEFORE this
        # library so that both resolve to ONE HIP runtime; loaded the other way round the process
        # ends up with two runtimes and the second sees no device.
        import torch  # noqa: F401
        l = C.CDLL(LIB_PATH)
        with open("/proc/self/maps") as f:
            copies = {ln.split()[-1] for ln in f if "libamdhip64" in ln}
        if len(copies) > 1:
            raise BofiHipError(f"two HIP runtimes are loaded ({sorted(copies)}); import torch before boficap_amd.hip")
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)          # AttributeError here = header/library mismatch
            fn.restype, fn.argtypes = res, args
        if l.bofi_abi_version() != ABI_VERSION:
            raise BofiHipError(f"ABI version {l.bofi_abi_version()} != binding version {ABI_VERSION}")
        _lib = l
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().bofi_last_error()
        raise BofiHipError(f"{what or 'libboficap_hip'}: status {rc}: {msg.decode() if msg else ''}")


def ptr(t):
    """Device (or host) pointer of a torch tensor / None."""
    return None if t is None else C.c_void_p(t.data_ptr())


def dtype_code(t) -> int:
    import torch
    if t.dtype == torch.float32:
        return DT_F32
    if t.dtype == torch.bfloat16:
        return DT_BF16
    raise BofiHipError(f"unsupported dtype {t.dtype}")


_torch = None


def stream_ptr():
    """The current torch HIP stream as a raw pointer (hot: called once per kernel launch)."""
    global _torch
    if _torch is None:
        import torch
        _torch = torch
    return _torch._C._cuda_getCurrentRawStream(_torch.cuda.current_device())


def vocab_block(x, wp, c, cs, V, S, seq, *, ntok=None, ntok_bias=0, pad_idx=0, row_plogp=None, row_chosen=None, nan_flag=None, alone=False):
    """``bofi_vocab_block`` on torch tensors: x float32 [M, 512] (row stride x.stride(0)), wp / c / cs the generator's packed weight, folded bias and column sums for
    ``c.numel()`` (padded) columns of which the first ``V`` count; seq int64 [M] out, row_plogp / row_chosen float32 [M] (both or neither), nan_flag int32 [1]."""
    check(lib().bofi_vocab_block(ptr(x), x.stride(0), ptr(wp), ptr(c), ptr(cs), x.shape[0], c.numel(), int(V), int(S), ptr(ntok), int(ntok_bias), int(pad_idx),
                                 ptr(seq), ptr(row_plogp), ptr(row_chosen), ptr(nan_flag), 1 if alone else 0, stream_ptr()), "bofi_vocab_block")


def pack_regions(rows, offsets, offsets_host, out, *, norm=False, att_len=None):
    """``bofi_pack_regions`` on torch tensors: rows [sum len, F] float32 / float16 / bfloat16 and offsets int32 [B + 1] on the device, offsets_host the host's
    int32 copy of the offsets (checked before the launch) or None, out [B, out_R, F] float32 / bfloat16 contiguous, att_len int32 [B] or None.  One launch on
    the current stream, no synchronisation."""
    import torch
    codes = {torch.float32: DT_F32, torch.bfloat16: DT_BF16, torch.float16: DT_F16}
    if rows.dtype not in codes or out.dtype not in (torch.float32, torch.bfloat16):
        raise BofiHipError(f"pack_regions: rows {rows.dtype} -> out {out.dtype} is not a supported pair")
    if rows.dim() != 2 or out.dim() != 3 or rows.size(1) != out.size(2) or not rows.is_contiguous() or not out.is_contiguous() or not rows.is_cuda or not out.is_cuda:
        raise BofiHipError("pack_regions: contiguous device tensors rows [n, F] and out [B, out_R, F] expected")
    B = out.size(0)
    if offsets.dtype != torch.int32 or offsets.numel() != B + 1 or not offsets.is_cuda or not offsets.is_contiguous():
        raise BofiHipError("pack_regions: offsets must be int32 [B + 1] on the device")
    if offsets_host is not None and (offsets_host.dtype != torch.int32 or offsets_host.numel() != B + 1 or offsets_host.is_cuda or not offsets_host.is_contiguous()):
        raise BofiHipError("pack_regions: offsets_host must be int32 [B + 1] on the host")
    if offsets_host is not None and int(offsets_host[B]) > rows.size(0):
        raise BofiHipError(f"pack_regions: the offsets name {int(offsets_host[B])} rows, rows holds {rows.size(0)}")
    if att_len is not None and (att_len.dtype != torch.int32 or att_len.numel() != B or not att_len.is_cuda or not att_len.is_contiguous()):
        raise BofiHipError("pack_regions: att_len must be int32 [B] on the device")
    check(lib().bofi_pack_regions(ptr(rows), codes[rows.dtype], ptr(offsets), ptr(offsets_host), B, rows.size(1), ptr(out), dtype_code(out), out.size(1),
                                  1 if norm else 0, ptr(att_len), stream_ptr()), "bofi_pack_regions")


def pack_regions_box(rows, boxes, wh, wh_host, offsets, offsets_host, out, *, norm_att=False, norm_box=False, att_len=None):
    """``bofi_pack_regions_box`` on torch tensors: rows [sum len, F_att] float32 / float16 / bfloat16, boxes float32 [sum len, 4], wh int32 [B, 2] and offsets
    int32 [B + 1] on the device, wh_host / offsets_host the host's int32 copies (checked before the launch) or None, out [B, out_R, F_out] float32 / bfloat16
    contiguous with F_out >= F_att + 5, att_len int32 [B] or None.  One launch on the current stream, no synchronisation."""
    import torch
    codes = {torch.float32: DT_F32, torch.bfloat16: DT_BF16, torch.float16: DT_F16}
    if rows.dtype not in codes or out.dtype not in (torch.float32, torch.bfloat16):
        raise BofiHipError(f"pack_regions_box: rows {rows.dtype} -> out {out.dtype} is not a supported pair")
    if rows.dim() != 2 or out.dim() != 3 or not rows.is_contiguous() or not out.is_contiguous() or not rows.is_cuda or not out.is_cuda:
        raise BofiHipError("pack_regions_box: contiguous device tensors rows [n, F_att] and out [B, out_R, F_out] expected")
    if boxes.dtype != torch.float32 or boxes.dim() != 2 or boxes.size(1) != 4 or boxes.size(0) != rows.size(0) or not boxes.is_cuda or not boxes.is_contiguous():
        raise BofiHipError(f"pack_regions_box: boxes must be float32 [{rows.size(0)}, 4] on the device, one box per row")
    B = out.size(0)
    if wh.dtype != torch.int32 or tuple(wh.shape) != (B, 2) or not wh.is_cuda or not wh.is_contiguous():
        raise BofiHipError("pack_regions_box: wh must be int32 [B, 2] on the device")
    if wh_host is not None and (wh_host.dtype != torch.int32 or tuple(wh_host.shape) != (B, 2) or wh_host.is_cuda or not wh_host.is_contiguous()):
        raise BofiHipError("pack_regions_box: wh_host must be int32 [B, 2] on the host")
    if offsets.dtype != torch.int32 or offsets.numel() != B + 1 or not offsets.is_cuda or not offsets.is_contiguous():
        raise BofiHipError("pack_regions_box: offsets must be int32 [B + 1] on the device")
    if offsets_host is not None and (offsets_host.dtype != torch.int32 or offsets_host.numel() != B + 1 or offsets_host.is_cuda or not offsets_host.is_contiguous()):
        raise BofiHipError("pack_regions_box: offsets_host must be int32 [B + 1] on the host")
    if offsets_host is not None and int(offsets_host[B]) > rows.size(0):
        raise BofiHipError(f"pack_regions_box: the offsets name {int(offsets_host[B])} rows, rows holds {rows.size(0)}")
    if att_len is not None and (att_len.dtype != torch.int32 or att_len.numel() != B or not att_len.is_cuda or not att_len.is_contiguous()):
        raise BofiHipError("pack_regions_box: att_len must be int32 [B] on the device")
    check(lib().bofi_pack_regions_box(ptr(rows), codes[rows.dtype], ptr(boxes), ptr(wh), ptr(wh_host), ptr(offsets), ptr(offsets_host), B, rows.size(1), ptr(out),
                                      dtype_code(out), out.size(1), out.size(2), 1 if norm_att else 0, 1 if norm_box else 0, ptr(att_len), stream_ptr()),
          "bofi_pack_regions_box")


def attn_maps(q, k, B, H, Lq, Lk, *, scale=0.125, klen=None, qlen=None, qlen_bias=0, mean=None, heads=None, K=0, top_idx=None, top_w=None):
    """``bofi_attn_maps`` on torch tensors: q [B * Lq, >= 64 H] and k [B * Lk, >= 64 H] float32 / bfloat16 device tensors whose row strides are the pitches; klen / qlen
    int32 [B] or None; mean float32 [B, Lq, Lk], heads float32 [B, H, Lq, Lk], top_idx int32 / top_w float32 [B, Lq, K] -- contiguous, each optional.  One launch on the
    current stream, no synchronisation."""
    import torch
    if q.dtype != k.dtype or q.dim() != 2 or k.dim() != 2 or q.stride(1) != 1 or k.stride(1) != 1 or not q.is_cuda or not k.is_cuda:
        raise BofiHipError("attn_maps: q and k must be 2-d device tensors of one dtype with unit column stride")
    if q.size(0) < B * Lq or k.size(0) < B * Lk or q.size(1) < 64 * H or k.size(1) < 64 * H:
        raise BofiHipError("attn_maps: q needs B * Lq rows, k B * Lk rows, both 64 * H columns")
    for name, t, dt, shape in (("klen", klen, torch.int32, (B,)), ("qlen", qlen, torch.int32, (B,)), ("mean", mean, torch.float32, (B, Lq, Lk)),
                               ("heads", heads, torch.float32, (B, H, Lq, Lk)), ("top_idx", top_idx, torch.int32, (B, Lq, K)), ("top_w", top_w, torch.float32, (B, Lq, K))):
        if t is not None and (t.dtype != dt or tuple(t.shape) != shape or not t.is_cuda or not t.is_contiguous()):
            raise BofiHipError(f"attn_maps: {name} must be a contiguous {dt} device tensor of shape {shape}")
    check(lib().bofi_attn_maps(ptr(q), q.stride(0), ptr(k), k.stride(0), dtype_code(q), int(B), int(H), int(Lq), int(Lk), float(scale), ptr(klen), ptr(qlen), int(qlen_bias),
                               ptr(mean), ptr(heads), int(K), ptr(top_idx), ptr(top_w), stream_ptr()), "bofi_attn_maps")


def ban_bits(ids, V: int, device=None):
    """The bit table of ``bofi_vocab_constrain`` / ``bofi_call_opts_t.pick_ban`` from an id list: uint32 [(V + 31) / 32] (as int32 storage) on ``device``, bit id % 32 of word
    id / 32 set for every listed id.  Checked on the host: every id in 0..V-1, and at least two ids left unbanned (the kernel needs a second candidate per position)."""
    import numpy as np
    import torch
    ids = sorted({int(i) for i in ids})
    if ids and (ids[0] < 0 or ids[-1] >= V):
        raise BofiHipError(f"ban_ids: ids must lie in 0..{V - 1}, got {ids[0] if ids[0] < 0 else ids[-1]}")
    if V - len(ids) < 2:
        raise BofiHipError(f"ban_ids: {len(ids)} of {V} ids banned -- at least two must stay")
    words = np.zeros((V + 31) // 32, np.uint32)
    for i in ids:
        words[i >> 5] |= np.uint32(1 << (i & 31))
    t = torch.from_numpy(words.view(np.int32))
    return t if device is None else t.to(device)


def vocab_constrain(x, V, S, seq, *, ntok=None, ntok_bias=0, pad_idx=0, ban=None, no_repeat=False, repeat_min_id=7, row_chosen=None, changed=None):
    """``bofi_vocab_constrain`` on torch tensors: x float32 [rows, >= V] on the device with unit column stride (its row stride is the pitch; any 4-byte alignment), seq int64
    [rows] read and written, ntok int32 [rows / S] or None, ban the bit table of ``ban_bits`` (int32 / uint32 storage, (V + 31) / 32 words) or None, row_chosen float32 [rows]
    and changed int32 [rows / S] optional.  One launch on the current stream, no synchronisation."""
    import torch
    if x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1 or not x.is_cuda:
        raise BofiHipError("vocab_constrain: x must be a 2-d float32 device tensor with unit column stride")
    rows = x.size(0)
    if x.size(1) < V or S < 1 or rows % S:
        raise BofiHipError("vocab_constrain: x needs V columns and a multiple of S rows")
    B = rows // S
    for name, t, dt, n in (("seq", seq, torch.int64, rows), ("ntok", ntok, torch.int32, B), ("ban", ban, torch.int32, (V + 31) // 32),
                           ("row_chosen", row_chosen, torch.float32, rows), ("changed", changed, torch.int32, B)):
        if t is None and name != "seq":
            continue
        if t is None or t.dtype != dt or t.numel() != n or not t.is_cuda or not t.is_contiguous():
            raise BofiHipError(f"vocab_constrain: {name} must be a contiguous {dt} device tensor of {n} elements")
    check(lib().bofi_vocab_constrain(ptr(x), x.stride(0), rows, int(V), int(S), ptr(ntok), int(ntok_bias), int(pad_idx), ptr(ban), 1 if no_repeat else 0, int(repeat_min_id),
                                     ptr(seq), ptr(row_chosen), ptr(changed), stream_ptr()), "bofi_vocab_constrain")


def vocab_pick(x, V, S, seq, *, ntok=None, ntok_bias=0, pad_idx=0, ban=None, no_repeat=False, block_trigrams=False, repeat_min_id=7, row_chosen=None, changed=None,
               work=None):
    """``bofi_vocab_pick`` on torch tensors: ``vocab_constrain``'s arguments plus ``block_trigrams`` and ``work``, an int32 device workspace of at least
    ``bofi_vocab_pick_workspace(rows)`` bytes (None: one is made).  Two launches on the current stream, no synchronisation."""
    import torch
    if x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1 or not x.is_cuda:
        raise BofiHipError("vocab_pick: x must be a 2-d float32 device tensor with unit column stride")
    rows = x.size(0)
    if x.size(1) < V or S < 1 or rows % S:
        raise BofiHipError("vocab_pick: x needs V columns and a multiple of S rows")
    B = rows // S
    if work is None:
        work = torch.empty(max(1, lib().bofi_vocab_pick_workspace(rows) // 4), dtype=torch.int32, device=x.device)
    for name, t, dt, n in (("seq", seq, torch.int64, rows), ("ntok", ntok, torch.int32, B), ("ban", ban, torch.int32, (V + 31) // 32),
                           ("row_chosen", row_chosen, torch.float32, rows), ("changed", changed, torch.int32, B), ("work", work, torch.int32, None)):
        if t is None and name != "seq":
            continue
        if t is None or t.dtype != dt or (n is not None and t.numel() != n) or not t.is_cuda or not t.is_contiguous():
            raise BofiHipError(f"vocab_pick: {name} must be a contiguous {dt} device tensor" + ("" if n is None else f" of {n} elements"))
    check(lib().bofi_vocab_pick(ptr(x), x.stride(0), rows, int(V), int(S), ptr(ntok), int(ntok_bias), int(pad_idx), ptr(ban), 1 if no_repeat else 0,
                                1 if block_trigrams else 0, int(repeat_min_id), ptr(seq), ptr(row_chosen), ptr(changed), ptr(work), work.numel() * 4, stream_ptr()),
          "bofi_vocab_pick")


def require_table(require_ids, B: int, V: int, ban_ids=()):
    """The [B, K] int32 word table of ``bofi_vocab_require`` (host tensor, -1 padding) from host-side input: an int array / host tensor [B, K], a list of B per-image id
    lists, or one flat list applied to every image.  None when nothing is required (no input, empty lists, rows of -1 only).  Checked here: ids in 0..V-1 (-1 pads a row),
    at most ``REQUIRE_MAX`` per image, none of them in ``ban_ids``; duplicates within an image are dropped."""
    import numpy as np
    import torch
    if require_ids is None:
        return None
    if isinstance(require_ids, torch.Tensor):
        require_ids = require_ids.cpu().numpy()
    if isinstance(require_ids, np.ndarray):
        if require_ids.ndim == 1:
            require_ids = [require_ids.tolist()] * B
        elif require_ids.ndim == 2:
            require_ids = require_ids.tolist()
        else:
            raise BofiHipError("require_ids: a [B, K] table, a list of per-image id lists or one flat id list")
    rows = list(require_ids)
    if rows and not isinstance(rows[0], (list, tuple, np.ndarray)):
        rows = [rows] * B                                        # one flat list: every image
    if not rows:
        return None
    if len(rows) != B:
        raise BofiHipError(f"require_ids: {len(rows)} rows for {B} images")
    ban = {int(i) for i in ban_ids or ()}
    clean = []
    for r in rows:
        ids = []
        for i in r:
            i = int(i)
            if i == -1:
                continue
            if not 0 <= i < V:
                raise BofiHipError(f"require_ids: ids must lie in 0..{V - 1} (-1 pads a row), got {i}")
            if i in ban:
                raise BofiHipError(f"require_ids: id {i} is also in ban_ids")
            if i not in ids:
                ids.append(i)
        if len(ids) > REQUIRE_MAX:
            raise BofiHipError(f"require_ids: at most {REQUIRE_MAX} required words per image, got {len(ids)}")
        clean.append(ids)
    K = max(len(r) for r in clean)
    if K == 0:
        return None
    t = np.full((B, K), -1, np.int32)
    for b, r in enumerate(clean):
        t[b, :len(r)] = r
    return torch.from_numpy(t)


def vocab_require(x, V, S, seq, words, pos, *, ntok=None, ntok_bias=0, ban=None, no_repeat=False, repeat_min_id=7, row_chosen=None, moved=None):
    """``bofi_vocab_require`` on torch tensors: x float32 [rows, >= V] on the device with unit column stride (its row stride is the pitch; any 4-byte alignment), seq int64
    [rows] read and written, words int32 [rows / S, K] (1 <= K <= ``REQUIRE_MAX``), pos int32 [rows / S, K] out; ntok int32 [rows / S] or None, ban the bit table of
    ``ban_bits`` or None, row_chosen float32 [rows] and moved int32 [rows / S] optional.  One launch on the current stream, no synchronisation."""
    import torch
    if x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1 or not x.is_cuda:
        raise BofiHipError("vocab_require: x must be a 2-d float32 device tensor with unit column stride")
    rows = x.size(0)
    if x.size(1) < V or S < 1 or rows % S:
        raise BofiHipError("vocab_require: x needs V columns and a multiple of S rows")
    B = rows // S
    if words is None or words.dim() != 2 or words.size(0) != B:
        raise BofiHipError(f"vocab_require: words must be int32 [{B}, K]")
    K = words.size(1)
    for name, t, dt, n in (("seq", seq, torch.int64, rows), ("words", words, torch.int32, B * K), ("pos", pos, torch.int32, B * K), ("ntok", ntok, torch.int32, B),
                           ("ban", ban, torch.int32, (V + 31) // 32), ("row_chosen", row_chosen, torch.float32, rows), ("moved", moved, torch.int32, B)):
        if t is None and name not in ("seq", "words", "pos"):
            continue
        if t is None or t.dtype != dt or t.numel() != n or not t.is_cuda or not t.is_contiguous():
            raise BofiHipError(f"vocab_require: {name} must be a contiguous {dt} device tensor of {n} elements")
    check(lib().bofi_vocab_require(ptr(x), x.stride(0), rows, int(V), int(S), ptr(ntok), int(ntok_bias), ptr(words), int(K), ptr(ban), 1 if no_repeat else 0,
                                   int(repeat_min_id), ptr(seq), ptr(row_chosen), ptr(pos), ptr(moved), stream_ptr()), "bofi_vocab_require")


def _units_meet(a, b, min_id: int) -> bool:
    """Two required units could meet and form an adjacent repeat of a word: the last id of one is the first id of the other."""
    return (a[-1] == b[0] and a[-1] >= min_id) or (b[-1] == a[0] and b[-1] >= min_id)


def require_unit_table(require_phrases, B: int, V: int, ban_ids=(), no_repeat: bool = False, repeat_min_id: int = 7):
    """The [B, K, L] int32 unit table of ``bofi_vocab_require_units`` (host tensor, -1 padding) from host-side input: per image a list of units, each a list of 1 ..
    ``REQUIRE_UNIT_MAX`` ids, or one flat list of units applied to every image.  None when nothing is required (no input, empty lists).
    Checked here, each refusal naming the offender: ids in 0..V-1, units of at most ``REQUIRE_UNIT_MAX`` ids, at most ``REQUIRE_MAX`` units per image, no id of
    ``ban_ids``; under ``no_repeat`` no unit with two equal adjacent words (ids >= ``repeat_min_id``) and no two units of an image that could meet at a shared word (the
    last id of one is the first of the other: the kernel would skip the later one).  Empty units and a repeated unit within an image are dropped."""
    import numpy as np
    import torch
    if require_phrases is None:
        return None
    if isinstance(require_phrases, torch.Tensor):
        require_phrases = require_phrases.cpu().numpy()
    if isinstance(require_phrases, np.ndarray):                  # a [B, K, L] table (or [K, L] for every image) with -1 padding: a unit is its leading run of ids
        if require_phrases.ndim not in (2, 3):
            raise BofiHipError("require_phrases: a [B, K, L] table, per image a list of units (each a list of ids), or one flat list of units")
        run = lambda u: u[:next((i for i, v in enumerate(u) if v == -1), len(u))]
        units_of = lambda r: [run(u) for u in r if run(u)]
        require_phrases = units_of(require_phrases.tolist()) if require_phrases.ndim == 2 else [units_of(r) for r in require_phrases.tolist()]
    rows = list(require_phrases)
    if any(isinstance(u, (int, np.integer)) for u in rows):
        raise BofiHipError("require_phrases: a unit is a list of ids -- [[3, 4]] is one unit of two ids; for single ids give require_ids")
    if any(u is not None and len(u) and isinstance(u[0], (int, np.integer)) for u in rows):
        rows = [rows] * B                                        # one flat list of units: every image
    if not rows:
        return None
    if len(rows) != B:
        raise BofiHipError(f"require_phrases: {len(rows)} rows for {B} images")
    ban = {int(i) for i in ban_ids or ()}
    clean = []
    for r in rows:
        units = []
        for u in (r if r is not None else ()):
            if isinstance(u, (int, np.integer)):
                raise BofiHipError(f"require_phrases: a unit is a list of ids, got the bare id {int(u)}")
            if any(not isinstance(i, (int, np.integer)) for i in u):
                raise BofiHipError(f"require_phrases: a unit is a list of ids, got {list(u)}")
            u = [int(i) for i in u]
            if not u:
                continue
            if len(u) > REQUIRE_UNIT_MAX:
                raise BofiHipError(f"require_phrases: a unit holds at most {REQUIRE_UNIT_MAX} ids, got {u}")
            for i in u:
                if not 0 <= i < V:
                    raise BofiHipError(f"require_phrases: ids must lie in 0..{V - 1}, got {i} in unit {u}")
                if i in ban:
                    raise BofiHipError(f"require_phrases: id {i} of unit {u} is also in ban_ids")
            if no_repeat and any(x == y and x >= repeat_min_id for x, y in zip(u, u[1:])):
                raise BofiHipError(f"require_phrases: unit {u} repeats a word (not under no_repeat)")
            if u in units:
                continue
            if no_repeat:
                for v in units:
                    if _units_meet(v, u, int(repeat_min_id)):
                        raise BofiHipError(f"require_phrases: units {v} and {u} could meet at a shared word and form an adjacent repeat (not under no_repeat)")
            units.append(u)
        if len(units) > REQUIRE_MAX:
            raise BofiHipError(f"require_phrases: at most {REQUIRE_MAX} required units per image, got {len(units)}")
        clean.append(units)
    K = max(len(r) for r in clean)
    if K == 0:
        return None
    L = max(len(u) for r in clean for u in r)
    t = np.full((B, K, L), -1, np.int32)
    for b, r in enumerate(clean):
        for j, u in enumerate(r):
            t[b, j, :len(u)] = u
    return torch.from_numpy(t)


def vocab_require_units(x, V, S, seq, units, pos, *, ntok=None, ntok_bias=0, ban=None, no_repeat=False, repeat_min_id=7, row_chosen=None, moved=None):
    """``bofi_vocab_require_units`` on torch tensors: as ``vocab_require`` with units int32 [rows / S, K, L] (1 <= K <= ``REQUIRE_MAX``, 1 <= L <= ``REQUIRE_UNIT_MAX``)
    in place of the words and pos int32 [rows / S, K] the units' start positions.  One launch on the current stream, no synchronisation."""
    import torch
    if x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1 or not x.is_cuda:
        raise BofiHipError("vocab_require_units: x must be a 2-d float32 device tensor with unit column stride")
    rows = x.size(0)
    if x.size(1) < V or S < 1 or rows % S:
        raise BofiHipError("vocab_require_units: x needs V columns and a multiple of S rows")
    B = rows // S
    if units is None or units.dim() != 3 or units.size(0) != B:
        raise BofiHipError(f"vocab_require_units: units must be int32 [{B}, K, L]")
    K, L = units.size(1), units.size(2)
    for name, t, dt, n in (("seq", seq, torch.int64, rows), ("units", units, torch.int32, B * K * L), ("pos", pos, torch.int32, B * K), ("ntok", ntok, torch.int32, B),
                           ("ban", ban, torch.int32, (V + 31) // 32), ("row_chosen", row_chosen, torch.float32, rows), ("moved", moved, torch.int32, B)):
        if t is None and name not in ("seq", "units", "pos"):
            continue
        if t is None or t.dtype != dt or t.numel() != n or not t.is_cuda or not t.is_contiguous():
            raise BofiHipError(f"vocab_require_units: {name} must be a contiguous {dt} device tensor of {n} elements")
    check(lib().bofi_vocab_require_units(ptr(x), x.stride(0), rows, int(V), int(S), ptr(ntok), int(ntok_bias), ptr(units), int(K), int(L), ptr(ban),
                                         1 if no_repeat else 0, int(repeat_min_id), ptr(seq), ptr(row_chosen), ptr(pos), ptr(moved), stream_ptr()),
          "bofi_vocab_require_units")


_ANY_NESTING = "a group is a list of alternatives, each a list of ids -- [[[3], [4, 5]]] is one group of two alternatives, [3] and [4, 5]"


def require_any_table(require_any, B: int, V: int, ban_ids=(), no_repeat: bool = False, repeat_min_id: int = 7):
    """The [B, K, A, L] int32 table of ``bofi_vocab_require_any`` (host tensor, -1 padding) from host-side input: per image a list of GROUPS, each a list of 1 ..
    ``REQUIRE_ALT_MAX`` alternatives, each a list of 1 .. ``REQUIRE_UNIT_MAX`` ids; one flat list of groups applied to every image; or a [B, K, A, L] ([K, A, L]: every
    image) int array with -1 padding, an alternative being its leading run of ids.  None when nothing is required (no input, empty lists).
    Checked here, each refusal naming the offender: ids in 0..V-1, alternatives of at most ``REQUIRE_UNIT_MAX`` ids, at most ``REQUIRE_ALT_MAX`` alternatives per group, at
    most ``REQUIRE_MAX`` groups per image, no id of ``ban_ids``, no alternative given twice for an image (in one group or across groups: the kernel would skip the later
    one); under ``no_repeat`` no alternative with two equal adjacent words (ids >= ``repeat_min_id``) and no two alternatives of DIFFERENT groups that could meet at a
    shared word (the last id of one is the first of the other).  Groups without an alternative are dropped; an empty alternative keeps its place inside its group (an
    empty slot of the table), so that the kernel's ``which`` indexes the group as it was given."""
    import numpy as np
    import torch
    if require_any is None:
        return None
    if isinstance(require_any, torch.Tensor):
        require_any = require_any.cpu().numpy()
    if isinstance(require_any, np.ndarray):
        if require_any.ndim not in (3, 4):
            raise BofiHipError("require_any: a [B, K, A, L] table, per image a list of groups (each a list of alternatives, each a list of ids), or one flat list of groups")
        run = lambda u: u[:next((i for i, v in enumerate(u) if v < 0), len(u))]
        groups_of = lambda r: [[run(u) for u in g] for g in r]
        require_any = [groups_of(require_any.tolist())] * B if require_any.ndim == 3 else [groups_of(r) for r in require_any.tolist()]
    is_id = lambda v: isinstance(v, (int, np.integer))
    rows = list(require_any)
    if any(is_id(g) for g in rows):
        raise BofiHipError(f"require_any: got the bare id {int(next(g for g in rows if is_id(g)))}: {_ANY_NESTING}")
    for g in rows:                                               # one flat list of groups: its first non-empty alternative holds ids, not lists
        first = next((u for u in (g if g is not None else ()) if is_id(u) or (u is not None and len(u))), None)
        if first is None:
            continue
        if is_id(first):
            raise BofiHipError(f"require_any: got the bare id {int(first)} where an alternative is expected: {_ANY_NESTING}")
        if is_id(first[0]):
            rows = [rows] * B
        break
    if not rows:
        return None
    if len(rows) != B:
        raise BofiHipError(f"require_any: {len(rows)} rows for {B} images")
    ban = {int(i) for i in ban_ids or ()}
    clean = []
    for r in rows:
        groups, seen = [], []                                    # seen: (group index, alternative) of the image so far
        for g in (r if r is not None else ()):
            if is_id(g):
                raise BofiHipError(f"require_any: got the bare id {int(g)} where a group is expected: {_ANY_NESTING}")
            alts = []
            for u in (g if g is not None else ()):
                if is_id(u):
                    raise BofiHipError(f"require_any: got the bare id {int(u)} where an alternative is expected: {_ANY_NESTING}")
                if any(not is_id(i) for i in u):
                    raise BofiHipError(f"require_any: an alternative is a list of ids, got {list(u)}: {_ANY_NESTING}")
                u = [int(i) for i in u]
                alts.append(u)
                if not u:
                    continue
                if len(u) > REQUIRE_UNIT_MAX:
                    raise BofiHipError(f"require_any: an alternative holds at most {REQUIRE_UNIT_MAX} ids, got {u}")
                for i in u:
                    if not 0 <= i < V:
                        raise BofiHipError(f"require_any: ids must lie in 0..{V - 1}, got {i} in alternative {u}")
                    if i in ban:
                        raise BofiHipError(f"require_any: id {i} of alternative {u} is also in ban_ids")
                if no_repeat and any(x == y and x >= repeat_min_id for x, y in zip(u, u[1:])):
                    raise BofiHipError(f"require_any: alternative {u} repeats a word (not under no_repeat)")
                for j, v in seen:
                    if v == u:
                        raise BofiHipError(f"require_any: alternative {u} is given twice " + ("in one group" if j == len(groups) else "(in two groups)"))
                    if no_repeat and j != len(groups) and _units_meet(v, u, int(repeat_min_id)):
                        raise BofiHipError(f"require_any: alternatives {v} and {u} of different groups could meet at a shared word and form an adjacent repeat "
                                           "(not under no_repeat)")
                seen.append((len(groups), u))
            while alts and not alts[-1]:
                alts.pop()
            if len(alts) > REQUIRE_ALT_MAX:
                raise BofiHipError(f"require_any: a group holds at most {REQUIRE_ALT_MAX} alternatives, got {len(alts)}: {alts}")
            if alts:
                groups.append(alts)
        if len(groups) > REQUIRE_MAX:
            raise BofiHipError(f"require_any: at most {REQUIRE_MAX} required groups per image, got {len(groups)}")
        clean.append(groups)
    K = max(len(r) for r in clean)
    if K == 0:
        return None
    A = max(len(g) for r in clean for g in r)
    L = max(len(u) for r in clean for g in r for u in g)
    t = np.full((B, K, A, L), -1, np.int32)
    for b, r in enumerate(clean):
        for j, g in enumerate(r):
            for a, u in enumerate(g):
                t[b, j, a, :len(u)] = u
    return torch.from_numpy(t)


def vocab_require_any(x, V, S, seq, alts, pos, which, *, ntok=None, ntok_bias=0, ban=None, no_repeat=False, repeat_min_id=7, row_chosen=None, moved=None):
    """``bofi_vocab_require_any`` on torch tensors: as ``vocab_require_units`` with alts int32 [rows / S, K, A, L] (1 <= K <= ``REQUIRE_MAX``, 1 <= A <=
    ``REQUIRE_ALT_MAX``, 1 <= L <= ``REQUIRE_UNIT_MAX``) in place of the units, pos int32 [rows / S, K] the start of each group's placed alternative and which int32
    [rows / S, K] its index in the group (-1: not placed).  One launch on the current stream, no synchronisation."""
    import torch
    if x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1 or not x.is_cuda:
        raise BofiHipError("vocab_require_any: x must be a 2-d float32 device tensor with unit column stride")
    rows = x.size(0)
    if x.size(1) < V or S < 1 or rows % S:
        raise BofiHipError("vocab_require_any: x needs V columns and a multiple of S rows")
    B = rows // S
    if alts is None or alts.dim() != 4 or alts.size(0) != B:
        raise BofiHipError(f"vocab_require_any: alts must be int32 [{B}, K, A, L]")
    K, A, L = alts.size(1), alts.size(2), alts.size(3)
    for name, t, dt, n in (("seq", seq, torch.int64, rows), ("alts", alts, torch.int32, B * K * A * L), ("pos", pos, torch.int32, B * K), ("which", which, torch.int32, B * K),
                           ("ntok", ntok, torch.int32, B), ("ban", ban, torch.int32, (V + 31) // 32), ("row_chosen", row_chosen, torch.float32, rows),
                           ("moved", moved, torch.int32, B)):
        if t is None and name not in ("seq", "alts", "pos", "which"):
            continue
        if t is None or t.dtype != dt or t.numel() != n or not t.is_cuda or not t.is_contiguous():
            raise BofiHipError(f"vocab_require_any: {name} must be a contiguous {dt} device tensor of {n} elements")
    check(lib().bofi_vocab_require_any(ptr(x), x.stride(0), rows, int(V), int(S), ptr(ntok), int(ntok_bias), ptr(alts), int(K), int(A), int(L), ptr(ban),
                                       1 if no_repeat else 0, int(repeat_min_id), ptr(seq), ptr(row_chosen), ptr(pos), ptr(which), ptr(moved), stream_ptr()),
          "bofi_vocab_require_any")


def vocab_nbest(x, V, S, N, *, ntok=None, ntok_bias=0, pad_idx=0, ban=None, seq_n=None, total=None, count=None, work=None):
    """``bofi_vocab_nbest`` on torch tensors: the N most probable captions of the rows x float32 [rows, >= V] (device, unit column stride, any 4-byte alignment; read
    only), ntok int32 [rows / S] or None, ban the bit table of ``ban_bits`` or None.  Returns ``(seq_n int64 [B, N, S], total float64 [B, N], count int32 [B])``; each may
    be given (contiguous, on the device), as may ``work``, an int32 workspace of at least ``bofi_vocab_nbest_workspace(rows)`` bytes.  Two launches on the current stream,
    no synchronisation."""
    import torch
    if x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1 or not x.is_cuda:
        raise BofiHipError("vocab_nbest: x must be a 2-d float32 device tensor with unit column stride")
    rows = x.size(0)
    if x.size(1) < V or S < 1 or rows % S:
        raise BofiHipError("vocab_nbest: x needs V columns and a multiple of S rows")
    N = int(N)
    if not 1 <= N <= NBEST_MAX:
        raise BofiHipError(f"vocab_nbest: N must lie in 1..{NBEST_MAX}, got {N}")
    B = rows // S
    if seq_n is None:
        seq_n = torch.empty(B, N, S, dtype=torch.int64, device=x.device)
    if total is None:
        total = torch.empty(B, N, dtype=torch.float64, device=x.device)
    if count is None:
        count = torch.empty(B, dtype=torch.int32, device=x.device)
    if work is None:
        work = torch.empty(max(1, lib().bofi_vocab_nbest_workspace(rows) // 4), dtype=torch.int32, device=x.device)
    for name, t, dt, n in (("seq_n", seq_n, torch.int64, B * N * S), ("total", total, torch.float64, B * N), ("count", count, torch.int32, B),
                           ("ntok", ntok, torch.int32, B), ("ban", ban, torch.int32, (V + 31) // 32), ("work", work, torch.int32, None)):
        if t is None and name in ("ntok", "ban"):
            continue
        if t is None or t.dtype != dt or (n is not None and t.numel() != n) or not t.is_cuda or not t.is_contiguous():
            raise BofiHipError(f"vocab_nbest: {name} must be a contiguous {dt} device tensor" + ("" if n is None else f" of {n} elements"))
    check(lib().bofi_vocab_nbest(ptr(x), x.stride(0), rows, int(V), int(S), ptr(ntok), int(ntok_bias), int(pad_idx), ptr(ban), N, ptr(seq_n), ptr(total), ptr(count),
                                 ptr(work), work.numel() * 4, stream_ptr()), "bofi_vocab_nbest")
    return seq_n, total, count


def vocab_nbest_norepeat(x, V, S, N, *, ntok=None, ntok_bias=0, pad_idx=0, ban=None, repeat_min_id=7, seq_n=None, total=None, count=None, work=None):
    """``bofi_vocab_nbest_norepeat`` on torch tensors: the N most probable captions with no adjacent repeated word (an id >= ``repeat_min_id`` never follows itself) of the
    rows x float32 [rows, >= V]; the arguments, the results ``(seq_n int64 [B, N, S], total float64 [B, N], count int32 [B])`` and the workspace are ``vocab_nbest``'s,
    N lies in 1..6, and ``count`` may be 0.  Two launches on the current stream, no synchronisation."""
    import torch
    if x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1 or not x.is_cuda:
        raise BofiHipError("vocab_nbest_norepeat: x must be a 2-d float32 device tensor with unit column stride")
    rows = x.size(0)
    if x.size(1) < V or S < 1 or rows % S:
        raise BofiHipError("vocab_nbest_norepeat: x needs V columns and a multiple of S rows")
    N = int(N)
    if not 1 <= N <= NBEST_NR_MAX:
        raise BofiHipError(f"vocab_nbest_norepeat: N must lie in 1..{NBEST_NR_MAX}, got {N}")
    B = rows // S
    if seq_n is None:
        seq_n = torch.empty(B, N, S, dtype=torch.int64, device=x.device)
    if total is None:
        total = torch.empty(B, N, dtype=torch.float64, device=x.device)
    if count is None:
        count = torch.empty(B, dtype=torch.int32, device=x.device)
    if work is None:
        work = torch.empty(max(1, lib().bofi_vocab_nbest_workspace(rows) // 4), dtype=torch.int32, device=x.device)
    for name, t, dt, n in (("seq_n", seq_n, torch.int64, B * N * S), ("total", total, torch.float64, B * N), ("count", count, torch.int32, B),
                           ("ntok", ntok, torch.int32, B), ("ban", ban, torch.int32, (V + 31) // 32), ("work", work, torch.int32, None)):
        if t is None and name in ("ntok", "ban"):
            continue
        if t is None or t.dtype != dt or (n is not None and t.numel() != n) or not t.is_cuda or not t.is_contiguous():
            raise BofiHipError(f"vocab_nbest_norepeat: {name} must be a contiguous {dt} device tensor" + ("" if n is None else f" of {n} elements"))
    check(lib().bofi_vocab_nbest_norepeat(ptr(x), x.stride(0), rows, int(V), int(S), ptr(ntok), int(ntok_bias), int(pad_idx), ptr(ban), int(repeat_min_id), N,
                                          ptr(seq_n), ptr(total), ptr(count), ptr(work), work.numel() * 4, stream_ptr()), "bofi_vocab_nbest_norepeat")
    return seq_n, total, count


def diverse_check(N, lam, no_repeat=False, repeat_min_id=7, what="vocab_diverse"):
    """The host-side range checks of a diverse set: (N, lambda) as int and float; BofiHipError naming ``what`` for N outside 1..8 (1..6 under the repeat rule), a lambda
    that is negative, NaN or infinite, or a negative ``repeat_min_id``."""
    N, lam = int(N), float(lam)
    top = DIVERSE_NR_MAX if no_repeat else DIVERSE_MAX
    if not 1 <= N <= top:
        raise BofiHipError(f"{what}: N must lie in 1..{top}" + (" under the repeat rule (it needs N + 2 of a row's 8 candidate ids)" if no_repeat else "") + f", got {N}")
    if not (lam >= 0.0) or lam == float("inf"):
        raise BofiHipError(f"{what}: lambda must be finite and >= 0, got {lam}")
    if no_repeat and int(repeat_min_id) < 0:
        raise BofiHipError(f"{what}: repeat_min_id must be >= 0, got {repeat_min_id}")
    return N, lam


def vocab_diverse(x, V, S, N, *, lam=0.5, no_repeat=False, repeat_min_id=7, ntok=None, ntok_bias=0, pad_idx=0, ban=None, seq_n=None, total=None, aug=None, count=None,
                  work=None):
    """``bofi_vocab_diverse`` on torch tensors: the Hamming-diverse set of N captions of the rows x float32 [rows, >= V] (device, unit column stride, any 4-byte alignment;
    read only) -- group g is the exact maximiser of the sum of x minus ``lam`` times the number of earlier groups with the same id at the same position, with
    ``no_repeat`` over the captions in which no id >= ``repeat_min_id`` follows itself (N <= 6 then).  Returns ``(seq_n int64 [B, N, S], total float64 [B, N], aug
    float64 [B, N], count int32 [B])``: each caption's own log-prob and its augmented score; the buffers and ``work`` (``vocab_nbest``'s workspace) may be given.  Two
    launches on the current stream, no synchronisation."""
    import torch
    if x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1 or not x.is_cuda:
        raise BofiHipError("vocab_diverse: x must be a 2-d float32 device tensor with unit column stride")
    rows = x.size(0)
    if x.size(1) < V or S < 1 or rows % S:
        raise BofiHipError("vocab_diverse: x needs V columns and a multiple of S rows")
    N, lam = diverse_check(N, lam, no_repeat, repeat_min_id)
    B = rows // S
    if seq_n is None:
        seq_n = torch.empty(B, N, S, dtype=torch.int64, device=x.device)
    if total is None:
        total = torch.empty(B, N, dtype=torch.float64, device=x.device)
    if aug is None:
        aug = torch.empty(B, N, dtype=torch.float64, device=x.device)
    if count is None:
        count = torch.empty(B, dtype=torch.int32, device=x.device)
    if work is None:
        work = torch.empty(max(1, lib().bofi_vocab_nbest_workspace(rows) // 4), dtype=torch.int32, device=x.device)
    for name, t, dt, n in (("seq_n", seq_n, torch.int64, B * N * S), ("total", total, torch.float64, B * N), ("aug", aug, torch.float64, B * N),
                           ("count", count, torch.int32, B), ("ntok", ntok, torch.int32, B), ("ban", ban, torch.int32, (V + 31) // 32), ("work", work, torch.int32, None)):
        if t is None and name in ("ntok", "ban"):
            continue
        if t is None or t.dtype != dt or (n is not None and t.numel() != n) or not t.is_cuda or not t.is_contiguous():
            raise BofiHipError(f"vocab_diverse: {name} must be a contiguous {dt} device tensor" + ("" if n is None else f" of {n} elements"))
    check(lib().bofi_vocab_diverse(ptr(x), x.stride(0), rows, int(V), int(S), ptr(ntok), int(ntok_bias), int(pad_idx), ptr(ban), N, lam, 1 if no_repeat else 0,
                                   int(repeat_min_id), ptr(seq_n), ptr(total), ptr(aug), ptr(count), ptr(work), work.numel() * 4, stream_ptr()), "bofi_vocab_diverse")
    return seq_n, total, aug, count


def gemm_flops(reset: bool = False):
    """(GEMM FLOPs enqueued since the last reset, the part of them in early-out launches) -- host-side tally of the library."""
    sk = C.c_double(0.0)
    v = lib().bofi_gemm_flops(1 if reset else 0, C.cast(C.byref(sk), C.c_void_p))
    return float(v), float(sk.value)
