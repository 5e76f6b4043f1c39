// The region side of the loader's collate (captioning/data/dataloader.py:326-338) and its optional norm_att_feat (:475-476), on the device.
//
// Input: a batch staged RAGGED -- the images' real region rows back to back, [offsets[B], F] in the dtype of the feature files (float32,
// float16 or bfloat16) -- and int32 offsets [B + 1].  Output: what the engine and the trainer consume, [B, out_R, F] zero-padded in float32
// or bfloat16, plus the region counts.  The padding is produced here, so it never crosses the host link.
//
// One wavefront per OUTPUT row, four rows per workgroup.  A lane moves chunks of 8 elements (lane, lane + 64, ...: lanes beyond F / 8 are idle)
// with 16-byte loads and stores: one load and two stores for half-width -> float32, two loads and one store for float32 -> bfloat16.  A padding
// row (r >= len_b) is a store-only path.  len_b is clamped to [0, out_R] whatever the device array holds, and the output address is a function
// of the row index alone, so nothing is ever written outside out.
//
// norm: x / ||x||_2 per row.  Every lane sums the squares of its elements serially in float32 (fmaf, chunk after chunk: F / 64 additions), a
// fixed butterfly over the 64 lanes follows (bofi::wave_sum: 6 additions, every lane ends with the same bits), then sqrtf and ONE DIVISION per
// element -- the reference's operation, not a multiplication by a reciprocal.  No atomics, a fixed order: bit-identical run to run.  A row of
// zeros is 0 / 0 = NaN in every element, as numpy gives it.  The row is read a second time for the division (8 KB at F = 2048: from cache).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "bofi_common.h"
#include "boficap_hip.h"

namespace {

using bofi::f32x4;
using bofi::u32x4;

constexpr int WAVE = 64;
constexpr int ROWS = 4;           // output rows (wavefronts) per workgroup
constexpr int CHUNK = 8;          // elements per lane and step

typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;

template <int DT> __device__ __forceinline__ void load8(const void* base, int64_t at, float* v);
template <> __device__ __forceinline__ void load8<BOFI_DT_F32>(const void* base, int64_t at, float* v) {
    const f32x4* p = reinterpret_cast<const f32x4*>(static_cast<const float*>(base) + at);
    const f32x4 a = p[0], b = p[1];
    for (int i = 0; i < 4; ++i) { v[i] = a[i]; v[4 + i] = b[i]; }
}
template <> __device__ __forceinline__ void load8<BOFI_DT_BF16>(const void* base, int64_t at, float* v) {
    const u32x4 a = *reinterpret_cast<const u32x4*>(static_cast<const uint16_t*>(base) + at);
    for (int i = 0; i < 4; ++i) { v[2 * i] = __uint_as_float(a[i] << 16); v[2 * i + 1] = __uint_as_float(a[i] & 0xFFFF0000u); }
}
template <> __device__ __forceinline__ void load8<BOFI_DT_F16>(const void* base, int64_t at, float* v) {
    const f16x8 a = *reinterpret_cast<const f16x8*>(static_cast<const uint16_t*>(base) + at);
    for (int i = 0; i < CHUNK; ++i) v[i] = (float)a[i];          // exact
}

template <int DT> __device__ __forceinline__ void store8(void* base, int64_t at, const float* v);
template <> __device__ __forceinline__ void store8<BOFI_DT_F32>(void* base, int64_t at, const float* v) {
    f32x4* p = reinterpret_cast<f32x4*>(static_cast<float*>(base) + at);
    const f32x4 a = {v[0], v[1], v[2], v[3]}, b = {v[4], v[5], v[6], v[7]};
    p[0] = a;
    p[1] = b;
}
template <> __device__ __forceinline__ void store8<BOFI_DT_BF16>(void* base, int64_t at, const float* v) {      // round to nearest even
    const u32x4 a = {bofi::pack_bf16(v[0], v[1]), bofi::pack_bf16(v[2], v[3]), bofi::pack_bf16(v[4], v[5]), bofi::pack_bf16(v[6], v[7])};
    *reinterpret_cast<u32x4*>(static_cast<uint16_t*>(base) + at) = a;
}

template <int IN, int OUT, bool NORM>
__global__ void __launch_bounds__(WAVE * ROWS) pack_regions_kernel(const void* __restrict__ rows, const int* __restrict__ offsets, int B, int F, void* __restrict__ out,
                                                                  int out_R, int* __restrict__ att_len) {
    const int lane = threadIdx.x % WAVE;
    const int64_t g = (int64_t)blockIdx.x * ROWS + threadIdx.x / WAVE;          // output row
    if (g >= (int64_t)B * out_R) return;                         // the last workgroup's tail: whole wavefronts leave
    const int b = (int)(g / out_R), r = (int)(g % out_R);
    const int first = offsets[b];                                // (READS are not guarded: a corrupt device array can point src outside rows -- the wrapper's check of the host copy is the guard)
    const int len = min(max(offsets[b + 1] - first, 0), out_R);
    if (att_len && r == 0 && lane == 0) att_len[b] = len;
    const int chunks = F / CHUNK;
    const int64_t dst = g * F;
    float v[CHUNK];
    if (r >= len) {                                              // padding: store only
        for (int i = 0; i < CHUNK; ++i) v[i] = 0.0f;
        for (int c = lane; c < chunks; c += WAVE) store8<OUT>(out, dst + (int64_t)c * CHUNK, v);
        return;
    }
    const int64_t src = ((int64_t)first + r) * F;
    if (NORM) {
        float acc = 0.0f;
        for (int c = lane; c < chunks; c += WAVE) {
            load8<IN>(rows, src + (int64_t)c * CHUNK, v);
            for (int i = 0; i < CHUNK; ++i) acc = fmaf(v[i], v[i], acc);
        }
        const float nrm = sqrtf(bofi::wave_sum(acc));             // all 64 lanes are here (idle ones carry 0)
        for (int c = lane; c < chunks; c += WAVE) {
            load8<IN>(rows, src + (int64_t)c * CHUNK, v);
            for (int i = 0; i < CHUNK; ++i) v[i] = v[i] / nrm;
            store8<OUT>(out, dst + (int64_t)c * CHUNK, v);
        }
    } else {
        for (int c = lane; c < chunks; c += WAVE) {
            load8<IN>(rows, src + (int64_t)c * CHUNK, v);
            store8<OUT>(out, dst + (int64_t)c * CHUNK, v);
        }
    }
}

template <int IN, int OUT>
void launch(bool norm, dim3 grid, hipStream_t st, const void* rows, const int* offsets, int B, int F, void* out, int out_R, int* att_len) {
    if (norm)
        hipLaunchKernelGGL((pack_regions_kernel<IN, OUT, true>), grid, dim3(WAVE * ROWS), 0, st, rows, offsets, B, F, out, out_R, att_len);
    else
        hipLaunchKernelGGL((pack_regions_kernel<IN, OUT, false>), grid, dim3(WAVE * ROWS), 0, st, rows, offsets, B, F, out, out_R, att_len);
}

}  // namespace

extern "C" int bofi_pack_regions(const void* rows, int rows_dtype, const int* offsets, const int* offsets_host, int B, int F, void* out, int out_dtype,
                                 int out_R, int norm, int* att_len, void* stream) {
    const char* const me = "bofi_pack_regions: ";
    if (!rows || !offsets || !out) return bofi::fail(BOFI_ERR_ARG, std::string(me) + "rows, offsets and out must be given");
    if (B < 1 || out_R < 1) return bofi::fail(BOFI_ERR_ARG, std::string(me) + "B >= 1 and out_R >= 1 expected, got B = " + std::to_string(B) + ", out_R = " + std::to_string(out_R));
    if (F < CHUNK || F % CHUNK != 0) return bofi::fail(BOFI_ERR_ARG, std::string(me) + "F = " + std::to_string(F) + " is not a multiple of 8 (16-byte vectors)");
    if (rows_dtype != BOFI_DT_F32 && rows_dtype != BOFI_DT_BF16 && rows_dtype != BOFI_DT_F16)
        return bofi::fail(BOFI_ERR_ARG, std::string(me) + "rows_dtype " + std::to_string(rows_dtype) + ": float32 (0), bfloat16 (1) or float16 (2)");
    if (out_dtype != BOFI_DT_F32 && out_dtype != BOFI_DT_BF16) return bofi::fail(BOFI_ERR_ARG, std::string(me) + "out_dtype " + std::to_string(out_dtype) + ": float32 (0) or bfloat16 (1)");
    if ((norm != 0 && norm != 1)) return bofi::fail(BOFI_ERR_ARG, std::string(me) + "norm is 0 or 1");
    if (((uintptr_t)rows | (uintptr_t)out) % 16 != 0) return bofi::fail(BOFI_ERR_ARG, std::string(me) + "rows and out must be 16-byte aligned");
    const int64_t blocks = ((int64_t)B * out_R + ROWS - 1) / ROWS;
    if (blocks > 0x7FFFFFFF) return bofi::fail(BOFI_ERR_ARG, std::string(me) + "B * out_R is too large for one launch");
    if (offsets_host) {
        if (offsets_host[0] != 0) return bofi::fail(BOFI_ERR_ARG, std::string(me) + "offsets[0] = " + std::to_string(offsets_host[0]) + ", expected 0");
        for (int b = 0; b < B; ++b) {
            const int len = offsets_host[b + 1] - offsets_host[b];
            if (len < 0) return bofi::fail(BOFI_ERR_ARG, std::string(me) + "offsets decrease at image " + std::to_string(b));
            if (len > out_R) return bofi::fail(BOFI_ERR_ARG, std::string(me) + "image " + std::to_string(b) + " has " + std::to_string(len) + " regions, out_R = " + std::to_string(out_R));
        }
    }
    const dim3 grid((unsigned)blocks);
    hipStream_t st = (hipStream_t)stream;
#define BOFI_PACK_CASE(IN, OUT) \
    if (rows_dtype == IN && out_dtype == OUT) launch<IN, OUT>(norm != 0, grid, st, rows, offsets, B, F, out, out_R, att_len)
    BOFI_PACK_CASE(BOFI_DT_F32, BOFI_DT_F32);
    BOFI_PACK_CASE(BOFI_DT_F32, BOFI_DT_BF16);
    BOFI_PACK_CASE(BOFI_DT_BF16, BOFI_DT_F32);
    BOFI_PACK_CASE(BOFI_DT_BF16, BOFI_DT_BF16);
    BOFI_PACK_CASE(BOFI_DT_F16, BOFI_DT_F32);
    BOFI_PACK_CASE(BOFI_DT_F16, BOFI_DT_BF16);
#undef BOFI_PACK_CASE
    if (hipGetLastError() != hipSuccess) return bofi::fail(BOFI_ERR_HIP, std::string(me) + "the launch failed");
    return BOFI_OK;
}
