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
//
// bofi_pack_regions_box (further down) is the same launch for the loader's use_box mode (dataloader.py:477-487): five box-geometry columns behind the
// attention columns, every image's rows sorted by box area, the width zero-padded to an aligned F_out.  Both kernels move a row with move_row.
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

// One row's `chunks` 8-element chunks from rows + src to out + dst, divided by the row's L2 norm when NORM: the whole wavefront calls it.
template <int IN, int OUT, bool NORM>
__device__ __forceinline__ void move_row(const void* __restrict__ rows, int64_t src, void* __restrict__ out, int64_t dst, int chunks, int lane) {
    float v[CHUNK];
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
    move_row<IN, OUT, NORM>(rows, ((int64_t)first + r) * F, out, dst, chunks, lane);
}

template <int IN, int OUT>
void launch(bool norm, dim3 grid, hipStream_t st, const void* rows, const int* offsets, int B, int F, void* out, int out_R, int* att_len) {
    if (norm)
        hipLaunchKernelGGL((pack_regions_kernel<IN, OUT, true>), grid, dim3(WAVE * ROWS), 0, st, rows, offsets, B, F, out, out_R, att_len);
    else
        hipLaunchKernelGGL((pack_regions_kernel<IN, OUT, false>), grid, dim3(WAVE * ROWS), 0, st, rows, offsets, B, F, out, out_R, att_len);
}

// ---- use_box (dataloader.py:477-487): five geometry columns behind the attention columns, the image's rows sorted by the last of them
constexpr int MAX_R = 1024;       // regions per image the key table in LDS holds (4 KB)
constexpr int BOX_COLS = 5;

// x1/w, y1/h, x2/w, y2/h, (x2-x1)(y2-y1)/(w h) of one box in float32, every operation rounded on its own in numpy's order; norm_box: each divided
// by sqrtf(((((c0^2 + c1^2) + c2^2) + c3^2) + c4^2)).  The library is built with contraction on, and this toolchain's __fmul_rn / __fadd_rn are the plain
// operators inside header functions (they would fuse after inlining), so the operations are written out under `fp contract(off)`: no fma, no reciprocal.
__device__ __forceinline__ void box_cols(const float* __restrict__ boxes, int64_t row, int w, int h, bool norm_box, float* c) {
#pragma clang fp contract(off)
    const f32x4 q = *reinterpret_cast<const f32x4*>(boxes + row * 4);      // x1, y1, x2, y2
    const float fw = (float)w, fh = (float)h, fa = (float)((int64_t)w * (int64_t)h);
    c[0] = q[0] / fw;
    c[1] = q[1] / fh;
    c[2] = q[2] / fw;
    c[3] = q[3] / fh;
    const float dx = q[2] - q[0], dy = q[3] - q[1];
    const float area = dx * dy;
    c[4] = area / fa;
    if (norm_box) {
        float s = c[0] * c[0];
        for (int i = 1; i < BOX_COLS; ++i) {
            const float sq = c[i] * c[i];
            s = s + sq;
        }
        const float nrm = sqrtf(s);
        for (int i = 0; i < BOX_COLS; ++i) c[i] = c[i] / nrm;
    }
}

// does row j (key kj) stand before row i (key ki) in the descending stable order?  A NaN key stands after every number; NaNs keep their source order.
__device__ __forceinline__ bool stands_before(float kj, int j, float ki, int i) {
    const bool nj = kj != kj, ni = ki != ki;
    if (nj || ni) return nj == ni ? j < i : ni;
    return kj > ki || (kj == ki && j < i);
}

// Grid: per image ceil(out_R / ROWS) workgroups, so a workgroup's four rows belong to ONE image.  Every workgroup computes its image's keys (the last box
// column of every real row) into LDS, all four wavefronts pass the one barrier, and then wavefront `wave` owns row index r = 4 * slot + wave: as SOURCE row r
// of the image when r < len -- it counts the rows that stand before it and writes to that rank, a permutation of 0 .. len - 1 -- and as the zero PADDING
// row r when len <= r < out_R.  Writes are bounded by out_R alone (rank < len <= out_R), reads by the clamped len.
template <int IN, int OUT, bool NORM>
__global__ void __launch_bounds__(WAVE * ROWS) pack_regions_box_kernel(const void* __restrict__ rows, const float* __restrict__ boxes, const int* __restrict__ wh,
                                                                      const int* __restrict__ offsets, int F_att, void* __restrict__ out, int out_R, int F_out,
                                                                      int norm_box, int* __restrict__ att_len, int slots) {
    __shared__ float keys[MAX_R];
    const int lane = threadIdx.x % WAVE;
    const int b = blockIdx.x / slots, r = (blockIdx.x % slots) * ROWS + threadIdx.x / WAVE;
    const int first = offsets[b];
    const int len = min(min(max(offsets[b + 1] - first, 0), out_R), MAX_R);
    const int w = wh[2 * b], h = wh[2 * b + 1];
    float c[BOX_COLS];
    for (int i = threadIdx.x; i < len; i += WAVE * ROWS) {
        box_cols(boxes, (int64_t)first + i, w, h, norm_box != 0, c);
        keys[i] = c[BOX_COLS - 1];
    }
    __syncthreads();                                             // (no wavefront has left before this point)
    if (r >= out_R) return;                                      // the image's last workgroup: rows past out_R
    if (att_len && r == 0 && lane == 0) att_len[b] = len;
    float v[CHUNK];
    if (r >= len) {                                              // padding: store only
        for (int i = 0; i < CHUNK; ++i) v[i] = 0.0f;
        const int64_t dst = ((int64_t)b * out_R + r) * F_out;
        for (int k = lane; k < F_out / CHUNK; k += WAVE) store8<OUT>(out, dst + (int64_t)k * CHUNK, v);
        return;
    }
    const float key = keys[r];
    int before = 0;
    for (int j = lane; j < len; j += WAVE) before += stands_before(keys[j], j, key, r) ? 1 : 0;
    // (at most 16 per lane, at most 1023 in all: exact in float32; all 64 lanes are here)
    const int rank = min(__builtin_amdgcn_readfirstlane((int)bofi::wave_sum((float)before)), len - 1);
    const int64_t dst = ((int64_t)b * out_R + rank) * F_out;
    move_row<IN, OUT, NORM>(rows, ((int64_t)first + r) * F_att, out, dst, F_att / CHUNK, lane);
    box_cols(boxes, (int64_t)first + r, w, h, norm_box != 0, c);
    for (int k = lane; k < (F_out - F_att) / CHUNK; k += WAVE) {   // the box columns and the zero columns up to F_out
        for (int i = 0; i < CHUNK; ++i) v[i] = (k == 0 && i < BOX_COLS) ? c[i] : 0.0f;
        store8<OUT>(out, dst + F_att + (int64_t)k * CHUNK, v);
    }
}

template <int IN, int OUT>
void launch_box(bool norm, dim3 grid, hipStream_t st, const void* rows, const float* boxes, const int* wh, const int* offsets, int F_att, void* out, int out_R, int F_out,
                int norm_box, int* att_len, int slots) {
    if (norm)
        hipLaunchKernelGGL((pack_regions_box_kernel<IN, OUT, true>), grid, dim3(WAVE * ROWS), 0, st, rows, boxes, wh, offsets, F_att, out, out_R, F_out, norm_box, att_len, slots);
    else
        hipLaunchKernelGGL((pack_regions_box_kernel<IN, OUT, false>), grid, dim3(WAVE * ROWS), 0, st, rows, boxes, wh, offsets, F_att, out, out_R, F_out, norm_box, att_len, slots);
}

}  // namespace

extern "C" int bofi_pack_regions_box(const void* rows, int rows_dtype, const float* boxes, const int* wh, const int* wh_host, const int* offsets, const int* offsets_host,
                                     int B, int F_att, void* out, int out_dtype, int out_R, int F_out, int norm_att, int norm_box, int* att_len, void* stream) {
    const char* const me = "bofi_pack_regions_box: ";
    if (!rows || !boxes || !wh || !offsets || !out) return bofi::fail(BOFI_ERR_ARG, std::string(me) + "rows, boxes, wh, offsets and out must be given");
    if (B < 1) return bofi::fail(BOFI_ERR_ARG, std::string(me) + "B >= 1 expected, got B = " + std::to_string(B));
    if (out_R < 1 || out_R > MAX_R) return bofi::fail(BOFI_ERR_ARG, std::string(me) + "out_R = " + std::to_string(out_R) + " is outside 1 .. 1024 (the key table of an image)");
    if (F_att < CHUNK || F_att % CHUNK != 0) return bofi::fail(BOFI_ERR_ARG, std::string(me) + "F_att = " + std::to_string(F_att) + " is not a multiple of 8 (16-byte vectors)");
    if (F_out % CHUNK != 0 || (int64_t)F_out < (int64_t)F_att + BOX_COLS)
        return bofi::fail(BOFI_ERR_ARG, std::string(me) + "F_out = " + std::to_string(F_out) + ": a multiple of 8 that is at least F_att + 5 = " + std::to_string((int64_t)F_att + BOX_COLS));
    if (rows_dtype != BOFI_DT_F32 && rows_dtype != BOFI_DT_BF16 && rows_dtype != BOFI_DT_F16)
        return bofi::fail(BOFI_ERR_ARG, std::string(me) + "rows_dtype " + std::to_string(rows_dtype) + ": float32 (0), bfloat16 (1) or float16 (2)");
    if (out_dtype != BOFI_DT_F32 && out_dtype != BOFI_DT_BF16) return bofi::fail(BOFI_ERR_ARG, std::string(me) + "out_dtype " + std::to_string(out_dtype) + ": float32 (0) or bfloat16 (1)");
    if ((norm_att != 0 && norm_att != 1) || (norm_box != 0 && norm_box != 1)) return bofi::fail(BOFI_ERR_ARG, std::string(me) + "norm_att and norm_box are 0 or 1");
    if (((uintptr_t)rows | (uintptr_t)out | (uintptr_t)boxes) % 16 != 0) return bofi::fail(BOFI_ERR_ARG, std::string(me) + "rows, boxes and out must be 16-byte aligned");
    const int slots = (out_R + ROWS - 1) / ROWS;
    const int64_t blocks = (int64_t)B * slots;
    if (blocks > 0x7FFFFFFF) return bofi::fail(BOFI_ERR_ARG, std::string(me) + "B * out_R is too large for one launch");
    if (offsets_host) {
        if (offsets_host[0] != 0) return bofi::fail(BOFI_ERR_ARG, std::string(me) + "offsets[0] = " + std::to_string(offsets_host[0]) + ", expected 0");
        for (int b = 0; b < B; ++b) {
            const int len = offsets_host[b + 1] - offsets_host[b];
            if (len < 0) return bofi::fail(BOFI_ERR_ARG, std::string(me) + "offsets decrease at image " + std::to_string(b));
            if (len > out_R) return bofi::fail(BOFI_ERR_ARG, std::string(me) + "image " + std::to_string(b) + " has " + std::to_string(len) + " regions, out_R = " + std::to_string(out_R));
        }
    }
    if (wh_host)
        for (int b = 0; b < B; ++b)
            if (wh_host[2 * b] < 1 || wh_host[2 * b + 1] < 1)
                return bofi::fail(BOFI_ERR_ARG, std::string(me) + "image " + std::to_string(b) + " is " + std::to_string(wh_host[2 * b]) + " x " + std::to_string(wh_host[2 * b + 1]) +
                                                    " pixels: width and height >= 1 expected");
    const dim3 grid((unsigned)blocks);
    hipStream_t st = (hipStream_t)stream;
#define BOFI_PACK_CASE(IN, OUT) \
    if (rows_dtype == IN && out_dtype == OUT) launch_box<IN, OUT>(norm_att != 0, grid, st, rows, boxes, wh, offsets, F_att, out, out_R, F_out, norm_box, att_len, slots)
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
