// Word-to-region attention maps: the cross-attention PROBABILITIES of one decoder layer, which the fused attention sublayers never leave in memory
// (reference: MultiHeadedAttention keeps self.attn, TransformerModel.py:1459; after a mode='sample' call model.decoder.layers[-1].src_attn.attn is the
// [B, h, 20, R] map of the filling pass).  From the queries q [B*Lq, ldq] and keys k [B*Lk, ldk] the sublayer itself read (compute dtype, d_k = 64):
//   A[b,h,t,r] = softmax over r < len_b of (q[b,t,h,:] . k[b,r,h,:] * scale),  len_b = klen[b] (clamped to 0 .. Lk) or Lk
//   A[b,h,t,r] = +0.0 for len_b <= r < Lk -- unless the row's sum is NaN (a NaN or +inf score): then ALL Lk entries of the row are NaN, as the reference's
//                softmax over the masked_fill'ed scores leaves them
//   M[b,t,r]   = (A[b,0,t,r] + A[b,1,t,r] + ... in head order) / H
//   top[b,t,j], topw[b,t,j], j < K: the K largest M[b,t,:len_b] in descending order, equal weights by lower region index, topw = M's own floats; slots past len_b:
//                (-1, 0); a NaN row: (-1, NaN) in every slot; rows t >= qlen[b] + qlen_bias (no word laid out there): (-1, 0) -- M and A are written for them all the same.
// Everything is float32 from the inputs as stored (bf16 -> f32 is exact): four 16-term FMA chains per score, max-subtracted expf, fixed-order wave reductions, no atomics.
//
// Latency-bound (24 MFLOP at 64 x 8 x 20 x 36): one workgroup per image -- per chunk of TQ query rows of an image where that fills more of the chip or the LDS
// budget asks for it --, one wavefront per head (looping when H > 8), lane <-> key (two keys per lane beyond 64).
// The image's query rows are staged in LDS as float32 and read as broadcasts; a lane keeps its key row in registers for all query rows.  The heads' probabilities
// meet in LDS, [H][TQ][64 | 128] floats, and are summed in head order after one barrier; the top-K is K rounds of wave-max + ballot per row of M.  Rows do not depend on
// each other, so the chunking changes no result.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>

#include "bofi_common.h"
#include "bofi_kernels.h"
#include "boficap_hip.h"

namespace {

using namespace bofi;

constexpr int DK = 64;
constexpr int NW = 8;                          // wavefronts per workgroup
constexpr int NT = NW * WAVE;
constexpr int AM_LDS_MAX = 144 * 1024;         // of the CU's 160 KB
constexpr int AM_TARGET_WGS = 512;             // two workgroups per CU

// key row r's 64 elements of one head as float32; vec: 16-byte loads (pointer and pitch allow them)
__device__ __forceinline__ void load_row(const float* p, bool vec, float (&kr)[DK]) {
    if (vec) {
#pragma unroll
        for (int i = 0; i < DK / 4; ++i) {
            const float4 v = reinterpret_cast<const float4*>(p)[i];
            kr[4 * i] = v.x; kr[4 * i + 1] = v.y; kr[4 * i + 2] = v.z; kr[4 * i + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < DK; ++i) kr[i] = p[i];
    }
}
__device__ __forceinline__ void load_row(const bf16_t* p, bool vec, float (&kr)[DK]) {
    if (vec) {
#pragma unroll
        for (int i = 0; i < DK / 8; ++i) {
            const uint4 v = reinterpret_cast<const uint4*>(p)[i];
            const uint32_t u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                kr[8 * i + 2 * j] = __uint_as_float(u[j] << 16);
                kr[8 * i + 2 * j + 1] = __uint_as_float(u[j] & 0xffff0000u);
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < DK; ++i) kr[i] = bf16_to_f32(p[i]);
    }
}

// 16 bytes of a query row as float32 into LDS (dst 16-byte aligned)
template <typename T> __device__ __forceinline__ void stage16(const uint4& v, float* dst);
template <> __device__ __forceinline__ void stage16<float>(const uint4& v, float* dst) {
    *reinterpret_cast<float4*>(dst) = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}
template <> __device__ __forceinline__ void stage16<bf16_t>(const uint4& v, float* dst) {
    reinterpret_cast<float4*>(dst)[0] = make_float4(__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xffff0000u), __uint_as_float(v.y << 16), __uint_as_float(v.y & 0xffff0000u));
    reinterpret_cast<float4*>(dst)[1] = make_float4(__uint_as_float(v.z << 16), __uint_as_float(v.z & 0xffff0000u), __uint_as_float(v.w << 16), __uint_as_float(v.w & 0xffff0000u));
}

// grid (B, chunks); TQ: query rows per chunk; LKP: 64 or 128, the probabilities' row pitch in LDS
template <typename T>
__global__ void __launch_bounds__(NT) attn_maps_kernel(AttnMapsArgs a, int TQ, int LKP) {
    extern __shared__ __attribute__((aligned(16))) float am_smem[];
    const int b = blockIdx.x, lane = threadIdx.x % WAVE, w = threadIdx.x / WAVE;
    const int H = a.H, Lq = a.Lq, Lk = a.Lk, K = a.K, HD = H * DK;
    float* const qsm = am_smem;                                // [TQ][H * 64]
    float* const P = am_smem + (size_t)TQ * HD;                // [H][TQ][LKP]
    int len = a.klen ? a.klen[b] : Lk;
    len = len < 0 ? 0 : (len > Lk ? Lk : len);
    int nq = a.qlen ? a.qlen[b] + a.qlen_bias : Lq;
    nq = nq < 0 ? 0 : (nq > Lq ? Lq : nq);
    const T* const q = (const T*)a.q + (size_t)b * Lq * a.ldq;
    const T* const k = (const T*)a.k + (size_t)b * Lk * a.ldk;
    const bool vec = (((uintptr_t)a.k | ((size_t)a.ldk * sizeof(T))) & 15) == 0;       // (a head's offset, 64 elements, keeps the alignment)
    const bool qvec = (((uintptr_t)a.q | ((size_t)a.ldq * sizeof(T))) & 15) == 0;
    const bool two = LKP > WAVE;
    const bool v0 = lane < len, v1 = two && lane + WAVE < len;

    {
        const int t0 = blockIdx.y * TQ;                          // this workgroup's chunk of query rows (the launch makes ceil(Lq / TQ) chunks)
        const int tq = Lq - t0 < TQ ? Lq - t0 : TQ;
        if (qvec) {                                              // 16 bytes per lane, four loads in flight before the first LDS store
            constexpr int E = 16 / (int)sizeof(T), NV = 4;
            const int per_row = HD / E, n = tq * per_row;
            for (int base = 0; base < n; base += NT * NV) {
                uint4 v[NV];
#pragma unroll
                for (int j = 0; j < NV; ++j) {
                    const int i = base + j * NT + (int)threadIdx.x;
                    const int t = i / per_row, c = (i - t * per_row) * E;
                    v[j] = i < n ? *reinterpret_cast<const uint4*>(q + (size_t)(t0 + t) * a.ldq + c) : uint4{0, 0, 0, 0};
                }
#pragma unroll
                for (int j = 0; j < NV; ++j) {
                    const int i = base + j * NT + (int)threadIdx.x;
                    if (i < n) stage16<T>(v[j], qsm + (size_t)i * E);
                }
            }
        } else {
            for (int i = threadIdx.x; i < tq * HD; i += NT) {
                const int t = i / HD, c = i - t * HD;
                qsm[i] = ElemOps<T>::load(q + (size_t)(t0 + t) * a.ldq + c);
            }
        }
        __syncthreads();
        // ---- scores and softmax: wavefront w takes heads w, w + 8, ...
        for (int h = w; h < H; h += NW) {
            float* const Ph = P + (size_t)h * TQ * LKP;
            for (int half = 0; half < (two ? 2 : 1); ++half) {
                const int r = lane + WAVE * half;
                float kr[DK];
                if (r < len) {
                    load_row(k + (size_t)r * a.ldk + h * DK, vec, kr);
                } else {
#pragma unroll
                    for (int i = 0; i < DK; ++i) kr[i] = 0.f;
                }
                for (int t = 0; t < tq; ++t) {
                    const float4* const q4 = reinterpret_cast<const float4*>(qsm + (size_t)t * HD + h * DK);      // (one address per wavefront: a broadcast)
                    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;          // four chains of 16 terms (one chain of 64 waits on itself), closed in a fixed order
#pragma unroll
                    for (int i = 0; i < DK / 4; ++i) {
                        const float4 qv = q4[i];
                        a0 = fmaf(qv.x, kr[4 * i], a0); a1 = fmaf(qv.y, kr[4 * i + 1], a1);
                        a2 = fmaf(qv.z, kr[4 * i + 2], a2); a3 = fmaf(qv.w, kr[4 * i + 3], a3);
                    }
                    Ph[t * LKP + r] = ((a0 + a1) + (a2 + a3)) * a.scale;
                }
            }
            // (a lane reads back its own two scores: no exchange between lanes but the reductions.  Four rows per step: their reduction chains are independent and
            // interleave -- one row at a time the wavefront mostly waits on itself; a short last group computes its last row again and stores it once)
            constexpr int RB = 4;
            for (int tb = 0; tb < tq; tb += RB) {
                float s0[RB], s1[RB], m[RB], e0[RB], e1[RB], sum[RB];
#pragma unroll
                for (int j = 0; j < RB; ++j) {
                    const int t = tb + j < tq ? tb + j : tq - 1;
                    s0[j] = Ph[t * LKP + lane];
                    s1[j] = two ? Ph[t * LKP + WAVE + lane] : 0.f;
                }
#pragma unroll
                for (int j = 0; j < RB; ++j) m[j] = wave_max(fmaxf(v0 ? s0[j] : -INFINITY, v1 ? s1[j] : -INFINITY));
#pragma unroll
                for (int j = 0; j < RB; ++j) {                   // (a NaN score stays NaN whatever fmaxf made of it)
                    e0[j] = v0 ? expf(s0[j] - m[j]) : 0.f;
                    e1[j] = v1 ? expf(s1[j] - m[j]) : 0.f;
                }
#pragma unroll
                for (int j = 0; j < RB; ++j) sum[j] = wave_sum(e0[j] + e1[j]);
#pragma unroll
                for (int j = 0; j < RB; ++j) {
                    const int t = tb + j;
                    if (t >= tq) break;
                    const bool bad = sum[j] != sum[j];
                    const float p0 = v0 ? e0[j] / sum[j] : (bad ? sum[j] : 0.f), p1 = v1 ? e1[j] / sum[j] : (bad ? sum[j] : 0.f);
                    Ph[t * LKP + lane] = p0;
                    if (two) Ph[t * LKP + WAVE + lane] = p1;
                    if (a.heads) {
                        float* const hp = a.heads + (((size_t)b * H + h) * Lq + t0 + t) * Lk;
                        if (lane < Lk) hp[lane] = p0;
                        if (two && lane + WAVE < Lk) hp[lane + WAVE] = p1;
                    }
                }
            }
        }
        __syncthreads();
        // ---- the heads' mean in head order, and its top-K: wavefront w takes rows w, w + 8, ...
        for (int t = w; t < tq; t += NW) {
            float m0 = 0.f, m1 = 0.f;
            for (int h = 0; h < H; ++h) {
                const float* const row = P + ((size_t)h * TQ + t) * LKP;
                m0 += row[lane];
                if (two) m1 += row[WAVE + lane];
            }
            m0 = m0 / (float)H; m1 = m1 / (float)H;
            if (a.mean) {
                float* const mp = a.mean + ((size_t)b * Lq + t0 + t) * Lk;
                if (lane < Lk) mp[lane] = m0;
                if (two && lane + WAVE < Lk) mp[lane + WAVE] = m1;
            }
            if (K > 0) {
                int* const ti = a.top_idx + ((size_t)b * Lq + t0 + t) * K;
                float* const tw = a.top_w + ((size_t)b * Lq + t0 + t) * K;
                const bool off = t0 + t >= nq;
                const bool nan_row = __ballot((v0 && m0 != m0) || (v1 && m1 != m1)) != 0;
                float c0 = v0 ? m0 : -1.f, c1 = v1 ? m1 : -1.f;      // (probabilities are >= +0: -1 marks what is masked or taken)
                for (int j = 0; j < K; ++j) {                    // (every branch is uniform over the wavefront: the reductions see all 64 lanes)
                    int idx = -1;
                    float wt = 0.f;
                    if (off) {
                    } else if (nan_row) {
                        wt = __builtin_nanf("");
                    } else {
                        const float mx = wave_max(fmaxf(c0, c1));
                        if (mx >= 0.f) {
                            const unsigned long long b0 = __ballot(c0 == mx), b1 = __ballot(c1 == mx);
                            idx = b0 ? __builtin_ctzll(b0) : WAVE + __builtin_ctzll(b1);
                            wt = mx;
                            if (idx == lane) c0 = -1.f;
                            if (idx == lane + WAVE) c1 = -1.f;
                        }
                    }
                    if (lane == 0) { ti[j] = idx; tw[j] = wt; }
                }
            }
        }
    }
}

}  // namespace

const char* bofi::attn_maps_check(const AttnMapsArgs& a) {
    if (a.B < 1 || a.H < 1) return "B >= 1 and H >= 1";
    if (a.Lq < 1 || a.Lq > 64) return "Lq in 1..64";
    if (a.Lk < 1 || a.Lk > 128) return "Lk in 1..128";
    if (a.K < 0 || a.K > 8) return "K in 0..8";
    if (a.dtype != BOFI_DT_F32 && a.dtype != BOFI_DT_BF16) return "dtype float32 or bf16";
    if (!a.q || !a.k) return "non-null q and k";
    if ((int64_t)a.ldq < (int64_t)a.H * DK || (int64_t)a.ldk < (int64_t)a.H * DK) return "row pitches of at least H * 64 elements";
    if (!a.mean && !a.heads && !a.top_idx && !a.top_w) return "at least one output buffer";
    if (!a.top_idx != !a.top_w) return "top_idx and top_w: both or neither";
    if (a.K > 0 && !a.top_idx) return "K > 0 needs top_idx and top_w";
    if (!a.mean && !a.heads && a.K == 0) return "top_idx / top_w with K = 0 leave nothing to write";
    const int64_t per_row = (int64_t)a.H * (DK + (a.Lk > WAVE ? 128 : 64)) * 4;
    if (per_row > AM_LDS_MAX) return "H * (64 + Lk) * 4 bytes of LDS per query row exceed 144 KB";
    return nullptr;
}

int bofi::launch_attn_maps(const AttnMapsArgs& a, hipStream_t st) {
    if (attn_maps_check(a)) return BOFI_ERR_ARG;
    static bool attr_set = false;
    if (!attr_set) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(attn_maps_kernel<float>), hipFuncAttributeMaxDynamicSharedMemorySize, AM_LDS_MAX) != hipSuccess ||
            hipFuncSetAttribute(reinterpret_cast<const void*>(attn_maps_kernel<bf16_t>), hipFuncAttributeMaxDynamicSharedMemorySize, AM_LDS_MAX) != hipSuccess)
            return BOFI_ERR_HIP;
        attr_set = true;
    }
    const int LKP = a.Lk > WAVE ? 128 : 64;
    const int per_row = a.H * (DK + LKP) * 4;
    // chunks of query rows per image: as many as fill the chip twice over at small B (a workgroup's time is a chain of per-row latencies: measured 26 us for all 20 rows of
    // an image in one workgroup, with three quarters of the CUs idle at 64 images), and at least what the LDS budget asks for
    int chunks = (AM_TARGET_WGS + a.B - 1) / a.B;
    chunks = chunks > a.Lq ? a.Lq : chunks;
    int TQ = (a.Lq + chunks - 1) / chunks;
    if (TQ > AM_LDS_MAX / per_row) TQ = AM_LDS_MAX / per_row;
    chunks = (a.Lq + TQ - 1) / TQ;
    const size_t smem = (size_t)TQ * per_row;
    if (a.dtype == BOFI_DT_F32) hipLaunchKernelGGL(attn_maps_kernel<float>, dim3(a.B, chunks), dim3(NT), smem, st, a, TQ, LKP);
    else hipLaunchKernelGGL(attn_maps_kernel<bf16_t>, dim3(a.B, chunks), dim3(NT), smem, st, a, TQ, LKP);
    BOFI_CHECK_LAUNCH();
    return BOFI_OK;
}

extern "C" int bofi_attn_maps(const void* q, int ldq, const void* k, int ldk, int dtype, int B, int H, int Lq, int Lk, float scale, const int* klen,
                              const int* qlen, int qlen_bias, float* mean, float* heads, int K, int* top_idx, float* top_w, void* stream) {
    bofi::AttnMapsArgs a{};
    a.q = q; a.ldq = ldq; a.k = k; a.ldk = ldk; a.dtype = dtype; a.B = B; a.H = H; a.Lq = Lq; a.Lk = Lk; a.scale = scale; a.klen = klen; a.qlen = qlen;
    a.qlen_bias = qlen_bias; a.mean = mean; a.heads = heads; a.K = K; a.top_idx = top_idx; a.top_w = top_w;
    if (const char* why = bofi::attn_maps_check(a)) return bofi::fail(BOFI_ERR_ARG, std::string("attn_maps: ") + why);
    return bofi::launch_attn_maps(a, (hipStream_t)stream);
}
