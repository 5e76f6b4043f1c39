// The constrained pick behind the vocabulary epilogue: banned ids (the reference's suppress_UNK, CaptionModel.py:151-153 / AttModel.py:333-334, and any id list) and "never the
// same word twice in a row" (its decoding_constraint, AttModel.py:325-329) on the NON-autoregressive path, where the reference applies neither: every position of the filling
// pass is picked on its own (torch.max over the vocabulary, CaptionModel.py:388-390), so the same word at neighbouring positions is that decode's characteristic artefact.
//
// x [rows, ldx] float32 (log-probs or raw logits, read only), row b * S + s = position s of image b; n_b = clamp(ntok[b] + ntok_bias, 0, S) live positions.
//   order     id a comes BEFORE id c when x[a] is NaN and x[c] is not; else, neither NaN, when x[a] > x[c]; ties -- +0.0 against -0.0 and NaN against NaN included -- go to the
//             lower id (torch.max's rule, as bofi_vocab_finalize has it)
//   eligible  not banned, and (no_repeat == 0 or s == 0 or prev < repeat_min_id or id != prev), prev = the constrained pick of position s - 1 of the image
//   pick      the first eligible id in the order: the scan along a caption is sequential, and the two best non-banned ids of a row are all it needs
// seq[b, s] = pick (s < n_b) or pad_idx; row_chosen[b, s] = x[row, pick] (s < n_b; untouched past n_b); changed[b] = #{s < n_b: pick != the id that stood in seq}.
//
// Two launches.  (One workgroup of 16 wavefronts per image that streamed, merged in LDS and scanned was built first: at 64 images its 64 workgroups streamed 22 MB in 87 us,
// five times bofi_vocab_stats' time on the whole tensor -- an image's rows waited on each other in one workgroup while three quarters of the chip idled; profiles/r17_constrained_pick.txt.)
//   candidates  one workgroup of four wavefronts per LIVE row (rows past n_b leave at once and are not read), the row cut into four column segments.  A row is only 4-byte
//               aligned (V = 9 491: no pitch is a multiple of 16 bytes): segment 0 peels to the row's first 16-byte boundary, the segments split the 16-byte loads behind
//               it -- up to ten in flight per lane, the whole segment at V = 9 491 --, the last one takes the scalar tail.  A lane keeps its best two (value, id) under the
//               order above (one compare rejects almost every element; the ban bits, staged in LDS, are looked up only for an element that would enter the pair), the 64
//               lanes merge by a shuffle butterfly under the same order, the four wavefronts' pairs meet in LDS.  The row's two candidate ids are left IN seq[row] itself
//               (the low and the high 32 bits; bit 31 of each: "the id that stood here on entry was this one") -- the scan needs no workspace.
//   scan        one wavefront per image, lane = position: each lane unpacks its row's pair, the wavefront walks the caption once (a broadcast of the previous pick per
//               step), then every lane writes its outputs; x is read again only at the picked ids.
// No atomics, no float arithmetic at all: every comparison is exact, and the result does not depend on the cut into segments.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>

#include "bofi_common.h"
#include "bofi_kernels.h"
#include "boficap_hip.h"

namespace {

using namespace bofi;

constexpr int VC_SEG = 4;                      // wavefronts per row = column segments
constexpr int VC_NT = VC_SEG * WAVE;
constexpr int VC_MAX_S = 64;
constexpr int VC_NONE = 0x7fffffff;            // "no id": behind every real id in the order (value -inf)
constexpr int VC_BAN_LDS_WORDS = 8192;         // ban tables up to 262 144 ids are staged in LDS; longer ones are read through the cache
constexpr int VC_UNROLL = 10;                  // 16-byte loads in flight per lane
constexpr int VC_SCAN_WAVES = 4;               // images per workgroup of the scan

// does (v1, i1) come before (v2, i2)?
__device__ __forceinline__ bool vc_before(float v1, int i1, float v2, int i2) {
    const bool n1 = v1 != v1, n2 = v2 != v2;
    if (n1 || n2) return n1 && (!n2 || i1 < i2);
    return v1 > v2 || (v1 == v2 && i1 < i2);
}

struct Best2 { float v1; int i1; float v2; int i2; };

// the best two of two pairs over disjoint id sets (two "no id" entries compare as equal: either is kept)
__device__ __forceinline__ Best2 vc_merge(Best2 a, Best2 b) {
    Best2 r;
    if (vc_before(b.v1, b.i1, a.v1, a.i1)) {
        r.v1 = b.v1; r.i1 = b.i1;
        if (vc_before(a.v1, a.i1, b.v2, b.i2)) { r.v2 = a.v1; r.i2 = a.i1; } else { r.v2 = b.v2; r.i2 = b.i2; }
    } else {
        r.v1 = a.v1; r.i1 = a.i1;
        if (vc_before(b.v1, b.i1, a.v2, a.i2)) { r.v2 = b.v1; r.i2 = b.i1; } else { r.v2 = a.v2; r.i2 = a.i2; }
    }
    return r;
}

template <bool BAN>
__device__ __forceinline__ void vc_take(Best2& m, float v, int id, const uint32_t* ban) {
    if (v < m.v2) return;                                      // (both numbers and v below: behind the second best.  A NaN on either side is false: the full order decides)
    if (!vc_before(v, id, m.v2, m.i2)) return;
    if (BAN && ((ban[id >> 5] >> (id & 31)) & 1u)) return;
    if (vc_before(v, id, m.v1, m.i1)) { m.v2 = m.v1; m.i2 = m.i1; m.v1 = v; m.i1 = id; }
    else { m.v2 = v; m.i2 = id; }
}

struct VcArgs {
    const float* x; int ldx, V, S;
    const int* ntok; int ntok_bias, pad_idx;
    const uint32_t* ban; int ban_words, ban_lds;
    int no_repeat, repeat_min_id;
    int64_t* seq; float* row_chosen; int* changed;
};

__device__ __forceinline__ int vc_live(const VcArgs& a, int b) {
    const int n = a.ntok ? a.ntok[b] + a.ntok_bias : a.S;
    return n < 0 ? 0 : (n > a.S ? a.S : n);
}

// grid = rows: the two best unbanned ids of a live row into seq[row] (packed), pad_idx into a row past n_b
template <bool BAN>
__global__ void __launch_bounds__(VC_NT) vocab_candidates_kernel(VcArgs a) {
    extern __shared__ uint32_t vc_ban[];                       // [ban_words] when the table is staged
    __shared__ Best2 cand[VC_SEG];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid % WAVE, seg = tid / WAVE;
    const int V = a.V, b = row / a.S, s = row - b * a.S;
    if (s >= vc_live(a, b)) {                                   // (the whole workgroup: nothing below waits for it)
        if (tid == 0) a.seq[row] = (int64_t)a.pad_idx;
        return;
    }
    const uint32_t* ban = a.ban;
    if (BAN && a.ban_lds) {
        for (int i = tid; i < a.ban_words; i += VC_NT) vc_ban[i] = a.ban[i];
        ban = vc_ban;
        __syncthreads();
    }
    const float* const p = a.x + (size_t)row * (size_t)a.ldx;
    int peel = (4 - (int)(((uintptr_t)p >> 2) & 3)) & 3;       // elements in front of the row's first 16-byte boundary
    peel = peel > V ? V : peel;
    const int nv = (V - peel) / 4, tail0 = peel + 4 * nv;      // 16-byte groups behind it; the first element of the scalar tail
    const int g0 = (int)((int64_t)seg * nv / VC_SEG), g1 = (int)((int64_t)(seg + 1) * nv / VC_SEG);
    Best2 m{-INFINITY, VC_NONE, -INFINITY, VC_NONE};
    if (seg == 0 && lane < peel) vc_take<BAN>(m, p[lane], lane, ban);
    if (seg == VC_SEG - 1 && tail0 + lane < V) vc_take<BAN>(m, p[tail0 + lane], tail0 + lane, ban);
    const float4* const p4 = reinterpret_cast<const float4*>(p + peel);
    for (int base = g0; base < g1; base += WAVE * VC_UNROLL) {
        float4 r[VC_UNROLL];
#pragma unroll
        for (int j = 0; j < VC_UNROLL; ++j) {
            const int g = base + j * WAVE + lane;
            r[j] = g < g1 ? p4[g] : float4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int j = 0; j < VC_UNROLL; ++j) {
            const int g = base + j * WAVE + lane;
            if (g < g1) {
                const int id = peel + 4 * g;
                vc_take<BAN>(m, r[j].x, id, ban); vc_take<BAN>(m, r[j].y, id + 1, ban);
                vc_take<BAN>(m, r[j].z, id + 2, ban); vc_take<BAN>(m, r[j].w, id + 3, ban);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {                          // butterfly: the lanes hold disjoint ids, so both partners of a step arrive at the same pair
        Best2 t;
        t.v1 = __shfl_xor(m.v1, o, WAVE); t.i1 = __shfl_xor(m.i1, o, WAVE);
        t.v2 = __shfl_xor(m.v2, o, WAVE); t.i2 = __shfl_xor(m.i2, o, WAVE);
        m = vc_merge(m, t);
    }
    if (lane == 0) cand[seg] = m;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int k = 1; k < VC_SEG; ++k) m = vc_merge(m, cand[k]);
        const int64_t old = a.seq[row];
        const uint32_t w1 = (uint32_t)m.i1 | (old == (int64_t)m.i1 ? 0x80000000u : 0u), w2 = (uint32_t)m.i2 | (old == (int64_t)m.i2 ? 0x80000000u : 0u);
        a.seq[row] = (int64_t)(((uint64_t)w2 << 32) | w1);
    }
}

// grid = ceil(B / 4) workgroups of four wavefronts: wavefront = image, lane = position
__global__ void __launch_bounds__(VC_SCAN_WAVES * WAVE) vocab_scan_kernel(VcArgs a, int B) {
    const int lane = threadIdx.x % WAVE, b = blockIdx.x * VC_SCAN_WAVES + threadIdx.x / WAVE;
    if (b >= B) return;                                         // (whole wavefronts leave)
    const int S = a.S, n = vc_live(a, b);
    const bool live = lane < n;
    const size_t row = (size_t)b * S + lane;
    uint32_t w1 = VC_NONE, w2 = VC_NONE;
    if (live) {
        const uint64_t w = (uint64_t)a.seq[row];
        w1 = (uint32_t)w; w2 = (uint32_t)(w >> 32);
    }
    const int i1 = (int)(w1 & 0x7fffffffu), i2 = (int)(w2 & 0x7fffffffu);
    int pick = i1;
    if (a.no_repeat) {
        for (int s = 1; s < n; ++s) {                           // (n is the same in every lane: the broadcasts see the whole wavefront)
            const int prev = __shfl(pick, s - 1, WAVE);
            if (lane == s && prev >= a.repeat_min_id && i1 == prev) pick = i2;
        }
    }
    bool was = ((pick != i1 ? w2 : w1) & 0x80000000u) != 0;     // the id that stood here on entry was the pick
    float v = -INFINITY;
    if (live) {
        if (pick == VC_NONE) { pick = a.pad_idx; was = false; } // (fewer than two unbanned ids: the caller's duty -- never an id outside the vocabulary)
        else v = a.x[row * (size_t)a.ldx + pick];
        a.seq[row] = (int64_t)pick;
        if (a.row_chosen) a.row_chosen[row] = v;
    }
    const unsigned long long ch = __ballot(live && !was);
    if (lane == 0 && a.changed) a.changed[b] = __popcll(ch);
}

}  // namespace

int bofi::launch_vocab_constrain(const float* x, int ldx, int rows, int V, int S, const int* ntok, int ntok_bias, int pad_idx, const uint32_t* ban_bits,
                                 int no_repeat, int repeat_min_id, int64_t* seq, float* row_chosen, int* changed, hipStream_t st) {
    if (vocab_constrain_check(x, ldx, rows, V, S, no_repeat, repeat_min_id, seq)) return BOFI_ERR_ARG;
    if (rows == 0) return BOFI_OK;
    VcArgs a{};
    a.x = x; a.ldx = ldx; a.V = V; a.S = S; a.ntok = ntok; a.ntok_bias = ntok_bias; a.pad_idx = pad_idx; a.ban = ban_bits; a.ban_words = (V + 31) / 32;
    a.ban_lds = a.ban_words <= VC_BAN_LDS_WORDS; a.no_repeat = no_repeat; a.repeat_min_id = repeat_min_id; a.seq = seq; a.row_chosen = row_chosen; a.changed = changed;
    const int B = rows / S;
    if (ban_bits) hipLaunchKernelGGL(vocab_candidates_kernel<true>, dim3(rows), dim3(VC_NT), a.ban_lds ? (size_t)a.ban_words * 4 : 0, st, a);
    else hipLaunchKernelGGL(vocab_candidates_kernel<false>, dim3(rows), dim3(VC_NT), 0, st, a);
    BOFI_CHECK_LAUNCH();
    hipLaunchKernelGGL(vocab_scan_kernel, dim3((B + VC_SCAN_WAVES - 1) / VC_SCAN_WAVES), dim3(VC_SCAN_WAVES * WAVE), 0, st, a, B);
    BOFI_CHECK_LAUNCH();
    return BOFI_OK;
}

const char* bofi::vocab_constrain_check(const float* x, int ldx, int rows, int V, int S, int no_repeat, int repeat_min_id, const int64_t* seq) {
    if (!x || !seq) return "non-null x and seq";
    if (S < 1 || S > VC_MAX_S) return "S in 1..64";
    if (rows < 0 || rows % S != 0) return "rows a multiple of S (>= 0)";
    if (V < 2) return "V >= 2";
    if (ldx < V) return "a row pitch of at least V";
    if (no_repeat != 0 && no_repeat != 1) return "no_repeat 0 or 1";
    if (repeat_min_id < 0) return "repeat_min_id >= 0";
    return nullptr;
}

extern "C" int bofi_vocab_constrain(const float* x, int ldx, int rows, int V, int S, const int* ntok, int ntok_bias, int pad_idx, const uint32_t* ban_bits,
                                    int no_repeat, int repeat_min_id, int64_t* seq, float* row_chosen, int* changed, void* stream) {
    if (const char* why = bofi::vocab_constrain_check(x, ldx, rows, V, S, no_repeat, repeat_min_id, seq)) return bofi::fail(BOFI_ERR_ARG, std::string("vocab_constrain: ") + why);
    return bofi::launch_vocab_constrain(x, ldx, rows, V, S, ntok, ntok_bias, pad_idx, ban_bits, no_repeat, repeat_min_id, seq, row_chosen, changed, (hipStream_t)stream);
}
