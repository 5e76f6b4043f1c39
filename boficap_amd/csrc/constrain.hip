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

#include <cmath>
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

// a lane's best two (value, id) under the order.  empty() and take() are what vk_stream asks of a lane's accumulator (Best<N> below is the other one)
struct Best2 {
    float v1; int i1; float v2; int i2;
    static __device__ __forceinline__ Best2 empty() { return Best2{-INFINITY, VC_NONE, -INFINITY, VC_NONE}; }
    template <bool BAN, bool FLOOR>
    __device__ __forceinline__ void take(float v, int id, const uint32_t* ban, uint64_t /*floor*/) {
        static_assert(!FLOOR, "the pair has no floor");
        if (v < v2) return;                                    // (both numbers and v below: behind the second best.  A NaN on either side is false: the full order decides)
        if (!vc_before(v, id, v2, i2)) return;
        if (BAN && ((ban[id >> 5] >> (id & 31)) & 1u)) return;
        if (vc_before(v, id, v1, i1)) { v2 = v1; i2 = i1; v1 = v; i1 = id; }
        else { v2 = v; i2 = id; }
    }
};

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

struct VcArgs {
    const float* x; int ldx, V, S;
    const int* ntok; int ntok_bias, pad_idx;
    const uint32_t* ban; int ban_words, ban_lds;
    int no_repeat, repeat_min_id;
    int64_t* seq; float* row_chosen; int* changed;
};

__device__ __forceinline__ int vc_live(const VcArgs& a, int b) { return live_count(a.ntok, a.ntok_bias, b, a.S); }

// THE ROW STREAM, for both candidate kernels and the fallback re-read (vk_row_behind): one wavefront over column segment `seg` of `nseg` of the row at p -- peel to the row's
// first 16-byte boundary (segment 0), the segments split the 16-byte loads behind it, VC_UNROLL of them in flight per lane, scalar tail (the last segment).  M is the lane's
// accumulator: Best2, or Best<VP_L> (which alone knows a `floor`).
template <typename M, bool BAN, bool FLOOR>
__device__ __forceinline__ M vk_stream(const float* p, int V, int seg, int nseg, int lane, const uint32_t* ban, uint64_t floor) {
    int peel = (4 - (int)(((uintptr_t)p >> 2) & 3)) & 3;       // elements in front of the row's first 16-byte boundary
    peel = peel > V ? V : peel;
    const int nv = (V - peel) / 4, tail0 = peel + 4 * nv;      // 16-byte groups behind it; the first element of the scalar tail
    const int g0 = (int)((int64_t)seg * nv / nseg), g1 = (int)((int64_t)(seg + 1) * nv / nseg);
    M m = M::empty();
    if (seg == 0 && lane < peel) m.template take<BAN, FLOOR>(p[lane], lane, ban, floor);
    if (seg == nseg - 1 && tail0 + lane < V) m.template take<BAN, FLOOR>(p[tail0 + lane], tail0 + lane, ban, floor);
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
                m.template take<BAN, FLOOR>(r[j].x, id, ban, floor); m.template take<BAN, FLOOR>(r[j].y, id + 1, ban, floor);
                m.template take<BAN, FLOOR>(r[j].z, id + 2, ban, floor); m.template take<BAN, FLOOR>(r[j].w, id + 3, ban, floor);
            }
        }
    }
    return m;
}

// The entry of both candidate kernels (grid = rows, VC_NT threads): a row past n_b gets pad_idx into seq (where there is a seq: bofi_vocab_nbest has none, it pads its own
// outputs) and the WHOLE workgroup leaves -- false; nothing waits for it.  Else `ban` is the table to look up: staged in dynamic LDS (and one barrier) when it fits.
template <bool BAN>
__device__ __forceinline__ bool vc_enter(const VcArgs& a, int row, int tid, const uint32_t*& ban) {
    extern __shared__ uint32_t vc_ban[];                       // [ban_words] when the table is staged
    const int b = row / a.S, s = row - b * a.S;
    if (s >= vc_live(a, b)) {
        if (tid == 0 && a.seq) a.seq[row] = (int64_t)a.pad_idx;
        return false;
    }
    ban = a.ban;
    if (BAN && a.ban_lds) {
        for (int i = tid; i < a.ban_words; i += VC_NT) vc_ban[i] = a.ban[i];
        ban = vc_ban;
        __syncthreads();
    }
    return true;
}

// grid = rows: the two best unbanned ids of a live row into seq[row] (packed), pad_idx into a row past n_b
template <bool BAN>
__global__ void __launch_bounds__(VC_NT) vocab_candidates_kernel(VcArgs a) {
    __shared__ Best2 cand[VC_SEG];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid % WAVE, seg = tid / WAVE;
    const uint32_t* ban;
    if (!vc_enter<BAN>(a, row, tid, ban)) return;
    Best2 m = vk_stream<Best2, BAN, false>(a.x + (size_t)row * (size_t)a.ldx, a.V, seg, VC_SEG, lane, ban, 0ull);
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

// ---- the K-candidate form (bofi_vocab_pick): the rule above plus block_trigrams -- an id that followed the bigram (p[s-2], p[s-1]) earlier in the image's picks, all
// three ids words, is not eligible at s; include/boficap_hip.h, bofi_vocab_pick, states the rule (the reference's table, AttModel.py:362-388, as a HARD block).
//   key         the order as ONE unsigned 64-bit compare, integer operations only: the high word is the float's bits made monotone (NaN above every number, -0.0 as
//               +0.0), the low word 2 (0x7fffffff - id) -- so a larger key comes first in the order --, bit 0 a mark (below); 0 is "no id".  A lane's sorted insert is
//               then a chain of compare-and-swaps of a few instructions each (with the order's float compares and their NaN cases the chain of a K-list cost several
//               times the pair's: DESIGN.md section 10).
//   candidates  as above, but a lane keeps its best VP_L = 4 keys (a sorted list in registers, one compare against its last entry rejects an element) and the ROW keeps
//               VP_K = 8: butterfly and LDS merge are bitonic merges of sorted 8-lists.  A lane's 4th entry carries the mark "this lane may hold more": the merged
//               list is the row's true order up to and including its first marked entry, and what stands behind that entry is written as VP_CUT ("not known from
//               here").  With ~37 elements per lane a lane holds four of a row's best eight in a few of 10^6 rows.  The row's ids go to an int32 workspace
//               [rows, VP_K]; seq[row] keeps the id that stood there.
//   scan        one wavefront per image, lane = position.  At step s the lanes j < s whose (p[j-2], p[j-1]) equal the current bigram form the excluded set (a ballot);
//               the candidates of lane s are tried in order against it.  All of them excluded, or VP_CUT reached: the wavefront streams that one row again (the
//               candidates launch's own loop) for the next VP_L ids BEHIND the last one tried -- exact, as a row's best four are among its lanes' best four --,
//               until one is eligible or the row is exhausted: the result is the rule's for every input; only the cost differs, and only for such rows.
constexpr int VP_K = 8;                        // candidates per row (DESIGN.md section 10 has the choice)
constexpr int VP_L = 4;                        // ... and per lane
constexpr int VP_CUT = 0x7ffffffe;             // in the workspace: the row's order is not known from this entry on
static_assert(VP_K == 2 * VP_L && (VP_L & (VP_L - 1)) == 0, "the merges are bitonic");

__device__ __forceinline__ uint64_t vk_key(float v, int id) {
    uint32_t u = __float_as_uint(v);
    if (u == 0x80000000u) u = 0u;                              // -0.0 ties with +0.0
    uint32_t h = u ^ ((uint32_t)((int32_t)u >> 31) | 0x80000000u);      // ascending with the value: -inf -> 0x007fffff, +inf -> 0xff800000
    if ((u & 0x7fffffffu) > 0x7f800000u) h = 0xffffffffu;      // every NaN alike, in front of every number
    return ((uint64_t)h << 32) | ((0x7fffffffu - (uint32_t)id) << 1);      // ties to the lower id
}
__device__ __forceinline__ int vk_id(uint64_t key) { return key ? (int)(0x7fffffffu - ((uint32_t)key >> 1)) : VC_NONE; }

// order entries a and c of a list: afterwards a is not behind c
__device__ __forceinline__ void vk_order(uint64_t& a, uint64_t& c) {
    const uint64_t hi = a > c ? a : c, lo = a > c ? c : a;
    a = hi; c = lo;
}

// a sorted list of keys, descending; 0 = no id.  As a lane's accumulator for vk_stream (as Best2): an element strictly behind `floor` (FLOOR) enters the list when it
// is in front of the list's last entry and not banned
template <int N>
struct Best {
    uint64_t k[N];
    static __device__ __forceinline__ Best empty() {
        Best m;
#pragma unroll
        for (int i = 0; i < N; ++i) m.k[i] = 0ull;
        return m;
    }
    template <bool BAN, bool FLOOR>
    __device__ __forceinline__ void take(float v, int id, const uint32_t* ban, uint64_t floor) {
        const uint64_t key = vk_key(v, id);
        if (key <= k[N - 1]) return;
        if (FLOOR && key >= floor) return;
        if (BAN && ((ban[id >> 5] >> (id & 31)) & 1u)) return;
        k[N - 1] = key;
#pragma unroll
        for (int i = N - 1; i > 0; --i) vk_order(k[i - 1], k[i]);
    }
};

// the best N of two sorted lists over disjoint id sets: a[k] against b[N-1-k] leaves the best N as a bitonic sequence, log2 N half-cleaners sort it
template <int N>
__device__ __forceinline__ Best<N> vk_merge(const Best<N>& a, const Best<N>& b) {
    Best<N> r;
#pragma unroll
    for (int k = 0; k < N; ++k) r.k[k] = a.k[k] > b.k[N - 1 - k] ? a.k[k] : b.k[N - 1 - k];
#pragma unroll
    for (int h = N / 2; h > 0; h >>= 1)
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (!(k & h)) vk_order(r.k[k], r.k[k + h]);
    return r;
}

template <int N>
__device__ __forceinline__ Best<N> vk_wave_merge(Best<N> m) {   // butterfly: every lane ends with the wavefront's list
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        Best<N> t;
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)m.k[k], o, WAVE), hi = (uint32_t)__shfl_xor((int)(uint32_t)(m.k[k] >> 32), o, WAVE);
            t.k[k] = ((uint64_t)hi << 32) | lo;
        }
        m = vk_merge<N>(m, t);
    }
    return m;
}

// grid = rows: the best unbanned ids of a live row into work[row][VP_K] (VP_CUT from where the order is not known); pad_idx into seq of a row past n_b
template <bool BAN>
__global__ void __launch_bounds__(VC_NT) vocab_candidates_k_kernel(VcArgs a, int* __restrict__ work) {
    __shared__ Best<VP_K> cand[VC_SEG];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid % WAVE, seg = tid / WAVE;
    const uint32_t* ban;
    if (!vc_enter<BAN>(a, row, tid, ban)) return;
    const Best<VP_L> own = vk_stream<Best<VP_L>, BAN, false>(a.x + (size_t)row * (size_t)a.ldx, a.V, seg, VC_SEG, lane, ban, 0ull);
    Best<VP_K> m;
#pragma unroll
    for (int k = 0; k < VP_K; ++k) m.k[k] = k < VP_L ? own.k[k] : 0ull;
    if (m.k[VP_L - 1]) m.k[VP_L - 1] |= 1ull;                   // a full lane list: the lane may hold more behind it
    m = vk_wave_merge<VP_K>(m);
    if (lane == 0) cand[seg] = m;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int k = 1; k < VC_SEG; ++k) m = vk_merge<VP_K>(m, cand[k]);
        bool cut = false;
#pragma unroll
        for (int k = 0; k < VP_K; ++k) {
            work[(size_t)row * VP_K + k] = cut ? VP_CUT : vk_id(m.k[k]);
            cut = cut || (m.k[k] & 1ull);
        }
    }
}

// the wavefront's next VP_L unbanned ids of one row strictly BEHIND `floor` in the order (the scan's fallback; the ban table through the cache), the same in every lane
__device__ __forceinline__ Best<VP_L> vk_row_behind(const float* p, int V, uint64_t floor, const uint32_t* ban, int lane) {
    return vk_wave_merge<VP_L>(ban ? vk_stream<Best<VP_L>, true, true>(p, V, 0, 1, lane, ban, floor) : vk_stream<Best<VP_L>, false, true>(p, V, 0, 1, lane, ban, floor));
}

// grid = ceil(B / 4) workgroups of four wavefronts: wavefront = image, lane = position
__global__ void __launch_bounds__(VC_SCAN_WAVES * WAVE) vocab_scan_k_kernel(VcArgs a, const int* __restrict__ work, int trigrams, int B) {
    const int lane = threadIdx.x % WAVE, b = __builtin_amdgcn_readfirstlane(blockIdx.x * VC_SCAN_WAVES + threadIdx.x / WAVE);
    if (b >= B) return;                                         // (whole wavefronts leave)
    const int S = a.S, n = __builtin_amdgcn_readfirstlane(vc_live(a, b)), lo = a.repeat_min_id;
    const bool live = lane < n;
    const size_t row = (size_t)b * S + lane;
    int c[VP_K];
#pragma unroll
    for (int k = 0; k < VP_K; ++k) c[k] = live ? work[row * VP_K + k] : VC_NONE;
    int pick = VC_NONE, pm1 = -1, pm2 = -1;                     // this lane's pick and those of the two lanes before it, as they are made
    int p1 = -1, p2 = -1;                                       // the picks of positions s - 1 and s - 2 (wave-uniform)
    for (int s = 0; s < n; ++s) {
        const int rep = (a.no_repeat && s > 0 && p1 >= lo) ? p1 : -1;
        const bool tri = trigrams && s >= 3 && p1 >= lo && p2 >= lo;
        const bool ex = tri && lane >= 2 && lane < s && pm2 == p2 && pm1 == p1 && pick >= lo;      // this lane's pick is trigram-blocked at s
        const bool any = __ballot(ex) != 0ull;
        int q = VC_NONE, tried = VC_NONE;                       // the pick; the last candidate found ineligible
        bool found = false, cut = false;
#pragma unroll
        for (int k = 0; k < VP_K; ++k) {
            if (!found && !cut) {
                const int ck = __builtin_amdgcn_readlane(c[k], s);
                if (ck == VC_NONE) found = true;                // (the row has no further unbanned id: pad_idx below)
                else if (ck == VP_CUT) cut = true;
                else if (ck != rep && !(any && __ballot(ex && pick == ck) != 0ull)) { found = true; q = ck; }
                else tried = ck;
            }
        }
        if (!found) {                                           // every known candidate is excluded: the row again, behind the last one tried (the first entry is never VP_CUT)
            const float* const p = a.x + ((size_t)b * S + s) * (size_t)a.ldx;
            uint64_t floor = vk_key(p[tried], tried);
            while (!found) {
                const Best<VP_L> m = vk_row_behind(p, a.V, floor, a.ban, lane);
#pragma unroll
                for (int k = 0; k < VP_L; ++k) {
                    if (!found) {
                        const int ck = __builtin_amdgcn_readfirstlane(vk_id(m.k[k]));
                        if (ck == VC_NONE) found = true;
                        else if (ck != rep && !(any && __ballot(ex && pick == ck) != 0ull)) { found = true; q = ck; }
                    }
                }
                floor = m.k[VP_L - 1];
            }
        }
        if (lane == s) pick = q;
        if (lane == s + 1) pm1 = q;
        if (lane == s + 2) pm2 = q;
        p2 = p1; p1 = q;
    }
    bool was = false;
    if (live) {
        const int64_t old = a.seq[row];
        float v = -INFINITY;
        if (pick == VC_NONE) pick = a.pad_idx;                  // (fewer eligible ids than the rule needs: the caller's duty -- never an id outside the vocabulary)
        else { v = a.x[row * (size_t)a.ldx + pick]; was = old == (int64_t)pick; }
        a.seq[row] = (int64_t)pick;
        if (a.row_chosen) a.row_chosen[row] = v;
    }
    const unsigned long long ch = __ballot(live && !was);
    if (lane == 0 && a.changed) a.changed[b] = __popcll(ch);
}

// ---- the N-best list (bofi_vocab_nbest): the N most probable captions of a pass that scores every position on its own.  A caption's log-prob is a sum of per-position
// terms, so the N best use only each row's N best ids, and a width-N merge over the positions finds them exactly; include/boficap_hip.h, bofi_vocab_nbest, states the rule
// (candidates, the float64 recurrence, the tie order), tests/test_nbest.py restates it in numpy and holds it to a brute force over every caption.
//   candidates  the K-candidate launch above, unchanged (seq = NULL: it writes the workspace only)
//   merge       one wavefront per image, four images per workgroup.  Lane = position first: the row's ids go from the workspace to LDS; a row whose order is cut
//               (VP_CUT) inside its first N entries is streamed again by the whole wavefront (vk_row_behind, as the scan above) -- the result is the rule's for every
//               input.  Then the n_b * N values x[p, c[p][r]]: scattered 4-byte loads, rows need no alignment.  Then lane = pair, lane = i * N + r (N <= 8: the 64 lanes
//               hold every pair of a step): the lane forms its total T_i + (double)x, the totals meet in LDS, every lane counts the valid pairs in front of it (a larger
//               total, or the same total and a lower lane) -- its rank --, the lanes of rank < N write (total, lane) as the new list.  The byte back-pointers [S][N], the
//               ids and the values stay in LDS; lane j walks caption j back, the wavefront writes seq_n[b] as one contiguous block.
// The loop over the positions is uniform over the workgroup (a wavefront past its n_b only meets the barriers).  No atomics; the only float arithmetic is the one float64
// add per pair: no product, so nothing contracts.
constexpr int NB_MAX = BOFI_NBEST_MAX;         // N at most
constexpr int NB_IPW = 4;                      // images (wavefronts) per workgroup
constexpr int NB_CHUNK = 16;                   // totals read from LDS at a time by the ranking loop
static_assert(WAVE % NB_CHUNK == 0, "the ranking loop reads whole chunks of the wavefront's totals");
static_assert(NB_MAX == VP_K && NB_MAX * NB_MAX == WAVE, "the candidates launch leaves NB_MAX ids per row; the lanes of a wavefront hold every pair of a step");

struct NbArgs {
    const float* x; int ldx, V, S, B;
    const int* ntok; int ntok_bias, pad_idx;
    const uint32_t* ban;
    int N;
    int64_t* seq_n; double* total; int* count;
};

// THE LIST KERNELS' FRONT END (vocab_nbest_kernel and vocab_nbest_norepeat_kernel; cid and xv have a stride of VP_K entries per row in both).  None of these helpers holds
// a barrier: the kernels keep theirs between the steps.
// one wavefront, lane = position: the first `want` workspace ids of the image's rows into cid (VC_NONE behind them and where the row has no such id).  Returns cutk, the
// first entry within `want` from which the row's order is not known (-1: none)
__device__ __forceinline__ int nb_ids(const int* __restrict__ work, size_t row0, int n, int want, int V, int* cid, int lane) {
    int cutk = -1;
    if (lane < n) {
#pragma unroll
        for (int k = 0; k < VP_K; ++k) {
            int c = k < want ? work[(row0 + lane) * VP_K + k] : VC_NONE;
            if (c == VP_CUT) { if (cutk < 0) cutk = k; }
            else if ((unsigned)c >= (unsigned)V) c = VC_NONE;  // (VC_NONE itself; never an index outside the row)
            cid[lane * VP_K + k] = cutk >= 0 ? VC_NONE : c;
        }
    }
    return cutk;
}
// ... then (behind a barrier) the rows with a cut order, one at a time: the whole wavefront streams the row again for the ids behind the last one known
__device__ __forceinline__ void nb_cut_rows(const NbArgs& a, size_t row0, int want, int cutk, int* cid, int lane) {
    for (unsigned long long cuts = __ballot(cutk >= 0); cuts; cuts &= cuts - 1) {
        const int s = __builtin_amdgcn_readfirstlane(__ffsll((long long)cuts) - 1);
        int k0 = __builtin_amdgcn_readlane(cutk, s);            // (>= 1: the first entry is never VP_CUT)
        const float* const p = a.x + (row0 + s) * (size_t)a.ldx;
        const int last = cid[s * VP_K + k0 - 1];
        if (last == VC_NONE) continue;                          // (cannot be: a cut stands behind a real id)
        uint64_t floor = vk_key(p[last], last);
        while (k0 < want) {
            const Best<VP_L> m = vk_row_behind(p, a.V, floor, a.ban, lane);
#pragma unroll
            for (int k = 0; k < VP_L; ++k)
                if (lane == 0 && k0 + k < want) cid[s * VP_K + k0 + k] = vk_id(m.k[k]);
            if (!m.k[VP_L - 1]) break;                          // the row is exhausted
            floor = m.k[VP_L - 1];
            k0 += VP_L;
        }
    }
}
// thread t of nt over the (position, candidate) pairs: the values x[p, c[p][r]] -- scattered 4-byte loads, rows need no alignment; NaN where there is no id
__device__ __forceinline__ void nb_values(const NbArgs& a, size_t row0, int n, const int* cid, float* xv, int t, int nt) {
    for (int i = t; i < n * VP_K; i += nt) {
        const int c = cid[i];
        xv[i] = c != VC_NONE ? a.x[(row0 + i / VP_K) * (size_t)a.ldx + (size_t)c] : NAN;
    }
}
// a live row whose first id has no finite value: the image is degenerate (a whole wavefront asks)
__device__ __forceinline__ bool nb_degen(const float* xv, int n, int lane) { return __ballot(lane < n && !f32_finite(xv[lane * VP_K])) != 0ull; }

// the rank of `mine`, the total in slot `lane`, among totals[0 .. upto): the entries in front of it -- a larger total, or the same total in a lower slot.  upto <= WAVE,
// totals holds WAVE entries and NB_CHUNK divides WAVE: a chunk never leaves the array, and an entry past upto that is read is -inf, in front of nothing
__device__ __forceinline__ int nb_rank(const double* totals, int upto, double mine, int lane) {
    int rank = 0;
    for (int j0 = 0; j0 < upto; j0 += NB_CHUNK) {
        double t[NB_CHUNK];
#pragma unroll
        for (int j = 0; j < NB_CHUNK; ++j) t[j] = totals[j0 + j];      // a chunk's LDS reads in flight together (one by one, a step was 64 dependent round trips)
#pragma unroll
        for (int j = 0; j < NB_CHUNK; ++j)      // (no && / ||: as branches they cost four times the compares)
            rank += (int)(t[j] > mine) | ((int)(t[j] == mine) & (int)(j0 + j < lane));
    }
    return rank;
}

// thread t of nt: the image's captions out [N][S] (LDS) into seq_n[b] as one contiguous block
__device__ __forceinline__ void nb_write_captions(const NbArgs& a, int b, const int* out, int t, int nt) {
    for (int i = t; i < a.N * a.S; i += nt) a.seq_n[(size_t)b * a.N * a.S + i] = (int64_t)out[i];
}

__global__ void __launch_bounds__(NB_IPW * WAVE) vocab_nbest_kernel(NbArgs a, const int* __restrict__ work) {
    __shared__ double tt_[NB_IPW][WAVE];                        // the totals of a step's pairs
    __shared__ double T_[NB_IPW][NB_MAX];                       // the list's totals
    __shared__ int cid_[NB_IPW][VC_MAX_S * NB_MAX];             // c[p][r]; VC_NONE: the row has no such id
    __shared__ float xv_[NB_IPW][VC_MAX_S * NB_MAX];            // x[p, c[p][r]]; NaN where there is no id
    __shared__ int out_[NB_IPW][NB_MAX * VC_MAX_S];             // the captions, [N][S]
    __shared__ uint8_t bp_[NB_IPW][VC_MAX_S * NB_MAX];          // [p][j]: the pair (lane) that entry j of L_{p+1} came from
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE, b = __builtin_amdgcn_readfirstlane(blockIdx.x * NB_IPW + wave);
    const bool on = b < a.B;                                    // (a wavefront past B stays for the barriers and touches no global memory)
    const int S = a.S, N = a.N, V = a.V;
    double* const tt = tt_[wave];
    double* const T = T_[wave];
    int* const cid = cid_[wave];
    float* const xv = xv_[wave];
    int* const out = out_[wave];
    uint8_t* const bp = bp_[wave];
    const int n = __builtin_amdgcn_readfirstlane(on ? live_count(a.ntok, a.ntok_bias, b, S) : 0);
    const size_t row0 = (size_t)(on ? b : 0) * S;
    const int cutk = nb_ids(work, row0, n, N, V, cid, lane);   // lane = position
    __syncthreads();
    nb_cut_rows(a, row0, N, cutk, cid, lane);
    __syncthreads();
    nb_values(a, row0, n, cid, xv, lane, WAVE);                 // lane over the (position, candidate) pairs
    if (lane < NB_MAX) T[lane] = 0.0;                           // L_0 = [(0.0, empty)]
    __syncthreads();
    const bool degen = nb_degen(xv, n, lane);
    // the merge, lane = pair
    const int pi = lane / N, pr = lane - pi * N;
    int cnt = 1;
    bool valid = false;
    double mine = 0.0;
    for (int p = 0; p < S; ++p) {
        const bool step = p < n && !degen;                      // (the same in every lane of the wavefront)
        if (step) {
            const float v = pi < cnt ? xv[p * NB_MAX + pr] : NAN;      // (pi < cnt <= N, so pr < N <= NB_MAX)
            valid = pi < cnt && f32_finite(v);
            mine = valid ? T[pi] + (double)v : -(double)INFINITY;      // (a pair that is not valid: in front of no valid pair, whose totals are finite)
            tt[lane] = mine;
        }
        __syncthreads();
        if (step) {
            const unsigned long long vm = __ballot(valid);
            const int rank = nb_rank(tt, cnt * N, mine, lane);      // (cnt * N <= WAVE)
            if (valid && rank < N) { T[rank] = mine; bp[p * NB_MAX + rank] = (uint8_t)lane; }
            const int nv = __popcll(vm);
            cnt = nv < N ? nv : N;
        }
        __syncthreads();
    }
    if (degen) cnt = 1;
    // lane j < N: caption j into LDS, walked back along the pairs
    if (on && lane < N) {
        int e = lane;
        for (int p = S - 1; p >= 0; --p) {
            int id = a.pad_idx;
            if (p < n && lane < cnt) {
                if (degen) { const int c = cid[p * NB_MAX]; id = c != VC_NONE ? c : a.pad_idx; }
                else {
                    const int pair = bp[p * NB_MAX + e];
                    e = pair / N;
                    id = cid[p * NB_MAX + pair - e * N];
                }
            }
            out[lane * S + p] = id;
        }
        a.total[(size_t)b * N + lane] = lane < cnt ? (degen ? (double)NAN : T[lane]) : -(double)INFINITY;
    }
    if (on && lane == 0) a.count[b] = cnt;
    __syncthreads();
    if (!on) return;
    nb_write_captions(a, b, out, lane, WAVE);
}

// ---- the N-best list under "no adjacent repeated word" (bofi_vocab_nbest_norepeat): the rule couples neighbours, so a width-N list no longer serves; the N best VALID
// captions come from a list-Viterbi over (position, candidate) states -- per candidate r of row p the N best prefixes that end in it.  K = N + 2 candidates per row suffice
// (at most two of the ids in front of a caption's id are excluded by its neighbours); include/boficap_hip.h, bofi_vocab_nbest_norepeat, states the rule,
// tests/test_nbest_no_repeat.py restates it in numpy and holds it to a brute force over every valid caption.
//   candidates  the K-candidate launch above, unchanged (seq = NULL), as for bofi_vocab_nbest
//   lists       one workgroup of NR_W = 8 wavefronts per image, wavefront = state r of the current row.  Front part as vocab_nbest_kernel (wavefront 0: ids to LDS, a row whose
//               order is cut inside its first K entries streamed again; then all threads: the scattered value loads).  A state's list has a stride of NR_W entries
//               (A[r * 8 + j], -inf where there is no entry), so lane = r' * 8 + j holds pair (r', j) -- lane order is the rule's (r', j) order, the index arithmetic is
//               shifts and the ranking loop's bounds are compile-time (the lanes j >= N hold -inf and are in front of nothing).  A step: every lane forms the totals
//               A_{p-1}[k] + (double)x of ALL pairs of its state itself -- the addend is the state's, wave-uniform, so the sums are the same bits in every lane and the
//               pairs need no LDS array of their own -- and counts those in front of its own (its rank); the predecessor state with the same word is skipped whole.  Lanes
//               of rank < N write (total, byte back-pointer) into A_p, double-buffered by parity: A_{p-1} is read while A_p is written, ONE barrier per step.
//   result      wavefront 0 ranks the 64 slots of A_{n_b-1} (lane = r * 8 + j: the rule's order again), lane j < count walks caption j back through the bytes, the
//               workgroup writes seq_n[b] as one contiguous block.
// The loop over the positions is uniform over the workgroup (n_b and "degenerate" are the same in every wavefront).  No atomics; the only float arithmetic is the float64
// add per pair.
constexpr int NR_MAX = BOFI_NBEST_NR_MAX;      // N at most
constexpr int NR_W = 8;                        // states per row = wavefronts per image = the stride of a state's list
static_assert(NR_MAX + 2 <= VP_K, "the candidates launch leaves VP_K ids per row: K = N + 2 of them are the states");
static_assert(VP_K == NR_W && NR_W * NR_W == WAVE && NR_MAX <= NR_W, "a wavefront's lanes hold every (state, entry) pair of the row before");

__global__ void __launch_bounds__(NR_W * WAVE) vocab_nbest_norepeat_kernel(NbArgs a, int lo, const int* __restrict__ work) {
    __shared__ double A_[2][WAVE];                              // [parity][r * 8 + j]: the lists' totals, -inf: no entry
    __shared__ double Tf[NR_W];                                 // the result's totals ...
    __shared__ uint8_t fl[NR_W];                                // ... and the slot r * 8 + j of A_{n-1} each came from
    __shared__ int cid[VC_MAX_S * NR_W];                        // c[p][r]; VC_NONE: the row has no such id
    __shared__ float xv[VC_MAX_S * NR_W];                       // x[p, c[p][r]]; NaN where there is no id
    __shared__ int out[NR_MAX * VC_MAX_S];                      // the captions, [N][S]
    __shared__ uint8_t bp[VC_MAX_S * WAVE];                     // [p][r * 8 + j]: the slot of A_{p-1} that entry j of A_p[r] came from
    const int tid = threadIdx.x, lane = tid % WAVE, r = __builtin_amdgcn_readfirstlane(tid / WAVE), b = blockIdx.x;
    const int S = a.S, N = a.N, V = a.V, K = N + 2;
    const int n = __builtin_amdgcn_readfirstlane(live_count(a.ntok, a.ntok_bias, b, S));
    const size_t row0 = (size_t)b * S;
    const double NINF = -(double)INFINITY;
    // the front end as vocab_nbest_kernel's, K entries a row: wavefront 0 has the ids and the cut rows, all threads the values
    const int cutk = nb_ids(work, row0, r == 0 ? n : 0, K, V, cid, lane);      // (no position in the other wavefronts)
    __syncthreads();
    if (r == 0) nb_cut_rows(a, row0, K, cutk, cid, lane);
    __syncthreads();
    nb_values(a, row0, n, cid, xv, tid, NR_W * WAVE);
    __syncthreads();
    const bool degen = nb_degen(xv, n, lane);                   // (every wavefront finds the same)
    const bool run = n > 0 && !degen;                           // (the same in every wavefront of the workgroup)
    if (run) {
        // A_0[r] = [0.0 + x[0, c[0][r]]]
        if (lane < NR_W) A_[0][r * NR_W + lane] = (lane == 0 && r < K && f32_finite(xv[r])) ? 0.0 + (double)xv[r] : NINF;
        __syncthreads();
        const int rp = lane / NR_W;                             // this lane's pair (r', j): the predecessor state
        for (int p = 1; p < n; ++p) {
            const double* const Ap = A_[(p - 1) & 1];
            double* const Ac = A_[p & 1];
            const float v = xv[p * NR_W + r];
            const int id = cid[p * NR_W + r], idp = cid[(p - 1) * NR_W + rp];
            const bool state = r < K && f32_finite(v);           // (wave-uniform) c[p][r] is a candidate
            const bool conf = idp == id && idp >= lo;           // the pair would repeat a word
            const unsigned long long cm = __ballot(conf);
            const double dv = (double)v, own = Ap[lane], mine = own + dv;
            const bool valid = state && !conf && own > NINF;
            int rank = 0;
            if (state) {
                for (int q = 0; q < K; ++q) {                   // the pairs of predecessor state q; a state past K holds no entry
                    if ((cm >> (q * NR_W)) & 1ull) continue;    // (wave-uniform: c[p-1][q] is this state's word)
                    double t[NR_MAX];
#pragma unroll
                    for (int j = 0; j < NR_MAX; ++j) t[j] = Ap[q * NR_W + j];      // (in flight together; an entry j >= N is -inf, and -inf + dv is in front of nothing)
#pragma unroll
                    for (int j = 0; j < NR_MAX; ++j) {
                        const double s = t[j] + dv;             // the same bits as that pair's own lane computes
                        rank += (int)(s > mine) | ((int)(s == mine) & (int)(q * NR_W + j < lane));
                    }
                }
            }
            const int nv = __popcll(__ballot(valid)), cnt = nv < N ? nv : N;
            if (valid && rank < N) { Ac[r * NR_W + rank] = mine; bp[p * WAVE + r * NR_W + rank] = (uint8_t)lane; }      // (the valid pairs' ranks are 0 .. nv-1, each once)
            if (lane < NR_W && lane >= cnt) Ac[r * NR_W + lane] = NINF;
            __syncthreads();
        }
    }
    // the result: wavefront 0 ranks all entries of A_{n-1}, lane = r * 8 + j
    int cnt = 1;
    if (r == 0 && run) {
        const double* const Al = A_[(n - 1) & 1];
        const double mine = Al[lane];
        const bool valid = mine > NINF;
        const int rank = nb_rank(Al, WAVE, mine, lane);
        if (valid && rank < N) { Tf[rank] = mine; fl[rank] = (uint8_t)lane; }
        const int nv = __popcll(__ballot(valid));
        cnt = nv < N ? nv : N;                                  // (0: no valid caption over the candidates)
    }
    __syncthreads();
    // lane j < N of wavefront 0: caption j into LDS, walked back along the slots
    if (r == 0) {
        if (lane < N) {
            int e = (run && lane < cnt) ? fl[lane] : 0;
            for (int p = S - 1; p >= 0; --p) {
                int id = a.pad_idx;
                if (p < n && lane < cnt) {
                    if (degen) { const int c = cid[p * NR_W]; id = c != VC_NONE ? c : a.pad_idx; }
                    else {
                        id = cid[p * NR_W + e / NR_W];
                        if (p > 0) e = bp[p * WAVE + e];
                    }
                }
                out[lane * S + p] = id;
            }
            a.total[(size_t)b * N + lane] = lane < cnt ? (degen ? (double)NAN : (n > 0 ? Tf[lane] : 0.0)) : NINF;
        }
        if (lane == 0) a.count[b] = cnt;
    }
    __syncthreads();
    nb_write_captions(a, b, out, tid, NR_W * WAVE);
}

// ---- the Hamming-diverse caption set (bofi_vocab_diverse): the reference's diverse beam search ('dbs': groups decoded one after another, each pushed away from the words
// the earlier groups put at the same position, CaptionModel.py:51-68) for the pass that scores every position on its own.  The augmented score of a caption is a sum of
// per-position terms, so every group's caption is the exact maximiser of its objective: a per-position pick, or with "no adjacent repeated word" a Viterbi over each
// row's candidates; include/boficap_hip.h, bofi_vocab_diverse, states the rule, tests/test_diverse_set.py restates it in numpy and holds it to a brute force.
//   candidates  the K-candidate launch above, unchanged (seq = NULL), as for the lists; K = N, or N + 2 under the repeat rule
//   groups      one wavefront per image, four images per workgroup; the lists' front end (ids to LDS, a cut row streamed again, the scattered value loads), behind
//               which LDS is only read and the kernel holds no barrier.  What changes from group to group stays in registers, lane = position: the counts of a row's
//               candidates as eight 4-bit fields of one word, the back-pointers of a row's eight states as a byte each of a 64-bit word.
//               no_repeat = 0: lane = position; a pass is one compare chain over the row's candidates.
//               no_repeat = 1: lane = r * 8 + r' is the pair (state r of row p, predecessor r' of row p - 1).  A step: the lane fetches V_{p-1}[r'] from the lanes of
//               state r' (a cross-lane read), adds its state's value -- one float64 add per pair --, the maximum over r' is a three-step butterfly inside the 8-lane
//               group on (has a V, value, then lower r'), three ballots pack the states' back-pointers for lane p.  The end state by a butterfly across the groups, the
//               walk back by scalar reads of the packed words.
//               The totals are summed left to right by reading lane after lane: that order is part of the rule.
// No atomics; the only float arithmetic is the float64 subtraction of a table entry (the table lambda * k comes from the host: the kernel never multiplies, nothing
// contracts) and the float64 adds.
constexpr int DV_IPW = 4;                      // images (wavefronts) per workgroup
constexpr int DV_PEN = 16;                     // the table in LDS: a 4-bit count indexes it
static_assert(BOFI_DIVERSE_MAX == VP_K && BOFI_DIVERSE_NR_MAX + 2 <= VP_K && VP_K * VP_K == WAVE, "the candidates launch leaves VP_K ids per row; the lanes hold every pair");
static_assert(BOFI_DIVERSE_MAX < DV_PEN, "a count fits its 4-bit field");

struct DvArgs {
    NbArgs nb;                                 // (seq_n, total, count: the set's)
    double pen[BOFI_DIVERSE_MAX];              // pen[k] = lambda * k, made on the host
    double* aug;
    int lo;                                    // repeat_min_id
};

// is (ok2, v2, i2) in front of (ok1, v1, i1)?  An entry that holds a value before one that does not, the larger value, then the lower index
__device__ __forceinline__ bool dv_front(bool ok2, double v2, int i2, bool ok1, double v1, int i1) {
    return ok2 && (!ok1 || v2 > v1 || (v2 == v1 && i2 < i1));
}

// one butterfly step at lane distance o: both partners keep the entry in front
__device__ __forceinline__ void dv_step(bool& ok, double& v, int& i, int o) {
    const bool ok2 = __shfl_xor((int)ok, o, WAVE) != 0;
    const double v2 = __shfl_xor(v, o, WAVE);
    const int i2 = __shfl_xor(i, o, WAVE);
    if (dv_front(ok2, v2, i2, ok, v, i)) { ok = ok2; v = v2; i = i2; }
}

__device__ __forceinline__ uint64_t dv_readlane64(uint64_t w, int p) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)w, p), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(w >> 32), p);
    return ((uint64_t)hi << 32) | lo;
}

template <bool NR>
__global__ void __launch_bounds__(DV_IPW * WAVE) vocab_diverse_kernel(DvArgs d, const int* __restrict__ work) {
    __shared__ int cid_[DV_IPW][VC_MAX_S * VP_K];               // c[p][r]; VC_NONE: the row has no such id
    __shared__ float xv_[DV_IPW][VC_MAX_S * VP_K];              // x[p, c[p][r]]; NaN where there is no id
    __shared__ double pen[DV_PEN];
    const NbArgs& a = d.nb;
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE, b = __builtin_amdgcn_readfirstlane(blockIdx.x * DV_IPW + wave);
    const bool on = b < a.B;                                    // (a wavefront past B stays for the barriers and touches no global memory)
    const int S = a.S, N = a.N, V = a.V, K = NR ? N + 2 : N;
    int* const cid = cid_[wave];
    float* const xv = xv_[wave];
    const int n = __builtin_amdgcn_readfirstlane(on ? live_count(a.ntok, a.ntok_bias, b, S) : 0);
    const size_t row0 = (size_t)(on ? b : 0) * S;
    if (threadIdx.x < DV_PEN) pen[threadIdx.x] = threadIdx.x < BOFI_DIVERSE_MAX ? d.pen[threadIdx.x] : 0.0;
    // the lists' front end, K entries a row
    const int cutk = nb_ids(work, row0, n, K, V, cid, lane);   // lane = position
    __syncthreads();
    nb_cut_rows(a, row0, K, cutk, cid, lane);
    __syncthreads();
    nb_values(a, row0, n, cid, xv, lane, WAVE);
    __syncthreads();
    if (!on) return;                                            // (no barrier from here on: LDS is only read)
    const double NINF = -(double)INFINITY;
    const size_t o0 = (size_t)b * N;                            // the image's first entry of total / aug; its rows of seq_n follow from it
    const bool degen = nb_degen(xv, n, lane);
    if (degen || n == 0) {                                      // one caption: each live row's first id; NaN for a degenerate image, 0.0 for the empty one
        int c0 = a.pad_idx;
        if (lane < n && cid[lane * VP_K] != VC_NONE) c0 = cid[lane * VP_K];
        if (lane < S)
            for (int g = 0; g < N; ++g) a.seq_n[(o0 + g) * S + lane] = (int64_t)(g == 0 ? c0 : a.pad_idx);
        if (lane < N) {
            const double t = lane == 0 ? (degen ? (double)NAN : 0.0) : NINF;
            a.total[o0 + lane] = t; d.aug[o0 + lane] = t;
        }
        if (lane == 0) a.count[b] = 1;
        return;
    }
    uint32_t cnt = 0;                                           // lane = position: field r = the earlier groups that took c[p][r]
    const int r = lane / VP_K, rp = lane % VP_K;                // (NR) this lane's pair: state r of row p, predecessor r' of row p - 1
    for (int g = 0; g < N; ++g) {
        int take = 0;                                           // lane = position: the candidate the group's caption has there
        double aug = 0.0;
        if (!NR) {
            double ba = 0.0;
            if (lane < n) {
                bool have = false;
#pragma unroll
                for (int k = 0; k < VP_K; ++k) {
                    const float v = xv[lane * VP_K + k];
                    const double av = (double)v - pen[(cnt >> (4 * k)) & 15u];
                    if (f32_finite(v) && (!have || av > ba)) { have = true; ba = av; take = k; }      // (ties to the lower k; entry 0 is finite here)
                }
            }
            for (int p = 0; p < n; ++p) aug = aug + __shfl(ba, p, WAVE);      // left to right
        } else {
            uint64_t bpw = 0ull;                                // lane = position p: byte r = the predecessor of state r of row p
            float v = xv[r];
            bool has = f32_finite(v);
            double Vc = 0.0 + ((double)v - pen[((uint32_t)__builtin_amdgcn_readlane((int)cnt, 0) >> (4 * r)) & 15u]);
            for (int p = 1; p < n; ++p) {
                v = xv[p * VP_K + r];
                const int id = cid[p * VP_K + r], idp = cid[(p - 1) * VP_K + rp];
                const double av = (double)v - pen[((uint32_t)__builtin_amdgcn_readlane((int)cnt, p) >> (4 * r)) & 15u];
                const unsigned long long hm = __ballot(has);
                const double Vp = __shfl(Vc, rp * VP_K, WAVE);  // V_{p-1}[r'], the same in every lane of state r'
                bool ok = f32_finite(v) && ((hm >> (rp * VP_K)) & 1ull) && !(idp == id && idp >= d.lo);
                double val = Vp + av;                           // one float64 add per pair
                int br = rp;
#pragma unroll
                for (int o = 1; o < VP_K; o <<= 1) dv_step(ok, val, br, o);      // the 8-lane group's best pair, in every lane of it
                Vc = val; has = ok;
                const uint64_t one = 0x0101010101010101ull;
                const uint64_t w = (__ballot(br & 1) & one) | ((__ballot(br & 2) & one) << 1) | ((__ballot(br & 4) & one) << 2);
                if (lane == p) bpw = w;
            }
            int er = r;                                         // the end state: the best V_{n-1}[r], ties to the lower r
#pragma unroll
            for (int o = VP_K; o < WAVE; o <<= 1) dv_step(has, Vc, er, o);
            if (!has) {                                         // no valid caption over the candidates, whatever the group (g = 0 here): count = 0
                if (lane < S)
                    for (int j = 0; j < N; ++j) a.seq_n[(o0 + j) * S + lane] = (int64_t)a.pad_idx;
                if (lane < N) { a.total[o0 + lane] = NINF; d.aug[o0 + lane] = NINF; }
                if (lane == 0) a.count[b] = 0;
                return;
            }
            aug = Vc;
            int rr = __builtin_amdgcn_readfirstlane(er);
            for (int p = n - 1; p >= 0; --p) {                  // back along the predecessors
                if (lane == p) take = rr;
                if (p > 0) rr = (int)((dv_readlane64(bpw, p) >> (8 * rr)) & 7ull);
            }
        }
        int id = a.pad_idx;
        float own = 0.f;
        if (lane < n) {
            id = cid[lane * VP_K + take];
            own = xv[lane * VP_K + take];
            cnt += 1u << (4 * take);
        }
        double total = 0.0;
        for (int p = 0; p < n; ++p) total = total + (double)__shfl(own, p, WAVE);      // the caption's own values, left to right
        if (lane < S) a.seq_n[(o0 + g) * S + lane] = (int64_t)id;
        if (lane == 0) { a.total[o0 + g] = total; d.aug[o0 + g] = aug; }
    }
    if (lane == 0) a.count[b] = N;
}

// ---- the host side
VcArgs vc_args(const float* x, int ldx, int V, int S, const int* ntok, int ntok_bias, int pad_idx, const uint32_t* ban_bits, int no_repeat, int repeat_min_id, int64_t* seq,
               float* row_chosen, int* changed) {
    VcArgs a{};
    a.x = x; a.ldx = ldx; a.V = V; a.S = S; a.ntok = ntok; a.ntok_bias = ntok_bias; a.pad_idx = pad_idx; a.ban = ban_bits; a.ban_words = (V + 31) / 32;
    a.ban_lds = a.ban_words <= VC_BAN_LDS_WORDS; a.no_repeat = no_repeat; a.repeat_min_id = repeat_min_id; a.seq = seq; a.row_chosen = row_chosen; a.changed = changed;
    return a;
}

// the candidate launches, one workgroup per row: the BAN form with a ban table, the table in dynamic LDS where it fits
inline size_t vc_ban_lds_bytes(const VcArgs& a) { return a.ban && a.ban_lds ? (size_t)a.ban_words * 4 : 0; }

int launch_candidates(const VcArgs& a, int rows, hipStream_t st) {
    if (a.ban) hipLaunchKernelGGL(vocab_candidates_kernel<true>, dim3(rows), dim3(VC_NT), vc_ban_lds_bytes(a), st, a);
    else hipLaunchKernelGGL(vocab_candidates_kernel<false>, dim3(rows), dim3(VC_NT), 0, st, a);
    BOFI_CHECK_LAUNCH();
    return BOFI_OK;
}

int launch_candidates_k(const VcArgs& a, int* work, int rows, hipStream_t st) {
    if (a.ban) hipLaunchKernelGGL(vocab_candidates_k_kernel<true>, dim3(rows), dim3(VC_NT), vc_ban_lds_bytes(a), st, a, work);
    else hipLaunchKernelGGL(vocab_candidates_k_kernel<false>, dim3(rows), dim3(VC_NT), 0, st, a, work);
    BOFI_CHECK_LAUNCH();
    return BOFI_OK;
}

// both lists: N at most n_max (n_range says so)
const char* list_check(const float* x, int ldx, int rows, int V, int S, int no_repeat, int repeat_min_id, int N, int n_max, const char* n_range, const int64_t* seq_n,
                       const double* total, const int* count, const void* work, size_t work_bytes) {
    if (!seq_n || !total || !count) return "non-null seq_n, total and count";
    if (const char* why = vocab_constrain_check(x, ldx, rows, V, S, no_repeat, repeat_min_id, seq_n)) return why;
    if (N < 1 || N > n_max) return n_range;
    if (rows > 0 && (!work || work_bytes < vocab_nbest_work_bytes(rows))) return "a workspace of bofi_vocab_nbest_workspace(rows) bytes";
    return nullptr;
}

// both lists (checked by the caller): the K-candidate launch (seq stays NULL: it writes the workspace only), then the list kernel
int launch_list(bool norepeat, const float* x, int ldx, int rows, int V, int S, const int* ntok, int ntok_bias, int pad_idx, const uint32_t* ban_bits, int repeat_min_id, int N,
                int64_t* seq_n, double* total, int* count, void* work, hipStream_t st) {
    if (rows == 0) return BOFI_OK;
    if (int rc = launch_candidates_k(vc_args(x, ldx, V, S, ntok, ntok_bias, pad_idx, ban_bits, 0, 0, nullptr, nullptr, nullptr), (int*)work, rows, st)) return rc;
    NbArgs nb{};
    nb.x = x; nb.ldx = ldx; nb.V = V; nb.S = S; nb.B = rows / S; nb.ntok = ntok; nb.ntok_bias = ntok_bias; nb.pad_idx = pad_idx; nb.ban = ban_bits; nb.N = N;
    nb.seq_n = seq_n; nb.total = total; nb.count = count;
    if (norepeat) hipLaunchKernelGGL(vocab_nbest_norepeat_kernel, dim3(nb.B), dim3(NR_W * WAVE), 0, st, nb, repeat_min_id, (const int*)work);      // one workgroup per image
    else hipLaunchKernelGGL(vocab_nbest_kernel, dim3((nb.B + NB_IPW - 1) / NB_IPW), dim3(NB_IPW * WAVE), 0, st, nb, (const int*)work);
    BOFI_CHECK_LAUNCH();
    return BOFI_OK;
}

}  // namespace

size_t bofi::vocab_nbest_work_bytes(int rows) { return vocab_pick_work_bytes(rows); }

const char* bofi::vocab_nbest_check(const float* x, int ldx, int rows, int V, int S, int N, const int64_t* seq_n, const double* total, const int* count, const void* work,
                                    size_t work_bytes) {
    return list_check(x, ldx, rows, V, S, 0, 0, N, NB_MAX, "N in 1..8 (BOFI_NBEST_MAX)", seq_n, total, count, work, work_bytes);
}

int bofi::launch_vocab_nbest(const float* x, int ldx, int rows, int V, int S, const int* ntok, int ntok_bias, int pad_idx, const uint32_t* ban_bits, int N,
                             int64_t* seq_n, double* total, int* count, void* work, size_t work_bytes, hipStream_t st) {
    if (vocab_nbest_check(x, ldx, rows, V, S, N, seq_n, total, count, work, work_bytes)) return BOFI_ERR_ARG;
    return launch_list(false, x, ldx, rows, V, S, ntok, ntok_bias, pad_idx, ban_bits, 0, N, seq_n, total, count, work, st);
}

extern "C" int64_t bofi_vocab_nbest_workspace(int rows) { return (int64_t)bofi::vocab_nbest_work_bytes(rows); }

extern "C" int bofi_vocab_nbest(const float* x, int ldx, int rows, int V, int S, const int* ntok, int ntok_bias, int pad_idx, const uint32_t* ban_bits, int N,
                                int64_t* seq_n, double* total, int* count, void* work, int64_t work_bytes, void* stream) {
    if (const char* why = bofi::vocab_nbest_check(x, ldx, rows, V, S, N, seq_n, total, count, work, work_bytes < 0 ? 0 : (size_t)work_bytes))
        return bofi::fail(BOFI_ERR_ARG, std::string("vocab_nbest: ") + why);
    return bofi::launch_vocab_nbest(x, ldx, rows, V, S, ntok, ntok_bias, pad_idx, ban_bits, N, seq_n, total, count, work, (size_t)work_bytes, (hipStream_t)stream);
}

const char* bofi::vocab_nbest_norepeat_check(const float* x, int ldx, int rows, int V, int S, int repeat_min_id, int N, const int64_t* seq_n, const double* total,
                                             const int* count, const void* work, size_t work_bytes) {
    return list_check(x, ldx, rows, V, S, 1, repeat_min_id, N, NR_MAX, "N in 1..6 (BOFI_NBEST_NR_MAX)", seq_n, total, count, work, work_bytes);
}

int bofi::launch_vocab_nbest_norepeat(const float* x, int ldx, int rows, int V, int S, const int* ntok, int ntok_bias, int pad_idx, const uint32_t* ban_bits,
                                      int repeat_min_id, int N, int64_t* seq_n, double* total, int* count, void* work, size_t work_bytes, hipStream_t st) {
    if (vocab_nbest_norepeat_check(x, ldx, rows, V, S, repeat_min_id, N, seq_n, total, count, work, work_bytes)) return BOFI_ERR_ARG;
    return launch_list(true, x, ldx, rows, V, S, ntok, ntok_bias, pad_idx, ban_bits, repeat_min_id, N, seq_n, total, count, work, st);
}

extern "C" int bofi_vocab_nbest_norepeat(const float* x, int ldx, int rows, int V, int S, const int* ntok, int ntok_bias, int pad_idx, const uint32_t* ban_bits,
                                         int repeat_min_id, int N, int64_t* seq_n, double* total, int* count, void* work, int64_t work_bytes, void* stream) {
    if (const char* why = bofi::vocab_nbest_norepeat_check(x, ldx, rows, V, S, repeat_min_id, N, seq_n, total, count, work, work_bytes < 0 ? 0 : (size_t)work_bytes))
        return bofi::fail(BOFI_ERR_ARG, std::string("vocab_nbest_norepeat: ") + why);
    return bofi::launch_vocab_nbest_norepeat(x, ldx, rows, V, S, ntok, ntok_bias, pad_idx, ban_bits, repeat_min_id, N, seq_n, total, count, work, (size_t)work_bytes,
                                             (hipStream_t)stream);
}

const char* bofi::vocab_diverse_check(const float* x, int ldx, int rows, int V, int S, int N, double lambda, int no_repeat, int repeat_min_id, const int64_t* seq_n,
                                      const double* total, const double* aug, const int* count, const void* work, size_t work_bytes) {
    if (!aug) return "non-null seq_n, total, aug and count";
    if (no_repeat != 0 && no_repeat != 1) return "no_repeat 0 or 1";
    if (const char* why = list_check(x, ldx, rows, V, S, no_repeat, repeat_min_id, N, no_repeat ? BOFI_DIVERSE_NR_MAX : BOFI_DIVERSE_MAX,
                                     no_repeat ? "N in 1..6 under no_repeat (BOFI_DIVERSE_NR_MAX)" : "N in 1..8 (BOFI_DIVERSE_MAX)", seq_n, total, count, work, work_bytes))
        return why;
    if (!(lambda >= 0.0) || std::isinf(lambda)) return "a finite lambda >= 0";
    return nullptr;
}

int bofi::launch_vocab_diverse(const float* x, int ldx, int rows, int V, int S, const int* ntok, int ntok_bias, int pad_idx, const uint32_t* ban_bits, int N, double lambda,
                               int no_repeat, int repeat_min_id, int64_t* seq_n, double* total, double* aug, int* count, void* work, size_t work_bytes, hipStream_t st) {
    if (vocab_diverse_check(x, ldx, rows, V, S, N, lambda, no_repeat, repeat_min_id, seq_n, total, aug, count, work, work_bytes)) return BOFI_ERR_ARG;
    if (rows == 0) return BOFI_OK;
    if (int rc = launch_candidates_k(vc_args(x, ldx, V, S, ntok, ntok_bias, pad_idx, ban_bits, 0, 0, nullptr, nullptr, nullptr), (int*)work, rows, st)) return rc;
    DvArgs d{};
    NbArgs& nb = d.nb;
    nb.x = x; nb.ldx = ldx; nb.V = V; nb.S = S; nb.B = rows / S; nb.ntok = ntok; nb.ntok_bias = ntok_bias; nb.pad_idx = pad_idx; nb.ban = ban_bits; nb.N = N;
    nb.seq_n = seq_n; nb.total = total; nb.count = count;
    for (int k = 0; k < BOFI_DIVERSE_MAX; ++k) d.pen[k] = k < N ? lambda * (double)k : 0.0;      // the one product of the rule, on the host; pen[0] = 0.0
    d.aug = aug; d.lo = repeat_min_id;
    const dim3 grid((nb.B + DV_IPW - 1) / DV_IPW), block(DV_IPW * WAVE);
    if (no_repeat) hipLaunchKernelGGL(vocab_diverse_kernel<true>, grid, block, 0, st, d, (const int*)work);
    else hipLaunchKernelGGL(vocab_diverse_kernel<false>, grid, block, 0, st, d, (const int*)work);
    BOFI_CHECK_LAUNCH();
    return BOFI_OK;
}

extern "C" int bofi_vocab_diverse(const float* x, int ldx, int rows, int V, int S, const int* ntok, int ntok_bias, int pad_idx, const uint32_t* ban_bits, int N,
                                  double lambda, int no_repeat, int repeat_min_id, int64_t* seq_n, double* total, double* aug, int* count, void* work,
                                  int64_t work_bytes, void* stream) {
    if (const char* why = bofi::vocab_diverse_check(x, ldx, rows, V, S, N, lambda, no_repeat, repeat_min_id, seq_n, total, aug, count, work,
                                                    work_bytes < 0 ? 0 : (size_t)work_bytes))
        return bofi::fail(BOFI_ERR_ARG, std::string("vocab_diverse: ") + why);
    return bofi::launch_vocab_diverse(x, ldx, rows, V, S, ntok, ntok_bias, pad_idx, ban_bits, N, lambda, no_repeat, repeat_min_id, seq_n, total, aug, count, work,
                                      (size_t)work_bytes, (hipStream_t)stream);
}

size_t bofi::vocab_pick_work_bytes(int rows) { return (size_t)(rows > 0 ? rows : 0) * VP_K * sizeof(int); }

const char* bofi::vocab_pick_check(const float* x, int ldx, int rows, int V, int S, int no_repeat, int block_trigrams, int repeat_min_id, const int64_t* seq,
                                   const void* work, size_t work_bytes) {
    if (const char* why = vocab_constrain_check(x, ldx, rows, V, S, no_repeat, repeat_min_id, seq)) return why;
    if (block_trigrams != 0 && block_trigrams != 1) return "block_trigrams 0 or 1";
    if (rows > 0 && (!work || work_bytes < vocab_pick_work_bytes(rows))) return "a workspace of bofi_vocab_pick_workspace(rows) bytes";
    return nullptr;
}

int bofi::launch_vocab_pick(const float* x, int ldx, int rows, int V, int S, const int* ntok, int ntok_bias, int pad_idx, const uint32_t* ban_bits, int no_repeat,
                            int block_trigrams, int repeat_min_id, int64_t* seq, float* row_chosen, int* changed, void* work, size_t work_bytes, hipStream_t st) {
    if (vocab_pick_check(x, ldx, rows, V, S, no_repeat, block_trigrams, repeat_min_id, seq, work, work_bytes)) return BOFI_ERR_ARG;
    if (rows == 0) return BOFI_OK;
    const VcArgs a = vc_args(x, ldx, V, S, ntok, ntok_bias, pad_idx, ban_bits, no_repeat, repeat_min_id, seq, row_chosen, changed);
    const int B = rows / S;
    if (int rc = launch_candidates_k(a, (int*)work, rows, st)) return rc;
    hipLaunchKernelGGL(vocab_scan_k_kernel, dim3((B + VC_SCAN_WAVES - 1) / VC_SCAN_WAVES), dim3(VC_SCAN_WAVES * WAVE), 0, st, a, (const int*)work, block_trigrams, B);
    BOFI_CHECK_LAUNCH();
    return BOFI_OK;
}

extern "C" int64_t bofi_vocab_pick_workspace(int rows) { return (int64_t)bofi::vocab_pick_work_bytes(rows); }

extern "C" int bofi_vocab_pick(const float* x, int ldx, int rows, int V, int S, const int* ntok, int ntok_bias, int pad_idx, const uint32_t* ban_bits, int no_repeat,
                               int block_trigrams, int repeat_min_id, int64_t* seq, float* row_chosen, int* changed, void* work, int64_t work_bytes, void* stream) {
    if (const char* why = bofi::vocab_pick_check(x, ldx, rows, V, S, no_repeat, block_trigrams, repeat_min_id, seq, work, work_bytes < 0 ? 0 : (size_t)work_bytes))
        return bofi::fail(BOFI_ERR_ARG, std::string("vocab_pick: ") + why);
    return bofi::launch_vocab_pick(x, ldx, rows, V, S, ntok, ntok_bias, pad_idx, ban_bits, no_repeat, block_trigrams, repeat_min_id, seq, row_chosen, changed, work,
                                   (size_t)work_bytes, (hipStream_t)stream);
}

int bofi::launch_vocab_constrain(const float* x, int ldx, int rows, int V, int S, const int* ntok, int ntok_bias, int pad_idx, const uint32_t* ban_bits,
                                 int no_repeat, int repeat_min_id, int64_t* seq, float* row_chosen, int* changed, hipStream_t st) {
    if (vocab_constrain_check(x, ldx, rows, V, S, no_repeat, repeat_min_id, seq)) return BOFI_ERR_ARG;
    if (rows == 0) return BOFI_OK;
    const VcArgs a = vc_args(x, ldx, V, S, ntok, ntok_bias, pad_idx, ban_bits, no_repeat, repeat_min_id, seq, row_chosen, changed);
    const int B = rows / S;
    if (int rc = launch_candidates(a, rows, st)) return rc;
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
