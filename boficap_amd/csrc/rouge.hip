// ROUGE-L of the validation pass (the Rouge scorer of the pycocoevalcap package, beta = 1.2) on id token lists, on the device.
//
// One wavefront per candidate.  Its tokens sit in LDS; lane i takes the image's references i, i + 64, ... and runs the 64-bit
// bit-vector recurrence of the longest common subsequence on each: V starts as all ones, and for every reference token with match
// mask M over the candidate's positions U = V & M, V = (V + U) | (V - U); the zero bits of V count the subsequence.  Rows hold at
// most 64 tokens, so one word serves, and the bits above a shorter candidate stay set (M is 0 there and V - U never borrows).
//
// p = max_i lcs_i / |c| and r = max_i lcs_i / |r_i| are found on the integers (fractions with denominators <= 64 compare by cross
// products exactly as their fp64 quotients do); the lowest reference index wins a tie.  The score is fp64 in one fixed order with
// contraction off, so results are bit-identical run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "bofi_common.h"
#include "boficap_hip.h"

namespace {

constexpr int ROUGE_MAX_TOKENS = 64;
constexpr int WAVE = 64;

struct Best {                     // a reference's fraction num / den (den >= 1) and its index within the image; idx < 0: none yet
    int num, den, idx;
};

__device__ inline bool better(const Best& a, const Best& b) {      // a beats b: the larger fraction, else the lower index
    if (a.idx < 0) return false;
    if (b.idx < 0) return true;
    const int x = a.num * b.den, y = b.num * a.den;
    return x > y || (x == y && a.idx < b.idx);
}

__device__ inline Best wave_best(Best v) {
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        Best o;
        o.num = __shfl_xor(v.num, off, WAVE);
        o.den = __shfl_xor(v.den, off, WAVE);
        o.idx = __shfl_xor(v.idx, off, WAVE);
        if (better(o, v)) v = o;
    }
    return v;
}

__global__ void __launch_bounds__(WAVE) rouge_score_kernel(const int64_t* __restrict__ seq, const int* __restrict__ cand_len, int S, int seq_per_img,
                                                           const int* __restrict__ ref_start, const int* __restrict__ ref_tok,
                                                           const int* __restrict__ ref_len, int width, int eval_rule, double beta,
                                                           double* __restrict__ out64, int* __restrict__ lcs, int* __restrict__ best) {
#pragma clang fp contract(off)
    __shared__ int64_t tok[ROUGE_MAX_TOKENS];
    const int j = blockIdx.x, lane = threadIdx.x;
    const int64_t* row = seq + (int64_t)j * S;
    // the candidate's token list: cand_len[j] ids, else the ids up to and including the first 0 ('reward' rule) or before the first
    // id <= 0 ('eval' rule), else the whole row
    const int64_t v = lane < S ? row[lane] : 1;
    const bool stop = lane < S && (eval_rule ? v <= 0 : v == 0);
    const unsigned long long stops = __ballot(stop);
    int T = S;
    if (cand_len)
        T = min(max(cand_len[j], 0), S);
    else if (stops)
        T = __ffsll(stops) - 1 + (eval_rule ? 0 : 1);
    tok[lane] = v;
    __syncthreads();

    const int img = j / seq_per_img;
    const int r0 = ref_start[img], n = ref_start[img + 1] - r0;
    const int64_t pair0 = (int64_t)r0 * seq_per_img + (int64_t)(j % seq_per_img) * n;      // candidate j's pairs in the lcs output
    Best bp = {0, 1, -1}, br = {0, 1, -1};
    for (int i = lane; i < n; i += WAVE) {
        const int ref = r0 + i;
        const int len = min(max(ref_len[ref], 0), width);
        const int* rt = ref_tok + (int64_t)ref * width;
        uint64_t V = ~0ull;
        for (int q = 0; q < len; ++q) {
            const int64_t y = rt[q];
            uint64_t M = 0;
            for (int c = 0; c < T; ++c) M |= (uint64_t)(tok[c] == y) << c;
            const uint64_t U = V & M;
            V = (V + U) | (V - U);
        }
        const int l = __popcll(~V);
        if (lcs) lcs[pair0 + i] = l;
        const Best cp = {l, 1, i}, cr = {l, max(len, 1), i};      // |c| is the same for every pair: p compares by lcs alone
        if (better(cp, bp)) bp = cp;
        if (better(cr, br)) br = cr;
    }
    bp = wave_best(bp);
    br = wave_best(br);
    if (lane == 0) {
        const double p = T > 0 && bp.idx >= 0 ? (double)bp.num / (double)T : 0.0;
        const double r = br.idx >= 0 ? (double)br.num / (double)br.den : 0.0;
        const double b2 = beta * beta;
        double s = 0.0;
        if (p != 0.0 && r != 0.0) s = (1.0 + b2) * p * r / (r + b2 * p);
        out64[j] = s;
        if (best) {
            best[2 * j] = bp.idx;
            best[2 * j + 1] = br.idx;
        }
    }
}

}  // namespace

extern "C" int bofi_rouge_score(const int64_t* seq, const int* cand_len, int N, int S, int seq_per_img, const int* ref_start, const int* ref_tok,
                                const int* ref_len, int width, int eval_rule, double beta, double* out64, int* lcs, int* best, void* stream) {
    if (!seq || !ref_start || !ref_len || !out64 || N < 0 || S < 1 || S > ROUGE_MAX_TOKENS || seq_per_img < 1 || N % seq_per_img != 0 || width < 0 ||
        width > ROUGE_MAX_TOKENS || (width > 0 && !ref_tok) || (eval_rule != 0 && eval_rule != 1) || !std::isfinite(beta) || !(beta > 0.0))
        return BOFI_ERR_ARG;
    if (N == 0) return BOFI_OK;
    hipLaunchKernelGGL(rouge_score_kernel, dim3(N), dim3(WAVE), 0, (hipStream_t)stream, seq, cand_len, S, seq_per_img, ref_start, ref_tok, ref_len, width,
                       eval_rule, beta, out64, lcs, best);
    BOFI_CHECK_LAUNCH();
    return BOFI_OK;
}
