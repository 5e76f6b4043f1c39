// Oracle and average language scores of an image's n sampled captions (the reference's --eval_oracle 1: eval_utils.py:112-114 over the
// per-sentence scores of COCOEvalCap), on the device.
//
// Input: the per-candidate outputs of bofi_reward_score (the BLEU counts and the CIDEr value) and bofi_rouge_score at seq_per_img = n, so
// row m * n + i is sample i of image m.  One wavefront per image, four images per workgroup; lane j < n turns sample j's counts into its
// sentence-level BLEU-1..4 -- the operations of reward_score_kernel (cider.hip) in their order, restated here so that kernel stays as it
// is: a running product of (correct + 1e-15) / (guess + 1e-9), pow(b, 1 / (k + 1)) per order, every order times exp(1 - 1 / ratio) when
// ratio < 1 -- and holds the six values Bleu_1..4, ROUGE_L, CIDEr.  Per metric the wavefront then finds the maximum by comparisons (exact),
// the lowest lane that attains it (a ballot), and the sum in index order (one lane-by-lane pass, one division by n): no atomics, every loop
// bounded by n or the wavefront, bit-identical run to run and reproducible on the host.  A NaN among the n values (a CIDEr whose row held
// an id without a key) makes the metric's oracle and average NaN and its pick -1.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "bofi_common.h"
#include "boficap_hip.h"

namespace {

constexpr int WAVE = 64;
constexpr int WAVES = 4;          // images per workgroup
constexpr int ORDERS = 4;
constexpr int METRICS = 6;        // Bleu_1, Bleu_2, Bleu_3, Bleu_4, ROUGE_L, CIDEr
constexpr int COMPS = 2 + 2 * ORDERS;

// BLEU-1..4 of one sentence's counts c = (testlen, reflen, guess[4], correct[4])
__device__ inline void sentence_bleu(const int* c, double* out) {
#pragma clang fp contract(off)
    const double tiny = 1e-15, small = 1e-9;
    double b = 1.0;
    for (int k = 0; k < ORDERS; ++k) {
        b *= ((double)c[2 + ORDERS + k] + tiny) / ((double)c[2 + k] + small);
        out[k] = pow(b, 1.0 / (double)(k + 1));
    }
    const double ratio = ((double)c[0] + tiny) / ((double)c[1] + small);
    if (ratio < 1.0) {
        const double f = exp(1.0 - 1.0 / ratio);
        for (int k = 0; k < ORDERS; ++k) out[k] *= f;
    }
}

__global__ void __launch_bounds__(WAVE * WAVES) oracle_stats_kernel(const int* __restrict__ comps, const double* __restrict__ cider,
                                                                   const double* __restrict__ rouge, int images, int n,
                                                                   double* __restrict__ sent, double* __restrict__ stats, int* __restrict__ pick) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x % WAVE;
    const int img = blockIdx.x * WAVES + threadIdx.x / WAVE;
    if (img >= images) return;                            // the last workgroup's tail: whole wavefronts leave, and nothing below waits for them
    const bool live = lane < n;
    double v[METRICS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (live) {
        const int64_t row = (int64_t)img * n + lane;
        int c[COMPS];
        for (int q = 0; q < COMPS; ++q) c[q] = comps[row * COMPS + q];
        sentence_bleu(c, v);
        v[ORDERS] = rouge[row];
        v[ORDERS + 1] = cider[row];
        if (sent)
            for (int m = 0; m < METRICS; ++m) sent[row * METRICS + m] = v[m];
    }
    for (int m = 0; m < METRICS; ++m) {
        const double x = v[m];
        const bool bad = __ballot(live && x != x) != 0;
        double best = live ? x : -INFINITY;
        for (int off = WAVE / 2; off > 0; off >>= 1) {
            const double o = __shfl_xor(best, off, WAVE);
            if (o > best) best = o;
        }
        const unsigned long long at = __ballot(live && x == best);
        double s = 0.0;
        for (int j = 0; j < n; ++j) s += __shfl(x, j, WAVE);      // index order
        if (lane == 0) {
            const int64_t o = (int64_t)img * METRICS + m;
            stats[2 * o] = bad ? __builtin_nan("") : best;
            stats[2 * o + 1] = s / (double)n;                     // (NaN with a NaN among the values)
            pick[o] = bad || at == 0 ? -1 : __ffsll(at) - 1;
        }
    }
}

}  // namespace

extern "C" int bofi_oracle_stats(const int* comps, const double* cider, const double* rouge, int images, int n, double* sent, double* stats, int* pick,
                                 void* stream) {
    if (!comps || !cider || !rouge || !stats || !pick || n < 1 || n > WAVE || images < 0) return BOFI_ERR_ARG;
    if (images == 0) return BOFI_OK;
    hipLaunchKernelGGL(oracle_stats_kernel, dim3((images + WAVES - 1) / WAVES), dim3(WAVE * WAVES), 0, (hipStream_t)stream, comps, cider, rouge, images, n,
                       sent, stats, pick);
    BOFI_CHECK_LAUNCH();
    return BOFI_OK;
}
