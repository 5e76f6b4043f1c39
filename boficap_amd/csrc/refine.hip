// Mask-predict refinement of the filling pass: the per-image step between two passes (BOFI_FLAG_MASK_PREDICT; the rules are stated in
// include/boficap_hip.h at bofi_mask_predict_step and in DESIGN.md).
//
// Pass t = 0 .. T of the filling pass leaves, per position, a greedy id, its log-prob ("confidence") and sum_v p log p.  This kernel
// runs after each pass.  One wavefront per image, four images per workgroup; lane s < S holds position s.
//   merge:  a position inside the image's n = last - 1 tokens takes the fresh values when it was in the mask of pass t (pass 0: always)
//           and keeps the state otherwise; the pad tail s >= n always takes the fresh values (pad, round 0).
//   select: when another pass follows, the k = n (T - t) / (T + 1) least confident of the n positions form its mask -- rank(s) counts the
//           positions that come before s in the total order (NaN first, then by value, ties and NaNs by position), one lane-by-lane
//           pass of S reads -- and its input ids are BOS under the mask and the state's id elsewhere.
//   export: after the last pass the state goes to the caller's buffers.
// No atomics, no data-dependent loop, comparisons only: bit-identical run to run and reproducible on the host.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bofi_common.h"
#include "bofi_kernels.h"
#include "boficap_hip.h"

namespace {

constexpr int WAVE = 64;
constexpr int WAVES = 4;          // images per workgroup

// does (a, position ja) come before (b, position jb)?  NaN ranks below every number; equal values and NaNs go by position
__device__ __forceinline__ bool conf_before(float a, int ja, float b, int jb) {
    const bool na = a != a, nb = b != b;
    if (na != nb) return na;
    if (na) return ja < jb;
    return a < b || (a == b && ja < jb);
}

__global__ void __launch_bounds__(WAVE * WAVES) mask_predict_step(bofi::MaskPredictArgs a) {
    const int lane = threadIdx.x % WAVE;
    const int b = blockIdx.x * WAVES + threadIdx.x / WAVE;
    if (b >= a.B) return;                                 // the last workgroup's tail: whole wavefronts leave, and nothing below waits for them
    const int S = a.S;
    const bool live = lane < S;
    int n = a.last[b] - 1;
    n = n < 0 ? 0 : (n > S ? S : n);
    const int64_t at = (int64_t)b * S + lane;
    int64_t y = a.pad_idx;
    float c = 0.f, e = 0.f;
    int r = 0;
    if (live) {
        const bool fresh = lane >= n || a.t == 0 || a.mask[at] != 0;
        if (fresh) {
            y = a.fresh_ids[at]; c = a.fresh_chosen[at]; e = a.fresh_plogp[at];
            r = lane < n ? a.t : 0;
            a.ids[at] = y; a.chosen[at] = c; a.plogp[at] = e; a.round[at] = r;
        } else {
            y = a.ids[at]; c = a.chosen[at]; e = a.plogp[at]; r = a.round[at];
        }
    }
    if (a.t < a.T) {
        const int k = n * (a.T - a.t) / (a.T + 1);        // the next pass, t + 1: n (T + 1 - (t + 1)) / (T + 1)
        int rank = 0;
        for (int j = 0; j < S; ++j) {                     // (every lane of the wavefront takes part in the reads)
            const float cj = __shfl(c, j, WAVE);
            rank += (j < n && conf_before(cj, j, c, lane)) ? 1 : 0;
        }
        if (live) {
            const bool m = lane < n && rank < k;
            a.mask[at] = m ? 1 : 0;
            a.next_ids[at] = m ? (int64_t)a.bos_idx : y;
        }
    } else if (live) {
        a.seq_out[at] = y;
        if (a.plogp_out) { a.plogp_out[at] = e; a.chosen_out[at] = c; }
        if (a.round_out) a.round_out[at] = r;
    }
}

}  // namespace

int bofi::mask_predict_check(const MaskPredictArgs& a) {
    if (a.B < 1 || a.S < 1 || a.S > WAVE || a.T < 0 || a.T > 15 || a.t < 0 || a.t > a.T) return BOFI_ERR_ARG;
    if (!a.ids || !a.chosen || !a.plogp || !a.round || !a.fresh_ids || !a.fresh_chosen || !a.fresh_plogp || !a.mask || !a.next_ids || !a.last) return BOFI_ERR_ARG;
    if (a.t == a.T && !a.seq_out) return BOFI_ERR_ARG;
    if (!a.plogp_out != !a.chosen_out) return BOFI_ERR_ARG;
    return BOFI_OK;
}

int bofi::launch_mask_predict_step(const MaskPredictArgs& a, hipStream_t st) {
    const int rc = mask_predict_check(a);
    if (rc != BOFI_OK) return rc;
    hipLaunchKernelGGL(mask_predict_step, dim3((a.B + WAVES - 1) / WAVES), dim3(WAVE * WAVES), 0, st, a);
    BOFI_CHECK_LAUNCH();
    return BOFI_OK;
}

extern "C" int bofi_mask_predict_step(int64_t* ids, float* chosen, float* plogp, int* round, const int64_t* fresh_ids, const float* fresh_chosen,
                                      const float* fresh_plogp, int* mask, int64_t* next_ids, const int* last, int B, int S, int t, int T, int bos_idx,
                                      int pad_idx, int64_t* seq_out, float* plogp_out, float* chosen_out, int* round_out, void* stream) {
    bofi::MaskPredictArgs a{};
    a.ids = ids; a.chosen = chosen; a.plogp = plogp; a.round = round; a.fresh_ids = fresh_ids; a.fresh_chosen = fresh_chosen; a.fresh_plogp = fresh_plogp;
    a.mask = mask; a.next_ids = next_ids; a.last = last; a.B = B; a.S = S; a.t = t; a.T = T; a.bos_idx = bos_idx; a.pad_idx = pad_idx;
    a.seq_out = seq_out; a.plogp_out = plogp_out; a.chosen_out = chosen_out; a.round_out = round_out;
    if (bofi::mask_predict_check(a) != BOFI_OK)
        return bofi::fail(BOFI_ERR_ARG, "mask_predict_step: B >= 1, 1 <= S <= 64, 0 <= t <= T <= 15, non-null state / fresh / mask / next_ids / last, seq_out after the last pass, both row-statistics outputs or none");
    return bofi::launch_mask_predict_step(a, (hipStream_t)stream);
}
