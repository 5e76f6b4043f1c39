// CIDEr-D caption reward (the scorer of captioning/utils/rewards.py:86-131, CiderD of the pyciderevalcap package) on the device.
//
// Every row -- a reference caption or a sampled candidate -- becomes a record: its unique n-grams (n = 1..4) as sorted 64-bit keys,
// their weights tf * (L - log(max(1, df))), the four per-order norms and the row's "length" (its number of bigrams, a quirk of the
// package kept on purpose).  An n-gram's key packs (id + 1) into 16-bit fields, first token in the highest used field, so keys are
// exact, and the keys of order k lie in [2^(16(k-1)), 2^(16k)): a sorted record is grouped by order.
//
// bofi_cider_refs builds the references' records into global memory (one workgroup per reference row); bofi_cider_score builds each
// candidate's record in LDS (one workgroup per candidate) and scores it against the records of its image's references.  All
// arithmetic is fp64; every reduction runs in a fixed order, so results are bit-identical run to run.
//
// bofi_reward_refs / bofi_reward_score are the whole reward of get_scores, cider_weight * CIDEr-D + bleu_weight * BLEU-4 (the Bleu(4)
// scorer of the pycocoevalcap package, option 'closest'): the same records plus each unique n-gram's raw count and the row's token
// count, and one binary search per candidate n-gram and reference that serves both terms.  BLEU's clipped counts are integer sums.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "bofi_common.h"
#include "bofi_record.h"
#include "boficap_hip.h"

namespace {

// record layout in global memory, per row: keys / weights [stride], off [5] (int), meta [5] = norms, length; with the counts (rec_cnt not
// NULL) also each unique n-gram's raw count [stride] (0 in the unused tail) and the row's token count
template <int NT>
__global__ void __launch_bounds__(NT) cider_refs_kernel(const int* ref_tok, const int* ref_len, int width, const uint64_t* df_keys,
                                                        const double* df_vals, int n_df, double L, uint64_t* rec_keys, double* rec_w,
                                                        int* rec_off, double* rec_meta, int* rec_cnt, int* rec_len, int stride) {
    __shared__ RecordLds<NT> r;
    const int row = blockIdx.x, t = threadIdx.x;
    if (t == 0) r.T = min(max(ref_len[row], 0), width);
    __syncthreads();
    if (t < r.T) r.tok[t] = ref_tok[(int64_t)row * width + t];
    __syncthreads();
    build_record<NT>(r, df_keys, df_vals, n_df, L);
    const int nU = r.off[CIDER_ORDERS];
    for (int q = t; q < stride; q += NT) {
        rec_keys[(int64_t)row * stride + q] = q < nU ? r.key[q] : KEY_NONE;
        rec_w[(int64_t)row * stride + q] = q < nU ? r.w[q] : 0.0;
        if (rec_cnt) rec_cnt[(int64_t)row * stride + q] = q < nU ? (int)r.part[q] : 0;    // build_record leaves the tf in r.part
    }
    if (t <= CIDER_ORDERS) rec_off[row * (CIDER_ORDERS + 1) + t] = r.off[t];
    if (t < CIDER_ORDERS) rec_meta[row * (CIDER_ORDERS + 1) + t] = r.norm[t];
    if (t == CIDER_ORDERS) rec_meta[row * (CIDER_ORDERS + 1) + t] = r.length;
    if (rec_len && t == 0) rec_len[row] = r.T;
}

// CIDEr-D's term of one reference for order t + 1 (thread t < 4) from the products min(w_h, w_r) * w_r in r.part; meta = the
// reference's norms and length
template <int NT>
__device__ inline double cider_term(const RecordLds<NT>& r, int t, const double* meta, double two_sigma2) {
    double val = 0.0;
    for (int q = r.off[t]; q < r.off[t + 1]; ++q) val += r.part[q];
    const double nr = meta[t];
    if (r.norm[t] != 0.0 && nr != 0.0) val /= r.norm[t] * nr;
    const double delta = r.length - meta[CIDER_ORDERS];
    return val * exp(-(delta * delta) / two_sigma2);
}

// 10 * mean over the orders / number of references
__device__ inline double cider_value(const double* acc, int n_refs) {
    double s = (acc[0] + acc[1] + acc[2] + acc[3]) / (double)CIDER_ORDERS;
    return s / (double)n_refs * 10.0;
}

template <int NT>
__global__ void __launch_bounds__(NT) cider_score_kernel(const int64_t* seq, const int* cand_len, int S, int seq_per_img, const int* ref_start,
                                                         const uint64_t* df_keys, const double* df_vals, int n_df, double L, double sigma,
                                                         double weight, const uint64_t* rec_keys, const double* rec_w, const int* rec_off,
                                                         const double* rec_meta, int stride, float* out, double* out64) {
    __shared__ RecordLds<NT> r;
    __shared__ double acc[CIDER_ORDERS];
    const int j = blockIdx.x, t = threadIdx.x;
    if (t < CIDER_ORDERS) acc[t] = 0.0;
    load_candidate<NT>(r, seq + (int64_t)j * S, cand_len, j, S);
    build_record<NT>(r, df_keys, df_vals, n_df, L);
    const int img = j / seq_per_img;
    const int r0 = ref_start[img], r1 = ref_start[img + 1];
    const int nU = r.off[CIDER_ORDERS];
    const double two_sigma2 = 2.0 * sigma * sigma;
    for (int ref = r0; ref < r1; ++ref) {                 // the image's references in index order
        const uint64_t* rk = rec_keys + (int64_t)ref * stride;
        const double* rw = rec_w + (int64_t)ref * stride;
        const int n_ref = rec_off[ref * (CIDER_ORDERS + 1) + CIDER_ORDERS];
        if (t < nU) {                                     // min(w_h, w_r) * w_r; w_r = 0 where the reference lacks the n-gram
            const int i = find_key(rk, n_ref, r.key[t]);
            const double wr = i < n_ref ? rw[i] : 0.0;
            r.part[t] = fmin(r.w[t], wr) * wr;
        }
        __syncthreads();
        if (t < CIDER_ORDERS) acc[t] += cider_term<NT>(r, t, rec_meta + ref * (CIDER_ORDERS + 1), two_sigma2);
        __syncthreads();
    }
    if (t == 0) {
        double s = cider_value(acc, r1 - r0);
        if (r.bad) s = __builtin_nan("");                 // an id outside [0, 65534] has no key: the score says so
        s *= weight;
        out[j] = (float)s;
        if (out64) out64[j] = s;
    }
}

// cider_weight * CIDEr-D + bleu_weight * BLEU-4 of candidate j.  One search per unique candidate n-gram and reference gives the reference's
// weight (CIDEr-D) and its count, whose running maximum over the references clips the candidate's count (BLEU).
template <int NT>
__global__ void __launch_bounds__(NT) reward_score_kernel(const int64_t* seq, const int* cand_len, int S, int seq_per_img, const int* ref_start,
                                                          const uint64_t* df_keys, const double* df_vals, int n_df, double L, double sigma,
                                                          double cider_weight, double bleu_weight, const uint64_t* rec_keys, const double* rec_w,
                                                          const int* rec_off, const double* rec_meta, const int* rec_cnt, const int* rec_len,
                                                          int stride, float* out, double* out64, int* comps) {
    __shared__ RecordLds<NT> r;
    __shared__ double acc[CIDER_ORDERS];
    __shared__ int clipped[NT];
    const int j = blockIdx.x, t = threadIdx.x;
    const bool with_cider = cider_weight != 0.0;          // 0: no CIDEr-D work at all (and no df table needed)
    if (t < CIDER_ORDERS) acc[t] = 0.0;
    load_candidate<NT>(r, seq + (int64_t)j * S, cand_len, j, S);
    build_record<NT>(r, df_keys, df_vals, n_df, L);
    const int img = j / seq_per_img;
    const int r0 = ref_start[img], r1 = ref_start[img + 1];
    const int nU = r.off[CIDER_ORDERS];
    const double two_sigma2 = 2.0 * sigma * sigma;
    const int tf = t < nU ? (int)r.part[t] : 0;          // the candidate's own count, before the loop overwrites r.part
    int maxref = 0;
    for (int ref = r0; ref < r1; ++ref) {                 // the image's references in index order
        const uint64_t* rk = rec_keys + (int64_t)ref * stride;
        const int n_ref = rec_off[ref * (CIDER_ORDERS + 1) + CIDER_ORDERS];
        if (t < nU) {
            const int i = find_key(rk, n_ref, r.key[t]);
            if (i < n_ref) maxref = max(maxref, rec_cnt[(int64_t)ref * stride + i]);
            if (with_cider) {                             // min(w_h, w_r) * w_r; w_r = 0 where the reference lacks the n-gram
                const double wr = i < n_ref ? rec_w[(int64_t)ref * stride + i] : 0.0;
                r.part[t] = fmin(r.w[t], wr) * wr;
            }
        }
        if (with_cider) {
            __syncthreads();
            if (t < CIDER_ORDERS) acc[t] += cider_term<NT>(r, t, rec_meta + ref * (CIDER_ORDERS + 1), two_sigma2);
            __syncthreads();
        }
    }
    clipped[t] = min(tf, maxref);
    __syncthreads();
    if (t == 0) {
        const int T = r.T;
        int correct[CIDER_ORDERS], guess[CIDER_ORDERS];
        for (int k = 0; k < CIDER_ORDERS; ++k) {
            int c = 0;
            for (int q = r.off[k]; q < r.off[k + 1]; ++q) c += clipped[q];
            correct[k] = c;
            guess[k] = max(0, T - k);
        }
        int reflen = 0, best = -1;                        // the closest reference length; a tie goes to the shorter one
        for (int ref = r0; ref < r1; ++ref) {
            const int l = rec_len[ref], d = abs(l - T);
            if (best < 0 || d < best || (d == best && l < reflen)) { best = d; reflen = l; }
        }
        const double tiny = 1e-15, small = 1e-9;
        double b = 1.0, bleu = 0.0;
        for (int k = 0; k < CIDER_ORDERS; ++k) {
            b *= ((double)correct[k] + tiny) / ((double)guess[k] + small);
            bleu = pow(b, 1.0 / (double)(k + 1));
        }
        const double ratio = ((double)T + tiny) / ((double)reflen + small);
        if (ratio < 1.0) bleu *= exp(1.0 - 1.0 / ratio);
        double s = 0.0;
        if (with_cider) s = cider_value(acc, r1 - r0) * cider_weight;     // bofi_cider_score's operations when bleu_weight is 0
        if (bleu_weight != 0.0) s += bleu_weight * bleu;
        if (r.bad) s = __builtin_nan("");                 // an id outside [0, 65534] has no key: the score says so
        out[j] = (float)s;
        if (out64) out64[j] = s;
        if (comps) {
            int* c = comps + (int64_t)j * (2 + 2 * CIDER_ORDERS);
            c[0] = T;
            c[1] = reflen;
            for (int k = 0; k < CIDER_ORDERS; ++k) {
                c[2 + k] = guess[k];
                c[2 + CIDER_ORDERS + k] = correct[k];
            }
        }
    }
}

}  // namespace

extern "C" int bofi_cider_refs(const int* ref_tok, const int* ref_len, int n_refs, int width, const uint64_t* df_keys, const double* df_vals,
                               int n_df, double log_ref_len, uint64_t* rec_keys, double* rec_w, int* rec_off, double* rec_meta, int stride,
                               void* stream) {
    return bofi_reward_refs(ref_tok, ref_len, n_refs, width, df_keys, df_vals, n_df, log_ref_len, rec_keys, rec_w, rec_off, rec_meta, nullptr,
                            nullptr, stride, stream);
}

extern "C" int bofi_reward_refs(const int* ref_tok, const int* ref_len, int n_refs, int width, const uint64_t* df_keys, const double* df_vals,
                                int n_df, double log_ref_len, uint64_t* rec_keys, double* rec_w, int* rec_off, double* rec_meta, int* rec_cnt,
                                int* rec_len, int stride, void* stream) {
    if (!ref_len || !rec_keys || !rec_w || !rec_off || !rec_meta || n_refs < 0 || width < 0 || width > CIDER_MAX_TOKENS || n_df < 0 ||
        (n_df > 0 && (!df_keys || !df_vals)) || (width > 0 && !ref_tok) || (stride != 128 && stride != 256) || ngram_count(width) > stride ||
        (!rec_cnt) != (!rec_len))
        return BOFI_ERR_ARG;
    if (n_refs == 0) return BOFI_OK;
    if (ngram_count(width) <= 128)
        hipLaunchKernelGGL(cider_refs_kernel<128>, dim3(n_refs), dim3(128), 0, (hipStream_t)stream, ref_tok, ref_len, width, df_keys, df_vals, n_df,
                           log_ref_len, rec_keys, rec_w, rec_off, rec_meta, rec_cnt, rec_len, stride);
    else
        hipLaunchKernelGGL(cider_refs_kernel<256>, dim3(n_refs), dim3(256), 0, (hipStream_t)stream, ref_tok, ref_len, width, df_keys, df_vals, n_df,
                           log_ref_len, rec_keys, rec_w, rec_off, rec_meta, rec_cnt, rec_len, stride);
    BOFI_CHECK_LAUNCH();
    return BOFI_OK;
}

extern "C" int bofi_cider_score(const int64_t* seq, const int* cand_len, int N, int S, int seq_per_img, const int* ref_start, const uint64_t* df_keys,
                                const double* df_vals, int n_df, double log_ref_len, double sigma, double weight, const uint64_t* rec_keys,
                                const double* rec_w, const int* rec_off, const double* rec_meta, int stride, float* out, double* out64,
                                void* stream) {
    if (!seq || !ref_start || !rec_keys || !rec_w || !rec_off || !rec_meta || !out || N < 0 || S < 1 || S > CIDER_MAX_TOKENS || seq_per_img < 1 ||
        N % seq_per_img != 0 || n_df < 0 || (n_df > 0 && (!df_keys || !df_vals)) || (stride != 128 && stride != 256) || !(sigma > 0.0))
        return BOFI_ERR_ARG;
    if (N == 0) return BOFI_OK;
    if (ngram_count(S) <= 128)
        hipLaunchKernelGGL(cider_score_kernel<128>, dim3(N), dim3(128), 0, (hipStream_t)stream, seq, cand_len, S, seq_per_img, ref_start, df_keys,
                           df_vals, n_df, log_ref_len, sigma, weight, rec_keys, rec_w, rec_off, rec_meta, stride, out, out64);
    else
        hipLaunchKernelGGL(cider_score_kernel<256>, dim3(N), dim3(256), 0, (hipStream_t)stream, seq, cand_len, S, seq_per_img, ref_start, df_keys,
                           df_vals, n_df, log_ref_len, sigma, weight, rec_keys, rec_w, rec_off, rec_meta, stride, out, out64);
    BOFI_CHECK_LAUNCH();
    return BOFI_OK;
}

extern "C" int bofi_reward_score(const int64_t* seq, const int* cand_len, int N, int S, int seq_per_img, const int* ref_start,
                                 const uint64_t* df_keys, const double* df_vals, int n_df, double log_ref_len, double sigma, double cider_weight,
                                 double bleu_weight, const uint64_t* rec_keys, const double* rec_w, const int* rec_off, const double* rec_meta,
                                 const int* rec_cnt, const int* rec_len, int stride, float* out, double* out64, int* comps, void* stream) {
    if (!seq || !ref_start || !rec_keys || !rec_w || !rec_off || !rec_meta || !rec_cnt || !rec_len || !out || N < 0 || S < 1 ||
        S > CIDER_MAX_TOKENS || seq_per_img < 1 || N % seq_per_img != 0 || n_df < 0 || (n_df > 0 && (!df_keys || !df_vals)) ||
        (stride != 128 && stride != 256) || !(sigma > 0.0) || !std::isfinite(cider_weight) || !std::isfinite(bleu_weight))
        return BOFI_ERR_ARG;
    if (N == 0) return BOFI_OK;
    if (ngram_count(S) <= 128)
        hipLaunchKernelGGL(reward_score_kernel<128>, dim3(N), dim3(128), 0, (hipStream_t)stream, seq, cand_len, S, seq_per_img, ref_start, df_keys,
                           df_vals, n_df, log_ref_len, sigma, cider_weight, bleu_weight, rec_keys, rec_w, rec_off, rec_meta, rec_cnt, rec_len,
                           stride, out, out64, comps);
    else
        hipLaunchKernelGGL(reward_score_kernel<256>, dim3(N), dim3(256), 0, (hipStream_t)stream, seq, cand_len, S, seq_per_img, ref_start, df_keys,
                           df_vals, n_df, log_ref_len, sigma, cider_weight, bleu_weight, rec_keys, rec_w, rec_off, rec_meta, rec_cnt, rec_len,
                           stride, out, out64, comps);
    BOFI_CHECK_LAUNCH();
    return BOFI_OK;
}
