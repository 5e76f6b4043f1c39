// Diversity of the n sampled captions of one image on the device: self-CIDEr (get_self_cider_scores, captioning/utils/rewards.py:119-139),
// and the counts behind Div-1 / Div-2 and mBLEU-1..4 (the div_stats of the reference's evaluation, eval_utils.py:105-120).
//
// One workgroup per image.  Each of its n samples (n <= 16) becomes the record of bofi_record.h; keys, weights and counts go to the image's
// slice of a caller-provided workspace, offsets, norms and token counts stay in LDS.  Then, for every sample i, one binary search per unique
// n-gram and other sample j serves all three families:
//   * M[i][j] = 1/4 * sum over the orders k of cos_k(i, j), plain CIDEr (no clipping, no length penalty), computed once per pair i <= j and
//     mirrored, so M is exactly symmetric; per-order sums run in index order, so it is bit-identical run to run;
//   * Div-n numerators: the n-grams of order <= 2 that no earlier sample of the image holds (integer sums);
//   * mBLEU counts: min(count_i, max over j != i of count_j) per n-gram, and the closest T_j (a tie goes to the shorter).
// The eigenvalues of M come from a cyclic Jacobi iteration in fp64 by one thread: rotations in the fixed order (p, q), p < q, until the
// off-diagonal is exactly 0 or JACOBI_SWEEPS sweeps are through.  score = -log(sqrt(l_max) / sum sqrt(l)) / log n over the eigenvalues clipped
// below at 0.  Every loop is bounded by n, T, the block size or JACOBI_SWEEPS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "bofi_common.h"
#include "bofi_record.h"
#include "boficap_hip.h"

namespace {

constexpr int DIV_MAX_SAMPLES = 16;
constexpr int JACOBI_SWEEPS = 50;
constexpr int DIV_COMPS = 2 + 2 * CIDER_ORDERS;

// sample j's token list into r.tok under the 'eval' rule (decode_sequence): the ids before the first id <= 0, else the whole row; r.bad if an
// id lies above 65534 (its tokens are then read as 0)
template <int NT>
__device__ inline void load_eval_sample(RecordLds<NT>& r, const int64_t* row, int S) {
    const int t = threadIdx.x;
    if (t == 0) {
        int T = S, bad = 0;
        for (int q = 0; q < S; ++q)
            if (row[q] <= 0) { T = q; break; }
        for (int q = 0; q < T; ++q) bad |= row[q] > CIDER_MAX_ID;
        r.T = T;
        r.bad = bad;
    }
    __syncthreads();
    if (t < r.T) r.tok[t] = r.bad ? 0 : (int)row[t];
    __syncthreads();
}

// Eigenvalues of the symmetric n x n matrix a (row stride DIV_MAX_SAMPLES, overwritten) by cyclic Jacobi rotations, left on its diagonal.
// One thread.  A rotation sets a[p][q] to exactly 0; an element too small to change either of its diagonal neighbours is set to 0 after the
// third sweep, so the iteration ends on an off-diagonal of exactly 0 (or at the cap).
__device__ inline void jacobi_eigenvalues(double* a, int n) {
    constexpr int LD = DIV_MAX_SAMPLES;
    for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) off += fabs(a[p * LD + q]);
        if (off == 0.0) return;
        for (int p = 0; p < n - 1; ++p) {
            for (int q = p + 1; q < n; ++q) {
                const double apq = a[p * LD + q];
                if (apq == 0.0) continue;
                const double app = a[p * LD + p], aqq = a[q * LD + q];
                const double g = 100.0 * fabs(apq);
                if (sweep > 2 && fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) {
                    a[p * LD + q] = 0.0;
                    a[q * LD + p] = 0.0;
                    continue;
                }
                const double h = aqq - app;
                double tn;                                 // tan of the rotation angle, the smaller root
                if (fabs(h) + g == fabs(h)) {
                    tn = apq / h;
                } else {
                    const double theta = 0.5 * h / apq;
                    tn = 1.0 / (fabs(theta) + sqrt(1.0 + theta * theta));
                    if (theta < 0.0) tn = -tn;
                }
                const double c = 1.0 / sqrt(1.0 + tn * tn), s = tn * c;
                for (int k = 0; k < n; ++k) {             // columns p and q of every other row, mirrored into rows p and q
                    if (k == p || k == q) continue;
                    const double akp = a[k * LD + p], akq = a[k * LD + q];
                    const double np_ = c * akp - s * akq, nq_ = s * akp + c * akq;
                    a[k * LD + p] = np_;
                    a[p * LD + k] = np_;
                    a[k * LD + q] = nq_;
                    a[q * LD + k] = nq_;
                }
                a[p * LD + p] = app - tn * apq;
                a[q * LD + q] = aqq + tn * apq;
                a[p * LD + q] = 0.0;
                a[q * LD + p] = 0.0;
            }
        }
    }
}

// workspace of image img: keys [n, NT] uint64, then weights [n, NT] double, then counts [n, NT] int32, each for all the images
template <int NT>
__global__ void __launch_bounds__(NT) diversity_kernel(const int64_t* seq, int n, int S, int eval_rule, const uint64_t* df_keys,
                                                       const double* df_vals, int n_df, double L, uint64_t* ws_keys, double* ws_w, int* ws_cnt,
                                                       double* score, double* mat, int* div, int* comps) {
    __shared__ RecordLds<NT> r;
    __shared__ int s_off[DIV_MAX_SAMPLES][CIDER_ORDERS + 1];
    __shared__ double s_norm[DIV_MAX_SAMPLES][CIDER_ORDERS];
    __shared__ int s_T[DIV_MAX_SAMPLES];
    __shared__ double s_cos[CIDER_ORDERS];
    __shared__ double s_M[DIV_MAX_SAMPLES * DIV_MAX_SAMPLES];
    __shared__ int s_clip[NT];
    __shared__ int s_new[NT];
    __shared__ int s_div[2];
    __shared__ int s_bad;
    const int img = blockIdx.x, t = threadIdx.x;
    const int64_t base = (int64_t)img * n;                // first sample row of this image
    if (t < 2) s_div[t] = 0;
    if (t == 0) s_bad = 0;
    __syncthreads();

    // ---- the n records
    for (int i = 0; i < n; ++i) {
        const int64_t* row = seq + (base + i) * S;
        if (eval_rule) load_eval_sample<NT>(r, row, S);
        else load_candidate<NT>(r, row, nullptr, 0, S);
        build_record<NT>(r, df_keys, df_vals, n_df, L);
        const int nU = r.off[CIDER_ORDERS];
        const int64_t o = (base + i) * NT + t;
        ws_keys[o] = t < nU ? r.key[t] : KEY_NONE;
        ws_w[o] = t < nU ? r.w[t] : 0.0;
        ws_cnt[o] = t < nU ? (int)r.part[t] : 0;          // build_record leaves the tf in r.part
        if (t <= CIDER_ORDERS) s_off[i][t] = r.off[t];
        if (t < CIDER_ORDERS) s_norm[i][t] = r.norm[t];
        if (t == 0) {
            s_T[i] = r.T;
            if (r.bad) s_bad = 1;
        }
        __syncthreads();                                  // the record is stored (workspace and LDS) before r is reused
    }

    // ---- every sample against the others
    for (int i = 0; i < n; ++i) {
        const int nU = s_off[i][CIDER_ORDERS];
        const uint64_t key = ws_keys[(base + i) * NT + t];
        const double w = ws_w[(base + i) * NT + t];
        const int tf = ws_cnt[(base + i) * NT + t];
        int maxref = 0, seen = 0;
        for (int j = 0; j < n; ++j) {
            const int nJ = s_off[j][CIDER_ORDERS];
            int idx = nJ;
            if (t < nU) idx = find_key(ws_keys + (base + j) * NT, nJ, key);
            const bool found = t < nU && idx < nJ;
            if (j != i && found) maxref = max(maxref, ws_cnt[(base + j) * NT + idx]);
            if (j < i && found) seen = 1;
            if (j >= i) {                                 // block-uniform: M once per pair i <= j
                r.part[t] = found ? w * ws_w[(base + j) * NT + idx] : 0.0;
                __syncthreads();
                if (t < CIDER_ORDERS) {
                    double val = 0.0;
                    for (int q = s_off[i][t]; q < s_off[i][t + 1]; ++q) val += r.part[q];
                    const double ni = s_norm[i][t], nj = s_norm[j][t];
                    s_cos[t] = ni != 0.0 && nj != 0.0 ? val / (ni * nj) : 0.0;
                }
                __syncthreads();
                if (t == 0) {
                    const double m = (s_cos[0] + s_cos[1] + s_cos[2] + s_cos[3]) / (double)CIDER_ORDERS;
                    s_M[i * DIV_MAX_SAMPLES + j] = m;
                    s_M[j * DIV_MAX_SAMPLES + i] = m;
                }
            }
        }
        s_clip[t] = t < nU ? min(tf, maxref) : 0;
        s_new[t] = t < s_off[i][2] && !seen ? 1 : 0;      // an n-gram of order <= 2 that no earlier sample holds
        __syncthreads();
        if (t == 0 && comps) {
            const int T = s_T[i];
            int* c = comps + (base + i) * DIV_COMPS;
            int reflen = 0, best = -1;                    // the closest other sample's length; a tie goes to the shorter one
            for (int j = 0; j < n; ++j) {
                if (j == i) continue;
                const int l = s_T[j], d = abs(l - T);
                if (best < 0 || d < best || (d == best && l < reflen)) { best = d; reflen = l; }
            }
            c[0] = T;
            c[1] = reflen;
            for (int k = 0; k < CIDER_ORDERS; ++k) {
                int cor = 0;
                for (int q = s_off[i][k]; q < s_off[i][k + 1]; ++q) cor += s_clip[q];
                c[2 + k] = max(0, T - k);
                c[2 + CIDER_ORDERS + k] = cor;
            }
        }
        if (t == 1 || t == 2) {                           // distinct unigrams (t = 1) and bigrams (t = 2) that sample i adds
            int c = 0;
            for (int q = s_off[i][t - 1]; q < s_off[i][t]; ++q) c += s_new[q];
            s_div[t - 1] += c;
        }
        __syncthreads();
    }

    // ---- outputs
    const bool bad = s_bad != 0;                          // an id outside [0, 65534] has no key: the score says so
    if (mat)
        for (int q = t; q < n * n; q += NT)
            mat[(int64_t)img * n * n + q] = bad ? __builtin_nan("") : s_M[(q / n) * DIV_MAX_SAMPLES + q % n];
    if (t == 1) {
        int tokens = 0;
        for (int i = 0; i < n; ++i) tokens += s_T[i];
        div[img * 3 + 0] = s_div[0];
        div[img * 3 + 1] = s_div[1];
        div[img * 3 + 2] = tokens;
    }
    __syncthreads();                                      // mat has read s_M before the rotations overwrite it
    if (t == 0) {
        jacobi_eigenvalues(s_M, n);
        double top = 0.0, sum = 0.0;
        for (int i = 0; i < n; ++i) {
            const double l = fmax(s_M[i * DIV_MAX_SAMPLES + i], 0.0);
            top = fmax(top, l);
            sum += sqrt(l);
        }
        const double s = -log(sqrt(top) / sum) / log((double)n);       // 0 / 0 = NaN where every eigenvalue clips to 0
        score[img] = bad ? __builtin_nan("") : s;
    }
}

}  // namespace

extern "C" int64_t bofi_diversity_workspace(int images, int n, int S) {
    if (images < 0 || n < 2 || n > DIV_MAX_SAMPLES || S < 1 || S > CIDER_MAX_TOKENS) return -1;
    const int64_t stride = ngram_count(S) <= 128 ? 128 : 256;
    return (int64_t)images * n * stride * (int64_t)(sizeof(uint64_t) + sizeof(double) + sizeof(int));
}

extern "C" int bofi_diversity_score(const int64_t* seq, int images, int n, int S, int eval_rule, const uint64_t* df_keys, const double* df_vals,
                                    int n_df, double log_ref_len, void* workspace, int64_t workspace_bytes, double* score, double* mat, int* div,
                                    int* comps, void* stream) {
    const int64_t need = bofi_diversity_workspace(images, n, S);
    if (!seq || !score || !div || need < 0 || n_df < 0 || (n_df > 0 && (!df_keys || !df_vals)) || (eval_rule != 0 && eval_rule != 1) ||
        (need > 0 && (!workspace || workspace_bytes < need)) || ((uintptr_t)workspace & 7) != 0)
        return BOFI_ERR_ARG;
    if (images == 0) return BOFI_OK;
    const int64_t stride = ngram_count(S) <= 128 ? 128 : 256;
    const int64_t rows = (int64_t)images * n;
    uint64_t* ws_keys = (uint64_t*)workspace;
    double* ws_w = (double*)(ws_keys + rows * stride);
    int* ws_cnt = (int*)(ws_w + rows * stride);
    if (stride == 128)
        hipLaunchKernelGGL(diversity_kernel<128>, dim3(images), dim3(128), 0, (hipStream_t)stream, seq, n, S, eval_rule, df_keys, df_vals, n_df,
                           log_ref_len, ws_keys, ws_w, ws_cnt, score, mat, div, comps);
    else
        hipLaunchKernelGGL(diversity_kernel<256>, dim3(images), dim3(256), 0, (hipStream_t)stream, seq, n, S, eval_rule, df_keys, df_vals, n_df,
                           log_ref_len, ws_keys, ws_w, ws_cnt, score, mat, div, comps);
    BOFI_CHECK_LAUNCH();
    return BOFI_OK;
}
