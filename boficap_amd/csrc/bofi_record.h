// The caption record of the token-level scorers (cider.hip, diversity.hip): a row's unique n-grams (n = 1..4) as sorted 64-bit keys, their
// weights tf * (L - log(max(1, df))), raw counts, the four per-order norms and the row's "length" (its number of bigrams), built by one
// workgroup in LDS.  An n-gram's key packs (id + 1) into 16-bit fields, first token in the highest used field, so keys are exact, and the
// keys of order k lie in [2^(16(k-1)), 2^(16k)): a sorted record is grouped by order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int CIDER_ORDERS = 4;
constexpr int CIDER_MAX_TOKENS = 64;          // 4 * 64 - 6 = 250 n-grams: fits a 256-thread record
constexpr int CIDER_MAX_ID = 65534;           // (id + 1) must fit a 16-bit field
constexpr uint64_t KEY_NONE = ~0ull;

__host__ __device__ inline int ngram_count(int T) {
    int c = 0;
    for (int k = 1; k <= CIDER_ORDERS; ++k) c += T >= k ? T - k + 1 : 0;
    return c;
}

// L - log(max(1, df(key))) from the sorted df table; an n-gram absent from it has df 0, i.e. the value L
__device__ inline double df_value(uint64_t key, const uint64_t* df_keys, const double* df_vals, int n_df, double L) {
    int lo = 0, hi = n_df;
    while (lo < hi) {
        int mid = (lo + hi) >> 1;
        if (df_keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo < n_df && df_keys[lo] == key ? df_vals[lo] : L;
}

// index of key in the sorted keys rk [0, n), or n if absent
__device__ inline int find_key(const uint64_t* rk, int n, uint64_t key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        int mid = (lo + hi) >> 1;
        if (rk[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo < n && rk[lo] == key ? lo : n;
}

template <int NT>
struct RecordLds {
    uint64_t key[NT];
    double w[NT];                 // tf on the way, then the weight
    double part[NT];              // per-n-gram terms of a similarity
    int scan[NT];
    int tok[CIDER_MAX_TOKENS];
    int off[CIDER_ORDERS + 1];    // first unique n-gram of each order; off[4] = number of unique n-grams
    double norm[CIDER_ORDERS];
    double length;
    int T;
    int bad;
};

// The record of the T tokens in r.tok (T set, tokens loaded, both visible to the block): sorted unique keys and their weights in
// r.key / r.w [0, r.off[4]), norms and length.  Every loop is bounded by T or NT.
template <int NT>
__device__ void build_record(RecordLds<NT>& r, const uint64_t* df_keys, const double* df_vals, int n_df, double L) {
    const int t = threadIdx.x;
    const int T = r.T;
    const int nG = ngram_count(T);
    uint64_t key = KEY_NONE;
    if (t < nG) {                                         // n-gram t: order k at position p
        int i = t, k = 1;
        while (k < CIDER_ORDERS && i >= T - k + 1) { i -= T - k + 1; ++k; }
        key = 0;
        for (int q = 0; q < k; ++q) key = (key << 16) | (uint64_t)(r.tok[i + q] + 1);
    }
    r.key[t] = key;
    __syncthreads();
    for (int k = 2; k <= NT; k <<= 1) {                   // bitonic sort, one key per thread
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int o = t ^ j;
            if (o > t) {
                const uint64_t a = r.key[t], b = r.key[o];
                if ((a > b) == ((t & k) == 0)) { r.key[t] = b; r.key[o] = a; }
            }
            __syncthreads();
        }
    }
    key = r.key[t];
    const bool head = t < nG && (t == 0 || r.key[t - 1] != key);
    int tf = 0;
    if (head)
        for (int q = t; q < nG && r.key[q] == key; ++q) ++tf;
    r.scan[t] = head ? 1 : 0;
    __syncthreads();
    for (int d = 1; d < NT; d <<= 1) {                    // inclusive scan of the head flags
        const int v = t >= d ? r.scan[t - d] : 0;
        __syncthreads();
        r.scan[t] += v;
        __syncthreads();
    }
    const int nU = r.scan[NT - 1];
    const int u = r.scan[t] - 1;
    __syncthreads();                                      // every thread has read its key before the compaction overwrites them
    if (head) {
        r.key[u] = key;
        r.w[u] = (double)tf * df_value(key, df_keys, df_vals, n_df, L);
        r.part[u] = (double)tf;
    }
    __syncthreads();
    if (t < CIDER_ORDERS) {                               // first unique n-gram of order t + 1 (keys are grouped by order)
        const uint64_t lo = t == 0 ? 0ull : 1ull << (16 * t);
        int q = 0;
        while (q < nU && r.key[q] < lo) ++q;
        r.off[t] = q;
    }
    if (t == CIDER_ORDERS) r.off[t] = nU;
    __syncthreads();
    if (t < CIDER_ORDERS) {
        double s = 0.0;
        for (int q = r.off[t]; q < r.off[t + 1]; ++q) s += r.w[q] * r.w[q];
        r.norm[t] = sqrt(s);
    }
    if (t == CIDER_ORDERS) {
        double len = 0.0;
        for (int q = r.off[1]; q < r.off[2]; ++q) len += r.part[q];
        r.length = len;
    }
    __syncthreads();
}

// candidate j's token list into r.tok: up to and including the first 0, else the whole row (or cand_len[j] tokens); r.bad if an id
// lies outside [0, 65534] (its tokens are then read as 0)
template <int NT>
__device__ inline void load_candidate(RecordLds<NT>& r, const int64_t* row, const int* cand_len, int j, int S) {
    const int t = threadIdx.x;
    if (t == 0) {
        int T = S, bad = 0;
        if (cand_len) {
            T = min(max(cand_len[j], 0), S);
        } else {
            for (int q = 0; q < S; ++q)
                if (row[q] == 0) { T = q + 1; break; }
        }
        for (int q = 0; q < T; ++q) bad |= row[q] < 0 || row[q] > CIDER_MAX_ID;
        r.T = T;
        r.bad = bad;
    }
    __syncthreads();
    if (t < r.T) r.tok[t] = r.bad ? 0 : (int)row[t];
    __syncthreads();
}

}  // namespace
