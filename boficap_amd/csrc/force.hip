// Required words behind the filling pass: "this caption must contain these ids", placed where they cost the least log-prob.  The positive counterpart of the constrained
// pick (constrain.hip): a pass that scores every position on its own leaves an [S, V] table of rows, and the best caption that holds all required words is an assignment
// of at most 8 words to at most 64 positions -- solved exactly, where an autoregressive model needs a constrained beam.  include/boficap_hip.h, bofi_vocab_require,
// states the rule; tests/test_required_words.py restates it in numpy (and holds that against a brute force over every placement).
//
// x [rows, ldx] float32 (log-probs or raw logits, read only), row b * S + p = position p of image b; n_b = clamp(ntok[b] + ntok_bias, 0, S) live positions; seq [rows]
// the ids standing there; words [B, K] the required ids of every image (< 0: empty; >= V, banned or a repeat of an earlier entry: skipped).
//   gain[p][j]   0 where seq[p] is word j already; else (double)x[p, f_j] - (double)x[p, seq[p]], both finite -- anything else makes p ineligible for j, as does (no_repeat,
//                f_j >= repeat_min_id) a live neighbour that holds f_j on entry
//   best[p][m]   (words placed, total gain) of positions p .. n_b - 1 with the words of mask m still to place: the options "p takes word j" (j ascending) and then "p keeps
//                its id", compared by count, then by total; the FIRST best option is choice[p][m]
//   result       the forward walk from (0, all required words) along choice
//
// One launch, no workspace: a wavefront per image, 4 images per workgroup (2 where S * 2^K needs it: the workgroup stays within 64 KB of LDS).
//   gather       lane = position reads seq and x[p, seq[p]]; then the lanes take the n_b * K (position, word) pairs -- scattered 4-byte loads, so rows need no alignment
//   recurrence   p = S - 1 .. 0, lanes over the 2^K masks; the rolling best (float64 total, byte count) and the byte-sized choice [S][2^K] live in LDS.  The loop is
//                uniform over the workgroup (a wavefront past its n_b only meets the barrier), so the barrier between two positions is a plain __syncthreads()
//   walk         lane 0 follows choice and writes seq, row_chosen, pos and moved
// No atomics.  The only float arithmetic is the float64 difference of the gain and the float64 sum gain + total, in the order stated: no product, so nothing contracts.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>

#include "bofi_common.h"
#include "bofi_kernels.h"
#include "boficap_hip.h"

namespace {

using namespace bofi;

constexpr int VR_MAX_S = 64;
constexpr int VR_MAX_K = BOFI_REQUIRE_MAX;
constexpr int VR_KEEP = 255;                   // choice: the position keeps its id
constexpr int VR_IPW = 4;                      // images (wavefronts) per workgroup, at most
constexpr size_t VR_LDS_MAX = 64 * 1024;
static_assert(VR_MAX_K == 8, "a mask of words is a byte's worth of bits; a choice is a byte");

struct VrArgs {
    const float* x; int ldx, V, S, B;
    const int* ntok; int ntok_bias;
    const int* words; int K;
    const uint32_t* ban; int no_repeat, repeat_min_id;
    int64_t* seq; float* row_chosen; int* pos; int* moved;
    int per_image;                              // LDS bytes of one image (vr_lds_bytes)
};

// LDS of one image, in this order (8-byte items first):
// tot [2][M] double, gain [S][K] double, xf [S][K] float, bvf [S] float, sq [S] int, cnt [2][M] byte, elig [S][K] byte, choice [S][M] byte
inline size_t vr_lds_bytes(int S, int K) {
    const size_t M = (size_t)1 << K, SK = (size_t)S * K;
    const size_t n = 2 * M * 8 + SK * 8 + SK * 4 + (size_t)S * 4 + (size_t)S * 4 + 2 * M + SK + (size_t)S * M;
    return (n + 7) & ~(size_t)7;
}

// grid = ceil(B / waves) workgroups of `waves` wavefronts: wavefront = image
__global__ void __launch_bounds__(VR_IPW * WAVE) vocab_require_kernel(VrArgs a) {
    extern __shared__ double vr_lds[];
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE, b = blockIdx.x * (blockDim.x / WAVE) + wave;
    const int S = a.S, K = a.K, M = 1 << K, V = a.V;
    const bool on = b < a.B;                                    // (a wavefront past B stays for the barriers and touches no global memory)
    char* const base = reinterpret_cast<char*>(vr_lds) + (size_t)wave * a.per_image;
    double* const tot = reinterpret_cast<double*>(base);       // [2][M]
    double* const gain = tot + 2 * M;                           // [S][K]
    float* const xf = reinterpret_cast<float*>(gain + S * K);  // [S][K]  x[p, f_j]
    float* const bvf = xf + S * K;                              // [S]     x[p, seq[p]]
    int* const sq = reinterpret_cast<int*>(bvf + S);           // [S]     seq[p] on entry; -1: an id outside 0..V-1 stands there
    uint8_t* const cnt = reinterpret_cast<uint8_t*>(sq + S);   // [2][M]
    uint8_t* const elig = cnt + 2 * M;                          // [S][K]
    uint8_t* const choice = elig + S * K;                       // [S][M]

    const int n = on ? live_count(a.ntok, a.ntok_bias, b, S) : 0;
    const size_t row0 = (size_t)(on ? b : 0) * S;
    const int* const wrow = a.words + (size_t)(on ? b : 0) * K;
    // the image's word row, classified (every lane alike): f[j] >= 0 a required word, -1 empty, -2 skipped
    int f[VR_MAX_K];
#pragma unroll
    for (int j = 0; j < VR_MAX_K; ++j) {
        int c = -1;
        if (on && j < K) {
            const int w = wrow[j];
            if (w >= V) c = -2;
            else if (w >= 0) {
                c = w;
                if (a.ban && ((a.ban[w >> 5] >> (w & 31)) & 1u)) c = -2;
                for (int i = 0; i < j; ++i)
                    if (wrow[i] == w) c = -2;
            }
        }
        f[j] = c;
    }
    // gather: the ids on entry and their values ...
    if (lane < n) {
        const int64_t id = a.seq[row0 + lane];
        const bool in = id >= 0 && id < (int64_t)V;
        sq[lane] = in ? (int)id : -1;
        bvf[lane] = in ? a.x[(row0 + lane) * (size_t)a.ldx + (size_t)id] : NAN;
    }
    __syncthreads();
    // ... then the (position, word) pairs
    for (int i = lane; i < n * K; i += WAVE) {
        const int p = i / K, j = i - p * K;
        int fj = -1;
#pragma unroll
        for (int t = 0; t < VR_MAX_K; ++t) fj = t == j ? f[t] : fj;
        double g = 0.0;
        float xv = 0.f;
        bool ok = false;
        if (fj >= 0) {
            xv = a.x[(row0 + p) * (size_t)a.ldx + (size_t)fj];
            const int here = sq[p];
            if (here == fj) ok = true;
            else {
                const float bv = bvf[p];
                if (f32_finite(xv) && f32_finite(bv)) { g = (double)xv - (double)bv; ok = true; }
                if (a.no_repeat && fj >= a.repeat_min_id && ((p > 0 && sq[p - 1] == fj) || (p + 1 < n && sq[p + 1] == fj))) ok = false;
            }
        }
        xf[i] = xv; gain[i] = g; elig[i] = ok ? 1 : 0;
    }
    for (int m = lane; m < M; m += WAVE) { tot[(n & 1) * M + m] = 0.0; cnt[(n & 1) * M + m] = 0; }      // best[n_b][.] = (0 words, 0.0)
    __syncthreads();
    // the recurrence, backwards; buffer p & 1 holds best[p][.]
    for (int p = S - 1; p >= 0; --p) {
        if (p < n) {
            const double* const tn = tot + ((p + 1) & 1) * M;
            const uint8_t* const cn = cnt + ((p + 1) & 1) * M;
            for (int m = lane; m < M; m += WAVE) {
                int bc = -1, bj = VR_KEEP;
                double bt = 0.0;
                for (int j = 0; j < K; ++j) {
                    if (!((m >> j) & 1) || !elig[p * K + j]) continue;
                    const int m2 = m ^ (1 << j);
                    const int c = 1 + (int)cn[m2];
                    const double t = gain[p * K + j] + tn[m2];
                    if (c > bc || (c == bc && t > bt)) { bc = c; bt = t; bj = j; }
                }
                {
                    const int c = (int)cn[m];
                    const double t = tn[m];
                    if (c > bc || (c == bc && t > bt)) { bc = c; bt = t; bj = VR_KEEP; }
                }
                tot[(p & 1) * M + m] = bt; cnt[(p & 1) * M + m] = (uint8_t)bc; choice[p * M + m] = (uint8_t)bj;
            }
        }
        __syncthreads();
    }
    // the forward walk
    if (on && lane == 0) {
        int m = 0, mv = 0;
        int where[VR_MAX_K];
#pragma unroll
        for (int j = 0; j < VR_MAX_K; ++j) {
            where[j] = f[j] >= 0 ? -3 : f[j];
            if (f[j] >= 0) m |= 1 << j;
        }
        for (int p = 0; p < n && m; ++p) {
            const int c = choice[p * M + m];
            if (c == VR_KEEP) continue;
            int fc = 0;
#pragma unroll
            for (int t = 0; t < VR_MAX_K; ++t) {
                if (t == c) { fc = f[t]; where[t] = p; }
            }
            if (sq[p] != fc) { a.seq[row0 + p] = (int64_t)fc; ++mv; }
            if (a.row_chosen) a.row_chosen[row0 + p] = xf[p * K + c];
            m ^= 1 << c;
        }
#pragma unroll
        for (int j = 0; j < VR_MAX_K; ++j)
            if (j < K) a.pos[(size_t)b * K + j] = where[j];
        if (a.moved) a.moved[b] = mv;
    }
}

}  // namespace

const char* bofi::vocab_require_check(const float* x, int ldx, int rows, int V, int S, const int* words, int K, int no_repeat, int repeat_min_id, const int64_t* seq,
                                      const int* pos) {
    if (!x || !seq || !words || !pos) return "non-null x, seq, words and pos";
    if (S < 1 || S > VR_MAX_S) return "S in 1..64";
    if (rows < 0 || rows % S != 0) return "rows a multiple of S (>= 0)";
    if (V < 2) return "V >= 2";
    if (ldx < V) return "a row pitch of at least V";
    if (K < 1 || K > VR_MAX_K) return "K in 1..8 (BOFI_REQUIRE_MAX)";
    if (no_repeat != 0 && no_repeat != 1) return "no_repeat 0 or 1";
    if (repeat_min_id < 0) return "repeat_min_id >= 0";
    return nullptr;
}

int bofi::launch_vocab_require(const float* x, int ldx, int rows, int V, int S, const int* ntok, int ntok_bias, const int* words, int K, const uint32_t* ban_bits,
                               int no_repeat, int repeat_min_id, int64_t* seq, float* row_chosen, int* pos, int* moved, hipStream_t st) {
    if (vocab_require_check(x, ldx, rows, V, S, words, K, no_repeat, repeat_min_id, seq, pos)) return BOFI_ERR_ARG;
    if (rows == 0) return BOFI_OK;
    VrArgs a{};
    a.x = x; a.ldx = ldx; a.V = V; a.S = S; a.B = rows / S; a.ntok = ntok; a.ntok_bias = ntok_bias; a.words = words; a.K = K; a.ban = ban_bits;
    a.no_repeat = no_repeat; a.repeat_min_id = repeat_min_id; a.seq = seq; a.row_chosen = row_chosen; a.pos = pos; a.moved = moved;
    const size_t per = vr_lds_bytes(S, K);
    a.per_image = (int)per;
    int waves = VR_IPW;
    while (waves > 1 && waves * per > VR_LDS_MAX) waves /= 2;      // (S = 64, K = 8: 28 KB an image, two per workgroup)
    hipLaunchKernelGGL(vocab_require_kernel, dim3((a.B + waves - 1) / waves), dim3(waves * WAVE), waves * per, st, a);
    BOFI_CHECK_LAUNCH();
    return BOFI_OK;
}

extern "C" int bofi_vocab_require(const float* x, int ldx, int rows, int V, int S, const int* ntok, int ntok_bias, const int* words, int K, const uint32_t* ban_bits,
                                  int no_repeat, int repeat_min_id, int64_t* seq, float* row_chosen, int* pos, int* moved, void* stream) {
    if (const char* why = bofi::vocab_require_check(x, ldx, rows, V, S, words, K, no_repeat, repeat_min_id, seq, pos))
        return bofi::fail(BOFI_ERR_ARG, std::string("vocab_require: ") + why);
    return bofi::launch_vocab_require(x, ldx, rows, V, S, ntok, ntok_bias, words, K, ban_bits, no_repeat, repeat_min_id, seq, row_chosen, pos, moved, (hipStream_t)stream);
}
