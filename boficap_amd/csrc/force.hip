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

// ---- required PHRASES: units of up to 4 ids placed side by side (include/boficap_hip.h, bofi_vocab_require_units, states the rule; tests/test_required_phrases.py restates
// it in numpy).  The same shape as above -- a wavefront per image, lanes over the 2^K masks, the state in LDS, float64 totals, a uniform position loop -- with a unit
// covering a span:
//   classify     the lanes load the image's [K][L] table into LDS, lane 0 classifies it in order (a unit is skipped against EARLIER units): ln[j] = its length, -1, -2
//   gather       lane = position reads seq and x[p, seq[p]]; the lanes take the n_b * K * L (position q, unit j, index i) triples, xq[q][j][i] = x[q, u_i] -- scattered
//                4-byte loads; then the n_b * K (start p, unit j) pairs sum their span's terms left to right in float64 and settle its eligibility
//   recurrence   p = S - 1 .. 0; best[p][.] lives in buffer p mod (L + 1) of L + 1 rolling ones: "p takes unit j" reads best[p + len_j][.], "p keeps" best[p + 1][.]
//   walk         lane 0 follows choice, advancing by len_j over a placed span, and writes seq, row_chosen, pos and moved
namespace {

using namespace bofi;

constexpr int VU_MAX_L = BOFI_REQUIRE_UNIT_MAX;
static_assert(VU_MAX_L == 4, "the LDS of one image at S = 64, K = 8 is sized for spans of up to 4");

struct VuArgs {
    const float* x; int ldx, V, S, B;
    const int* ntok; int ntok_bias;
    const int* units; int K, L;
    const uint32_t* ban; int no_repeat, repeat_min_id;
    int64_t* seq; float* row_chosen; int* pos; int* moved;
    int per_image;                              // LDS bytes of one image (vu_lds_bytes)
};

// LDS of one image, in this order (8-byte items first), D = L + 1:
// tot [D][M] double, gain [S][K] double, xq [S][K][L] float, bvf [S] float, sq [S] int, ut [K][L] int, ln [K] int, cnt [D][M] byte, elig [S][K] byte, choice [S][M] byte
// (S = 64, K = 8, L = 4: 10240 + 4096 + 8192 + 256 + 256 + 128 + 32 + 1280 + 512 + 16384 = 41376 bytes: one image per workgroup)
inline size_t vu_lds_bytes(int S, int K, int L) {
    const size_t M = (size_t)1 << K, SK = (size_t)S * K, D = (size_t)L + 1;
    const size_t n = D * M * 8 + SK * 8 + SK * L * 4 + (size_t)S * 4 + (size_t)S * 4 + (size_t)K * L * 4 + (size_t)K * 4 + D * M + SK + (size_t)S * M;
    return (n + 7) & ~(size_t)7;
}

// grid = ceil(B / waves) workgroups of `waves` wavefronts: wavefront = image
__global__ void __launch_bounds__(VR_IPW * WAVE) vocab_require_units_kernel(VuArgs a) {
    extern __shared__ double vu_lds[];
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE, b = blockIdx.x * (blockDim.x / WAVE) + wave;
    const int S = a.S, K = a.K, L = a.L, D = L + 1, M = 1 << K, V = a.V;
    const bool on = b < a.B;                                    // (a wavefront past B stays for the barriers and touches no global memory)
    char* const base = reinterpret_cast<char*>(vu_lds) + (size_t)wave * a.per_image;
    double* const tot = reinterpret_cast<double*>(base);       // [D][M]
    double* const gain = tot + D * M;                           // [S][K]     span gain of "unit j starts at p"
    float* const xq = reinterpret_cast<float*>(gain + S * K);  // [S][K][L]  x[q, u_i of unit j]
    float* const bvf = xq + S * K * L;                          // [S]        x[p, seq[p]]
    int* const sq = reinterpret_cast<int*>(bvf + S);           // [S]        seq[p] on entry; -1: an id outside 0..V-1 stands there
    int* const ut = sq + S;                                     // [K][L]     the image's table as given
    int* const ln = ut + K * L;                                 // [K]        len_j of a kept unit, -1 empty, -2 skipped
    uint8_t* const cnt = reinterpret_cast<uint8_t*>(ln + K);   // [D][M]
    uint8_t* const elig = cnt + D * M;                          // [S][K]
    uint8_t* const choice = elig + S * K;                       // [S][M]

    const int n = on ? live_count(a.ntok, a.ntok_bias, b, S) : 0;
    const size_t row0 = (size_t)(on ? b : 0) * S;
    // the image's table, classified by lane 0
    for (int t = lane; t < K * L; t += WAVE) ut[t] = on ? a.units[(size_t)b * K * L + t] : -1;
    __syncthreads();
    if (lane == 0) {
        for (int j = 0; j < K; ++j) {
            const int* const u = ut + j * L;
            int len = 0;
            while (len < L && u[len] >= 0) ++len;
            int c = len ? len : -1;
            for (int i = 0; i < len; ++i) {
                const int w = u[i];
                if (w >= V) c = -2;
                else if (a.ban && ((a.ban[w >> 5] >> (w & 31)) & 1u)) c = -2;
            }
            for (int e = 0; e < j && c > 0; ++e) {              // equal to an earlier unit, kept or not
                const int* const v = ut + e * L;
                bool same = true;
                for (int i = 0; i < L && same; ++i) {
                    const bool mine = i < len, theirs = v[i] >= 0;
                    if (mine != theirs || (mine && v[i] != u[i])) same = false;
                    if (!mine) break;                           // (both ended here)
                }
                if (same) c = -2;
            }
            if (c > 0 && a.no_repeat) {
                for (int i = 1; i < len; ++i)
                    if (u[i] == u[i - 1] && u[i] >= a.repeat_min_id) c = -2;
                for (int e = 0; e < j; ++e) {
                    if (ln[e] <= 0) continue;
                    const int* const v = ut + e * L;
                    if ((u[0] >= a.repeat_min_id && u[0] == v[ln[e] - 1]) || (u[len - 1] >= a.repeat_min_id && u[len - 1] == v[0])) c = -2;
                }
            }
            ln[j] = c;
        }
    }
    // gather: the ids on entry and their values ...
    if (lane < n) {
        const int64_t id = a.seq[row0 + lane];
        const bool in = id >= 0 && id < (int64_t)V;
        sq[lane] = in ? (int)id : -1;
        bvf[lane] = in ? a.x[(row0 + lane) * (size_t)a.ldx + (size_t)id] : NAN;
    }
    __syncthreads();
    // ... the (position, unit, index) triples ...
    const int KL = K * L;
    for (int t = lane; t < n * KL; t += WAVE) {
        const int q = t / KL, r = t - q * KL, j = r / L, i = r - j * L;
        xq[t] = i < ln[j] ? a.x[(row0 + q) * (size_t)a.ldx + (size_t)ut[r]] : 0.f;
    }
    __syncthreads();
    // ... and the spans
    for (int t = lane; t < n * K; t += WAVE) {
        const int p = t / K, j = t - p * K, len = ln[j];
        double g = 0.0;
        bool ok = len > 0 && p + len <= n;
        if (ok) {
            const int* const u = ut + j * L;
            for (int i = 0; i < len; ++i) {
                const int q = p + i;
                if (sq[q] == u[i]) continue;
                const float xv = xq[(q * K + j) * L + i], bv = bvf[q];
                if (f32_finite(xv) && f32_finite(bv)) g += (double)xv - (double)bv;
                else ok = false;
            }
            if (a.no_repeat) {
                const int u0 = u[0], ul = u[len - 1];
                if (u0 >= a.repeat_min_id && sq[p] != u0 && p > 0 && sq[p - 1] == u0) ok = false;
                if (ul >= a.repeat_min_id && sq[p + len - 1] != ul && p + len < n && sq[p + len] == ul) ok = false;
            }
        }
        gain[t] = ok ? g : 0.0; elig[t] = ok ? 1 : 0;
    }
    for (int m = lane; m < M; m += WAVE) { tot[(n % D) * M + m] = 0.0; cnt[(n % D) * M + m] = 0; }      // best[n_b][.] = (0 units, 0.0)
    __syncthreads();
    // the recurrence, backwards; buffer p mod D holds best[p][.]
    for (int p = S - 1; p >= 0; --p) {
        if (p < n) {
            const int pm = p % D, nx = pm + 1 == D ? 0 : pm + 1;
            for (int m = lane; m < M; m += WAVE) {
                int bc = -1, bj = VR_KEEP;
                double bt = 0.0;
                for (int j = 0; j < K; ++j) {
                    if (!((m >> j) & 1) || !elig[p * K + j]) continue;
                    int s = pm + ln[j];                         // best[p + len_j]: an eligible span ends at or before n_b, and len_j <= L < D
                    if (s >= D) s -= D;
                    const int m2 = m ^ (1 << j);
                    const int c = 1 + (int)cnt[s * M + m2];
                    const double t = gain[p * K + j] + tot[s * M + m2];
                    if (c > bc || (c == bc && t > bt)) { bc = c; bt = t; bj = j; }
                }
                {
                    const int c = (int)cnt[nx * M + m];
                    const double t = tot[nx * M + m];
                    if (c > bc || (c == bc && t > bt)) { bc = c; bt = t; bj = VR_KEEP; }
                }
                tot[pm * M + m] = bt; cnt[pm * M + m] = (uint8_t)bc; choice[p * M + m] = (uint8_t)bj;
            }
        }
        __syncthreads();
    }
    // the forward walk
    if (on && lane == 0) {
        int m = 0, mv = 0;
        int* const where = a.pos + (size_t)b * K;
        for (int j = 0; j < K; ++j) {
            where[j] = ln[j] > 0 ? -3 : ln[j];
            if (ln[j] > 0) m |= 1 << j;
        }
        for (int p = 0; p < n && m;) {
            const int c = choice[p * M + m];
            if (c == VR_KEEP) { ++p; continue; }
            const int len = ln[c];
            where[c] = p;
            for (int i = 0; i < len; ++i) {
                const int q = p + i, id = ut[c * L + i];
                if (sq[q] != id) { a.seq[row0 + q] = (int64_t)id; ++mv; }
                if (a.row_chosen) a.row_chosen[row0 + q] = xq[(q * K + c) * L + i];
            }
            m ^= 1 << c;
            p += len;
        }
        if (a.moved) a.moved[b] = mv;
    }
}

}  // namespace

const char* bofi::vocab_require_units_check(const float* x, int ldx, int rows, int V, int S, const int* units, int K, int L, int no_repeat, int repeat_min_id,
                                            const int64_t* seq, const int* pos) {
    if (!x || !seq || !units || !pos) return "non-null x, seq, units and pos";
    if (S < 1 || S > VR_MAX_S) return "S in 1..64";
    if (rows < 0 || rows % S != 0) return "rows a multiple of S (>= 0)";
    if (V < 2) return "V >= 2";
    if (ldx < V) return "a row pitch of at least V";
    if (K < 1 || K > VR_MAX_K) return "K in 1..8 (BOFI_REQUIRE_MAX)";
    if (L < 1 || L > VU_MAX_L) return "L in 1..4 (BOFI_REQUIRE_UNIT_MAX)";
    if (no_repeat != 0 && no_repeat != 1) return "no_repeat 0 or 1";
    if (repeat_min_id < 0) return "repeat_min_id >= 0";
    return nullptr;
}

int bofi::launch_vocab_require_units(const float* x, int ldx, int rows, int V, int S, const int* ntok, int ntok_bias, const int* units, int K, int L,
                                     const uint32_t* ban_bits, int no_repeat, int repeat_min_id, int64_t* seq, float* row_chosen, int* pos, int* moved, hipStream_t st) {
    if (vocab_require_units_check(x, ldx, rows, V, S, units, K, L, no_repeat, repeat_min_id, seq, pos)) return BOFI_ERR_ARG;
    if (rows == 0) return BOFI_OK;
    VuArgs a{};
    a.x = x; a.ldx = ldx; a.V = V; a.S = S; a.B = rows / S; a.ntok = ntok; a.ntok_bias = ntok_bias; a.units = units; a.K = K; a.L = L; a.ban = ban_bits;
    a.no_repeat = no_repeat; a.repeat_min_id = repeat_min_id; a.seq = seq; a.row_chosen = row_chosen; a.pos = pos; a.moved = moved;
    const size_t per = vu_lds_bytes(S, K, L);
    a.per_image = (int)per;
    int waves = VR_IPW;
    while (waves > 1 && waves * per > VR_LDS_MAX) waves /= 2;      // (S = 64, K = 8, L = 4: 40.4 KB an image, one per workgroup)
    hipLaunchKernelGGL(vocab_require_units_kernel, dim3((a.B + waves - 1) / waves), dim3(waves * WAVE), waves * per, st, a);
    BOFI_CHECK_LAUNCH();
    return BOFI_OK;
}

extern "C" int bofi_vocab_require_units(const float* x, int ldx, int rows, int V, int S, const int* ntok, int ntok_bias, const int* units, int K, int L,
                                        const uint32_t* ban_bits, int no_repeat, int repeat_min_id, int64_t* seq, float* row_chosen, int* pos, int* moved, void* stream) {
    if (const char* why = bofi::vocab_require_units_check(x, ldx, rows, V, S, units, K, L, no_repeat, repeat_min_id, seq, pos))
        return bofi::fail(BOFI_ERR_ARG, std::string("vocab_require_units: ") + why);
    return bofi::launch_vocab_require_units(x, ldx, rows, V, S, ntok, ntok_bias, units, K, L, ban_bits, no_repeat, repeat_min_id, seq, row_chosen, pos, moved,
                                            (hipStream_t)stream);
}

// ---- required ALTERNATIVES: groups of up to 4 units, any one of which satisfies the group -- "dog", "dogs" or "puppy" (include/boficap_hip.h, bofi_vocab_require_any,
// states the rule; tests/test_required_any.py restates it in numpy).  The units' recurrence with masks over GROUPS and K * A options per state: "position p takes
// alternative a of group j" clears bit j.  Slot c = j * A + a, slot order is table order.
//   LDS          the units' layout with [K] widened to [K * A] and WITHOUT xq [S][K * A][L] (32 KB at the ceiling): the span sums read x directly (each value is used
//                once), and the walk re-reads the few values it writes to row_chosen.  S = 64, K = 8, A = 4, L = 4: 46.4 KB an image, inside the 64 KB this file launches
//                with -- no raised dynamic-LDS attribute
//   workgroup    256 threads over as many images as fit (4, 2 or 1), so an image has 1, 2 or 4 wavefronts: at the ceiling (one image) the 2^8 masks are one per lane
//                instead of four per lane of one wavefront.  Every barrier is a plain __syncthreads()
//   classify     the image's threads load its [K * A][L] table into LDS, its first thread classifies the slots in order: ln[c] = its length, -1 empty, -2 skipped
//   gather       thread = position reads seq and x[p, seq[p]]; then the n_b * K * A (start p, slot c) pairs sum their span's terms left to right in float64, x read
//                in place -- scattered 4-byte loads, so rows need no alignment --, and settle its eligibility
//   recurrence   p = S - 1 .. 0, threads over the 2^K masks, L + 1 rolling buffers as for the units; options in slot order, then "p keeps its id"
//   walk         the image's first thread follows choice and writes seq, row_chosen, pos, which and moved
// With A = 1 every step is the units' step on the same values in the same order: the same bits out.
namespace {

using namespace bofi;

constexpr int VA_MAX_A = BOFI_REQUIRE_ALT_MAX;
constexpr int VA_THREADS = VR_IPW * WAVE;
static_assert(VR_MAX_K * VA_MAX_A <= 32 && VR_MAX_K * VA_MAX_A < VR_KEEP, "a choice byte holds a slot or VR_KEEP");

struct VaArgs {
    const float* x; int ldx, V, S, B;
    const int* ntok; int ntok_bias;
    const int* alts; int K, A, L;
    const uint32_t* ban; int no_repeat, repeat_min_id;
    int64_t* seq; float* row_chosen; int* pos; int* which; int* moved;
    int per_image;                              // LDS bytes of one image (va_lds_bytes)
    int tpi;                                    // threads of one image: VA_THREADS / images per workgroup
};

// LDS of one image, in this order (8-byte items first), D = L + 1, C = K * A:
// tot [D][M] double, gain [S][C] double, bvf [S] float, sq [S] int, ut [C][L] int, ln [C] int, cnt [D][M] byte, elig [S][C] byte, choice [S][M] byte
// (S = 64, K = 8, A = 4, L = 4: 10240 + 16384 + 256 + 256 + 512 + 128 + 1280 + 2048 + 16384 = 47488 bytes: one image per workgroup)
inline size_t va_lds_bytes(int S, int K, int A, int L) {
    const size_t M = (size_t)1 << K, C = (size_t)K * A, SC = (size_t)S * C, D = (size_t)L + 1;
    const size_t n = D * M * 8 + SC * 8 + (size_t)S * 4 + (size_t)S * 4 + C * L * 4 + C * 4 + D * M + SC + (size_t)S * M;
    return (n + 7) & ~(size_t)7;
}

// grid = ceil(B / ipw) workgroups of VA_THREADS threads: image = threadIdx.x / tpi, ipw = VA_THREADS / tpi images per workgroup
__global__ void __launch_bounds__(VA_THREADS) vocab_require_any_kernel(VaArgs a) {
    extern __shared__ double va_lds[];
    const int tpi = a.tpi, ti = threadIdx.x % tpi, img = threadIdx.x / tpi, b = blockIdx.x * (VA_THREADS / tpi) + img;
    const int S = a.S, K = a.K, A = a.A, C = K * A, L = a.L, D = L + 1, M = 1 << K, V = a.V;
    const bool on = b < a.B;                                    // (the threads of an image past B stay for the barriers and touch no global memory)
    char* const base = reinterpret_cast<char*>(va_lds) + (size_t)img * a.per_image;
    double* const tot = reinterpret_cast<double*>(base);       // [D][M]
    double* const gain = tot + D * M;                           // [S][C]     span gain of "slot c starts at p"
    float* const bvf = reinterpret_cast<float*>(gain + S * C); // [S]        x[p, seq[p]]
    int* const sq = reinterpret_cast<int*>(bvf + S);           // [S]        seq[p] on entry; -1: an id outside 0..V-1 stands there
    int* const ut = sq + S;                                     // [C][L]     the image's table as given
    int* const ln = ut + C * L;                                 // [C]        len_c of a kept slot, -1 empty, -2 skipped
    uint8_t* const cnt = reinterpret_cast<uint8_t*>(ln + C);   // [D][M]
    uint8_t* const elig = cnt + D * M;                          // [S][C]
    uint8_t* const choice = elig + S * C;                       // [S][M]

    const int n = on ? live_count(a.ntok, a.ntok_bias, b, S) : 0;
    const size_t row0 = (size_t)(on ? b : 0) * S;
    // the image's table, classified by its first thread
    for (int t = ti; t < C * L; t += tpi) ut[t] = on ? a.alts[(size_t)b * C * L + t] : -1;
    __syncthreads();
    if (ti == 0) {
        for (int s = 0; s < C; ++s) {
            const int* const u = ut + s * L;
            int len = 0;
            while (len < L && u[len] >= 0) ++len;
            int c = len ? len : -1;
            for (int i = 0; i < len; ++i) {
                const int w = u[i];
                if (w >= V) c = -2;
                else if (a.ban && ((a.ban[w >> 5] >> (w & 31)) & 1u)) c = -2;
            }
            for (int e = 0; e < s && c > 0; ++e) {              // equal to an earlier slot, of any group, kept or not
                const int* const v = ut + e * L;
                bool same = true;
                for (int i = 0; i < L && same; ++i) {
                    const bool mine = i < len, theirs = v[i] >= 0;
                    if (mine != theirs || (mine && v[i] != u[i])) same = false;
                    if (!mine) break;                           // (both ended here)
                }
                if (same) c = -2;
            }
            if (c > 0 && a.no_repeat) {
                for (int i = 1; i < len; ++i)
                    if (u[i] == u[i - 1] && u[i] >= a.repeat_min_id) c = -2;
                for (int e = 0; e < (s / A) * A; ++e) {         // earlier kept slots of ANOTHER group: alternatives of one group are never both placed
                    if (ln[e] <= 0) continue;
                    const int* const v = ut + e * L;
                    if ((u[0] >= a.repeat_min_id && u[0] == v[ln[e] - 1]) || (u[len - 1] >= a.repeat_min_id && u[len - 1] == v[0])) c = -2;
                }
            }
            ln[s] = c;
        }
    }
    // gather: the ids on entry and their values ...
    if (ti < n) {
        const int64_t id = a.seq[row0 + ti];
        const bool in = id >= 0 && id < (int64_t)V;
        sq[ti] = in ? (int)id : -1;
        bvf[ti] = in ? a.x[(row0 + ti) * (size_t)a.ldx + (size_t)id] : NAN;
    }
    __syncthreads();
    // ... and the spans, x read in place
    for (int t = ti; t < n * C; t += tpi) {
        const int p = t / C, s = t - p * C, len = ln[s];
        double g = 0.0;
        bool ok = len > 0 && p + len <= n;
        if (ok) {
            const int* const u = ut + s * L;
            for (int i = 0; i < len; ++i) {
                const int q = p + i;
                if (sq[q] == u[i]) continue;
                const float xv = a.x[(row0 + q) * (size_t)a.ldx + (size_t)u[i]], bv = bvf[q];
                if (f32_finite(xv) && f32_finite(bv)) g += (double)xv - (double)bv;
                else ok = false;
            }
            if (a.no_repeat) {
                const int u0 = u[0], ul = u[len - 1];
                if (u0 >= a.repeat_min_id && sq[p] != u0 && p > 0 && sq[p - 1] == u0) ok = false;
                if (ul >= a.repeat_min_id && sq[p + len - 1] != ul && p + len < n && sq[p + len] == ul) ok = false;
            }
        }
        gain[t] = ok ? g : 0.0; elig[t] = ok ? 1 : 0;
    }
    for (int m = ti; m < M; m += tpi) { tot[(n % D) * M + m] = 0.0; cnt[(n % D) * M + m] = 0; }      // best[n_b][.] = (0 groups, 0.0)
    __syncthreads();
    // the recurrence, backwards; buffer p mod D holds best[p][.]
    for (int p = S - 1; p >= 0; --p) {
        if (p < n) {
            const int pm = p % D, nx = pm + 1 == D ? 0 : pm + 1;
            for (int m = ti; m < M; m += tpi) {
                int bc = -1, bs = VR_KEEP;
                double bt = 0.0;
                for (int j = 0; j < K; ++j) {
                    if (!((m >> j) & 1)) continue;
                    const int m2 = m ^ (1 << j);
                    for (int s = j * A; s < j * A + A; ++s) {
                        if (!elig[p * C + s]) continue;
                        int r = pm + ln[s];                     // best[p + len_c]: an eligible span ends at or before n_b, and len_c <= L < D
                        if (r >= D) r -= D;
                        const int c = 1 + (int)cnt[r * M + m2];
                        const double t = gain[p * C + s] + tot[r * M + m2];
                        if (c > bc || (c == bc && t > bt)) { bc = c; bt = t; bs = s; }
                    }
                }
                {
                    const int c = (int)cnt[nx * M + m];
                    const double t = tot[nx * M + m];
                    if (c > bc || (c == bc && t > bt)) { bc = c; bt = t; bs = VR_KEEP; }
                }
                tot[pm * M + m] = bt; cnt[pm * M + m] = (uint8_t)bc; choice[p * M + m] = (uint8_t)bs;
            }
        }
        __syncthreads();
    }
    // the forward walk
    if (on && ti == 0) {
        int m = 0, mv = 0;
        int* const where = a.pos + (size_t)b * K;
        int* const alt = a.which + (size_t)b * K;
        for (int j = 0; j < K; ++j) {
            int code = -1;                                      // every slot empty
            for (int s = j * A; s < j * A + A; ++s) {
                if (ln[s] > 0) code = -3;
                else if (ln[s] == -2 && code == -1) code = -2;
            }
            where[j] = code; alt[j] = -1;
            if (code == -3) m |= 1 << j;
        }
        for (int p = 0; p < n && m;) {
            const int s = choice[p * M + m];
            if (s == VR_KEEP) { ++p; continue; }
            const int j = s / A, len = ln[s];
            where[j] = p; alt[j] = s - j * A;
            for (int i = 0; i < len; ++i) {
                const int q = p + i, id = ut[s * L + i];
                if (sq[q] != id) { a.seq[row0 + q] = (int64_t)id; ++mv; }
                if (a.row_chosen) a.row_chosen[row0 + q] = a.x[(row0 + q) * (size_t)a.ldx + (size_t)id];
            }
            m ^= 1 << j;
            p += len;
        }
        if (a.moved) a.moved[b] = mv;
    }
}

}  // namespace

const char* bofi::vocab_require_any_check(const float* x, int ldx, int rows, int V, int S, const int* alts, int K, int A, int L, int no_repeat, int repeat_min_id,
                                          const int64_t* seq, const int* pos, const int* which) {
    if (!x || !seq || !alts || !pos || !which) return "non-null x, seq, alts, pos and which";
    if (S < 1 || S > VR_MAX_S) return "S in 1..64";
    if (rows < 0 || rows % S != 0) return "rows a multiple of S (>= 0)";
    if (V < 2) return "V >= 2";
    if (ldx < V) return "a row pitch of at least V";
    if (K < 1 || K > VR_MAX_K) return "K in 1..8 (BOFI_REQUIRE_MAX)";
    if (A < 1 || A > VA_MAX_A) return "A in 1..4 (BOFI_REQUIRE_ALT_MAX)";
    if (L < 1 || L > VU_MAX_L) return "L in 1..4 (BOFI_REQUIRE_UNIT_MAX)";
    if (no_repeat != 0 && no_repeat != 1) return "no_repeat 0 or 1";
    if (repeat_min_id < 0) return "repeat_min_id >= 0";
    return nullptr;
}

int bofi::launch_vocab_require_any(const float* x, int ldx, int rows, int V, int S, const int* ntok, int ntok_bias, const int* alts, int K, int A, int L,
                                   const uint32_t* ban_bits, int no_repeat, int repeat_min_id, int64_t* seq, float* row_chosen, int* pos, int* which, int* moved,
                                   hipStream_t st) {
    if (vocab_require_any_check(x, ldx, rows, V, S, alts, K, A, L, no_repeat, repeat_min_id, seq, pos, which)) return BOFI_ERR_ARG;
    if (rows == 0) return BOFI_OK;
    VaArgs a{};
    a.x = x; a.ldx = ldx; a.V = V; a.S = S; a.B = rows / S; a.ntok = ntok; a.ntok_bias = ntok_bias; a.alts = alts; a.K = K; a.A = A; a.L = L; a.ban = ban_bits;
    a.no_repeat = no_repeat; a.repeat_min_id = repeat_min_id; a.seq = seq; a.row_chosen = row_chosen; a.pos = pos; a.which = which; a.moved = moved;
    const size_t per = va_lds_bytes(S, K, A, L);
    a.per_image = (int)per;
    int ipw = VR_IPW;
    while (ipw > 1 && ipw * per > VR_LDS_MAX) ipw /= 2;            // (S = 64, K = 8, A = 4, L = 4: 46.4 KB an image, one per workgroup, four wavefronts on it)
    a.tpi = VA_THREADS / ipw;
    hipLaunchKernelGGL(vocab_require_any_kernel, dim3((a.B + ipw - 1) / ipw), dim3(VA_THREADS), ipw * per, st, a);
    BOFI_CHECK_LAUNCH();
    return BOFI_OK;
}

extern "C" int bofi_vocab_require_any(const float* x, int ldx, int rows, int V, int S, const int* ntok, int ntok_bias, const int* alts, int K, int A, int L,
                                      const uint32_t* ban_bits, int no_repeat, int repeat_min_id, int64_t* seq, float* row_chosen, int* pos, int* which, int* moved,
                                      void* stream) {
    if (const char* why = bofi::vocab_require_any_check(x, ldx, rows, V, S, alts, K, A, L, no_repeat, repeat_min_id, seq, pos, which))
        return bofi::fail(BOFI_ERR_ARG, std::string("vocab_require_any: ") + why);
    return bofi::launch_vocab_require_any(x, ldx, rows, V, S, ntok, ntok_bias, alts, K, A, L, ban_bits, no_repeat, repeat_min_id, seq, row_chosen, pos, which, moved,
                                          (hipStream_t)stream);
}
