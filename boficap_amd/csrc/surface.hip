// The surface of evaluated captions, on the device: the bad-ending trim of the reference's decode_sequence (captioning/utils/misc.py:75-82,
// REMOVE_BAD_ENDINGS) with the bad-ending flag of its language_eval (count_bad, captioning/utils/eval_utils.py:32-37), and the lookup of
// generated sentences among the training sentences behind its novel_sentences / vocab_size (eval_utils.py:61-69).  Both on id rows.
//
// bofi_caption_trim: one wavefront per row, four rows per workgroup; lane t holds id t of the row (S <= 64).  The caption ends at the lowest set
// bit of the ballot of "id <= limit" (lanes past S count as ends), the kept length is one past the highest set bit of the ballot of "in the
// caption and not a trim word" -- and the whole caption when that ballot is empty, as the reference's loop removes nothing when it finds no
// good word.  The two word sets are bit tables over the vocabulary (~1.2 KB at V = 9 495), read through the cache.
//
// bofi_sentence_lookup: one wavefront per row runs a binary search over the M sorted training rows; a probe compares all positions at once,
// lane t against column t, and the lowest differing lane of the ballot gives the ordering.  Each kept id marks seen[id] with a plain store
// (every writer writes 1).
//
// Integers and comparisons only: bit-identical run to run and reproducible on the host.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bofi_common.h"
#include "boficap_hip.h"

namespace {

constexpr int WAVE = 64;
constexpr int WAVES = 4;          // rows per workgroup

// is id v in the bit table?  ids outside [0, V) are in no table and are not looked up
__device__ __forceinline__ bool in_table(const uint32_t* bits, int64_t v, int V) {
    if (!bits || v < 0 || v >= (int64_t)V) return false;
    return (bits[v >> 5] >> (v & 31)) & 1u;
}

// (seq and out_seq may be the same buffer: a lane reads its own element before it writes it, and no lane reads another's)
__global__ void __launch_bounds__(WAVE * WAVES) caption_trim_kernel(const int64_t* seq, int rows, int S, int limit, const uint32_t* __restrict__ trim_bits,
                                                                    const uint32_t* __restrict__ count_bits, int V, int pad, int64_t* out_seq,
                                                                    int* __restrict__ out_len, int* __restrict__ out_bad) {
    const int lane = threadIdx.x % WAVE;
    const int r = blockIdx.x * WAVES + threadIdx.x / WAVE;
    if (r >= rows) return;                                // the last workgroup's tail: whole wavefronts leave, and nothing below waits for them
    const bool live = lane < S;
    const int64_t at = (int64_t)r * S + lane;
    const int64_t v = live ? seq[at] : 0;
    const unsigned long long stops = __ballot(!live || v <= (int64_t)limit);
    const int L = stops ? __ffsll(stops) - 1 : WAVE;      // the caption: the ids before the first id <= limit
    const unsigned long long good = __ballot(lane < L && !in_table(trim_bits, v, V));
    const int keep = good ? WAVE - __clzll(good) : L;     // one past the last word that is no trim word; none at all: nothing is removed
    const unsigned long long bad = __ballot(lane == keep - 1 && in_table(count_bits, v, V));
    if (live) out_seq[at] = lane < keep ? v : (int64_t)pad;
    if (lane == 0) {
        out_len[r] = keep;
        out_bad[r] = bad ? 1 : 0;
    }
}

__global__ void __launch_bounds__(WAVE * WAVES) sentence_lookup_kernel(const int64_t* __restrict__ seq, const int* __restrict__ len, int rows, int S,
                                                                       const int* __restrict__ train, int M, int St, int V, int* __restrict__ novel,
                                                                       int* seen) {
    const int lane = threadIdx.x % WAVE;
    const int r = blockIdx.x * WAVES + threadIdx.x / WAVE;
    if (r >= rows) return;
    int n = len[r];
    n = n < 0 ? 0 : (n > S ? S : n);
    const bool kept = lane < n;
    const int64_t x = kept ? seq[(int64_t)r * S + lane] : 0;      // the canonical row, zero-extended to 64 positions
    if (kept && x >= 0 && x < (int64_t)V) seen[x] = 1;
    int lo = 0, hi = M;
    bool found = false;
    while (lo < hi) {                                     // (lo, hi and the branch are the same in every lane)
        const int mid = lo + (hi - lo) / 2;
        const int64_t y = lane < St ? (int64_t)train[(int64_t)mid * St + lane] : 0;
        const unsigned long long differ = __ballot(x != y);
        if (!differ) {
            found = true;
            break;
        }
        const unsigned long long below = __ballot(x < y);
        if ((below >> (__ffsll(differ) - 1)) & 1ull)      // the first differing position decides
            hi = mid;
        else
            lo = mid + 1;
    }
    if (lane == 0) novel[r] = found ? 0 : 1;
}

}  // namespace

extern "C" int bofi_caption_trim(const int64_t* seq, int rows, int S, int limit, const uint32_t* trim_bits, const uint32_t* count_bits, int V, int pad,
                                 int64_t* out_seq, int* out_len, int* out_bad, void* stream) {
    if (!seq || !out_seq || !out_len || !out_bad || rows < 0 || S < 1 || S > WAVE || V < 1)
        return bofi::fail(BOFI_ERR_ARG, "caption_trim: rows >= 0, 1 <= S <= 64, V >= 1, non-null seq / out_seq / out_len / out_bad");
    if (rows == 0) return BOFI_OK;
    hipLaunchKernelGGL(caption_trim_kernel, dim3((rows - 1) / WAVES + 1), dim3(WAVE * WAVES), 0, (hipStream_t)stream, seq, rows, S, limit, trim_bits,
                       count_bits, V, pad, out_seq, out_len, out_bad);
    BOFI_CHECK_LAUNCH();
    return BOFI_OK;
}

extern "C" int bofi_sentence_lookup(const int64_t* seq, const int* len, int rows, int S, const int* train, int M, int St, int V, int* novel, int* seen,
                                    void* stream) {
    if (!seq || !len || !novel || !seen || rows < 0 || S < 1 || S > WAVE || M < 0 || St < 1 || St > WAVE || (M > 0 && !train) || V < 1)
        return bofi::fail(BOFI_ERR_ARG, "sentence_lookup: rows >= 0, 1 <= S <= 64, M >= 0, 1 <= St <= 64, V >= 1, non-null seq / len / novel / seen, train when M > 0");
    if (rows == 0) return BOFI_OK;
    hipLaunchKernelGGL(sentence_lookup_kernel, dim3((rows - 1) / WAVES + 1), dim3(WAVE * WAVES), 0, (hipStream_t)stream, seq, len, rows, S, train, M, St, V,
                       novel, seen);
    BOFI_CHECK_LAUNCH();
    return BOFI_OK;
}
