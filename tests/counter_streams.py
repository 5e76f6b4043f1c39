"""Host restatement of the two counter hashes behind every random number drawn on the device (csrc/bofi_common.h), and of the
rules the kernels document for them: which id the Gumbel-max sampler draws (vocab_sample_kernel) and which element a dropout
site keeps (bofi_kernels.h).  Plain NumPy, uint64 arithmetic that wraps mod 2^64; nothing here is taken from the kernels but
those rules, so a test that compares a kernel with this file pins the stream itself -- not its rate, not two sites to each other."""
import numpy as np

GOLDEN = 0x9E3779B97F4A7C15
_M64 = (1 << 64) - 1
_U = np.uint64


def _u64(x):
    """Python int (any sign / width) or array -> uint64, mod 2^64."""
    if isinstance(x, (int, np.integer)):
        return _U(int(x) & _M64)
    return np.asarray(x).astype(np.uint64)


def _mix(z):
    with np.errstate(over="ignore"):
        z = (z ^ (z >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U(27))) * _U(0x94D049BB133111EB)
    return z ^ (z >> _U(31))


def hash64_hi(seed, i):
    """Upper half of the splitmix64 finaliser of seed + (i + 1) * golden: uint32, vectorised over i."""
    with np.errstate(over="ignore"):
        z = _u64(seed) + (_u64(i) + _U(1)) * _U(GOLDEN)
    return (_mix(z) >> _U(32)).astype(np.uint32)


def drop_hash(seed, i):
    """The dropout hash: a 64-bit mix of the seed keys a 32-bit multiply-xorshift hash of the element id (the id's upper half
    enters rotated left by 19)."""
    i = _u64(i)
    with np.errstate(over="ignore"):
        k = _mix((_u64(seed) + _U(0x632BE59BD9B4E019)) * _U(GOLDEN))
    klo, khi = np.uint32(int(k) & 0xFFFFFFFF), np.uint32(int(k) >> 32)
    lo, hi = (i & _U(0xFFFFFFFF)).astype(np.uint32), (i >> _U(32)).astype(np.uint32)
    with np.errstate(over="ignore"):
        x = lo + ((hi << np.uint32(19)) | (hi >> np.uint32(13)))
        x = x ^ klo
        x = (x ^ (x >> np.uint32(16))) * np.uint32(0x7FEB352D)
        x = ((x ^ (x >> np.uint32(15))) + khi) * np.uint32(0x846CA68B)
    return x ^ (x >> np.uint32(16))


U_MAX = np.float32(1.0) - np.float32(2.0 ** -24)          # the largest float32 below 1


def uniform(h):
    """The sampler's uniform number of a hash, operation by operation in float32: min((float(h) + 0.5) * 2^-32, 1 - 2^-24).
    The conversion and the sum round to nearest even as the device's do; the product by a power of two is exact."""
    f = np.asarray(h, dtype=np.uint32).astype(np.float32)
    u = (f + np.float32(0.5)) * np.float32(2.0 ** -32)
    return np.minimum(u, U_MAX)


def uniform_unclamped(h):
    """The rule before the clamp: rounds every hash >= 0xFFFFFF80 up to 1.0 exactly.  Kept to state what was wrong."""
    f = np.asarray(h, dtype=np.uint32).astype(np.float32)
    return (f + np.float32(0.5)) * np.float32(2.0 ** -32)


def gumbel_scores(lp_row, seed, row, c, n, T, uniform_fn=uniform):
    """Float64 Gumbel-max scores of draw ``c`` (of ``n``) of row ``row``: element i uses counter (row * n + c) * V + i, a NaN log-prob
    counts as -10, score = lp * float64(float32(1) / float32(T)) - log(-log(u)) from the float32 u.  ``c`` may be an array of
    draws: the result is then [len(c), V]."""
    lp = np.asarray(lp_row, dtype=np.float32)
    V = lp.shape[-1]
    with np.errstate(over="ignore"):
        base = (_u64(row) * _U(n) + _u64(c)) * _U(V)
        ctr = np.asarray(base)[..., None] + np.arange(V, dtype=np.uint64)
    u = uniform_fn(hash64_hi(seed, ctr)).astype(np.float64)
    inv_t = np.float64(np.float32(1.0) / np.float32(T))
    x = np.where(np.isnan(lp), np.float32(-10.0), lp).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return x * inv_t - np.log(-np.log(u))


def all_scores(lp, seed, n, T, uniform_fn=uniform):
    """gumbel_scores of every (row, draw): lp [rows, V] -> float64 [rows, n, V]."""
    lp = np.asarray(lp, dtype=np.float32)
    return np.stack([gumbel_scores(lp[r], seed, r, np.arange(n), n, T, uniform_fn) for r in range(lp.shape[0])])


def near_tie_tol(lp, T):
    """What two float32 evaluations of one score may differ by (16 ulp at the larger of the Gumbel term's and lp / T's magnitude):
    the device computes the score in float32, possibly with the multiply and subtract contracted, from a logf a few ulp off."""
    lp = np.asarray(lp, dtype=np.float64)
    fin = np.abs(lp[np.isfinite(lp)])
    big = float(fin.max()) / float(T) if fin.size else 0.0
    return 16.0 * float(np.spacing(np.float32(max(32.0, big))))


def draw_candidates(scores, tol):
    """Every index within ``tol`` of the maximum score, lowest first.  A row without any score above -inf (or NaN only) leaves the
    sampler's running best at its start: index 0."""
    s = np.asarray(scores, dtype=np.float64)
    s = np.where(np.isnan(s), -np.inf, s)
    m = s.max()
    if m == -np.inf:
        return np.zeros(1, dtype=np.int64)
    if m == np.inf:
        return np.flatnonzero(s == np.inf)
    return np.flatnonzero(s >= m - tol)


def drop_thresh(p):
    return np.uint32(int(np.float64(np.float32(p)) * 4294967296.0))


def keep_mask(seed, step, p, idx):
    """True where the element is kept: drop_hash(seed + step, idx) >= uint32(float64(float32(p)) * 2^32)."""
    return drop_hash((int(seed) + int(step)) & _M64, idx) >= drop_thresh(p)


def linear_ids(M, N):
    """Element ids of a linear site's [M, N] output: m * N + n."""
    return (np.arange(M, dtype=np.uint64)[:, None] * _U(N) + np.arange(N, dtype=np.uint64)[None, :])


def attn_ids_padded(B, H, Lq, Lk):
    """Element ids of attention-probability dropout over padded items, [B, H, Lq, Lk]: ((b * H + h) * Lq + q) * Lk + k."""
    b, h, q, k = np.ogrid[:B, :H, :Lq, :Lk]
    return (((b * H + h) * Lq + q) * Lk + k).astype(np.uint64)


def attn_ids_unpadded(rows, H, Lk):
    """Element ids over unpadded rows, [len(rows), H, Lk]: (global query row * H + h) * Lk + k."""
    r = np.asarray(rows, dtype=np.int64)[:, None, None]
    h, k = np.arange(H)[None, :, None], np.arange(Lk)[None, None, :]
    return ((r * H + h) * Lk + k).astype(np.uint64)
