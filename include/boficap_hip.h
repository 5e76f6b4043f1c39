/*
 * boficap_hip.h -- C ABI of libboficap_hip.so, the MI355X (gfx950) implementation of BoFiCap's
 * bound+fill caption decoder hot path.
 *
 * The reference (ChangxinWang/BoFiCap) is pure Python/PyTorch and has no FFI layer; its hot path
 * is a chain of stock torch ops.  Each entry point below therefore names the reference function
 * (file:line under /root/reference) whose arithmetic it replaces.  All pointers are DEVICE
 * pointers unless a name ends in _host; all sizes are element counts; `stream` is a hipStream_t
 * passed as void* (NULL = the default stream).  Every function returns 0 on success and a
 * BOFI_ERR_* code otherwise; nothing here allocates or synchronises except the engine
 * constructor/finaliser.  Thread-safety: one engine per host thread / per GPU process (the
 * reference is single-threaded per replica, tools/train.py:99-101).
 *
 * dtype codes: 0 = float32, 1 = bfloat16 (raw 16-bit).  "compute dtype" is the type GEMM and
 * attention operands are held in; accumulation, softmax, LayerNorm statistics and the residual
 * stream are always float32.
 */
#ifndef BOFICAP_HIP_H
#define BOFICAP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BOFI_OK 0
#define BOFI_ERR_ARG 1    /* bad shape / dtype / NULL pointer */
#define BOFI_ERR_HIP 2    /* a HIP runtime call failed */
#define BOFI_ERR_STATE 3  /* engine used before finalize, missing weight, ... */

#define BOFI_DT_F32 0
#define BOFI_DT_BF16 1
#define BOFI_DT_F16 2   /* float16 (raw 16-bit): the input of bofi_pack_regions only */

/* version of this ABI; bumped on any signature change */
int bofi_abi_version(void);

/* ---------------------------------------------------------------------------------------------
 * Operator level (stateless).  Used by the engine and by the per-kernel parity tests.
 * ------------------------------------------------------------------------------------------- */

/* BoFiCap LayerNorm: y = gain * (x - mean) / (std_unbiased + 1e-6) + bias, per row.
 * Replaces captioning/models/TransformerModel.py:1346-1349 (NOT nn.LayerNorm: N-1 variance, eps
 * added to std).  x: float32 [rows, d];  y: y_dtype [rows, d];  d % 64 == 0, d <= 2048. */
int bofi_layernorm(const float* x, const float* gain, const float* bias, void* y, int y_dtype,
                   int rows, int d, void* stream);

/* y = act(x . w^T + bias) [+ residual], the nn.Linear of TransformerModel.py:1454-1456,1467
 * (attention projections), :1477-1478 (FFN), :1642-1645 (att_embed Linear+ReLU), :1316-1319
 * (generator.proj).
 *   x: x_dtype [M, K] row stride ldx (x_dtype = w_dtype, or float32 converted on load)
 *   w: w_dtype [N, K] contiguous (the nn.Linear weight as stored);  bias: float32 [N] or NULL
 *   residual: float32 [M, N] row stride ldr or NULL, added AFTER bias/activation
 *             (SublayerConnection, TransformerModel.py:1361-1363)
 *   y: y_dtype [M, N] row stride ldy (float32 or w_dtype)
 *   relu: 0/1.   row_len/rows_per_group: if row_len != NULL, output row m is forced to exact 0
 *   when (m % rows_per_group) >= row_len[m / rows_per_group]  (pack_padded/pad_packed semantics of
 *   AttModel.py:46-51).   K % 64 == 0 for bf16, K % 32 == 0 for float32. */
int bofi_linear(const void* x, int x_dtype, int ldx, const void* w, int w_dtype, const float* bias,
                const float* residual, int ldr, void* y, int y_dtype, int ldy, int M, int N, int K,
                int relu, const int* row_len, int rows_per_group, void* stream);

/* Multi-head scaled-dot-product attention core, softmax(q k^T / sqrt(64) masked) v, head dim 64.
 * Replaces attention() TransformerModel.py:1421-1432 for prefix-structured masks: query row i of
 * batch item b may attend keys j < klen[b*klen_sb + i*klen_sq] (every mask the reference builds
 * for this path has that form).  A row with klen 0 yields NaN like the reference's
 * softmax over all -inf.  klen == NULL means all Lk keys.
 *   q: dtype, row (b,i) at q + (b*Lq+i)*ldq, head h at column h*64;  k, v likewise with Lk, ldk, ldv
 *   out: dtype [B*Lq, H*64] row stride ldo.    Lq, Lk <= 128. */
int bofi_attention(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* out,
                   int ldo, int dtype, int B, int H, int Lq, int Lk, const int* klen, int klen_sb,
                   int klen_sq, void* stream);

/* log_softmax over the vocabulary + greedy pick + pad-after-length, one row per (image, position).
 * Replaces F.log_softmax(self.logit(phrase), dim=2) AttModel.py:206-207, torch.max(logprobs, 2)
 * CaptionModel.py:388-390 (first maximal index; a NaN wins and the first NaN is returned, as
 * torch.max does on CPU) and seq[b, sum(phrase_length[b]):] = pad AttModel.py:422-423.
 *   logits: float32 [rows, V], overwritten in place with log-probabilities when log_softmax != 0
 *   ntok: int32 [rows / S] valid token count per image or NULL;  seq: int64 [rows]. */
int bofi_vocab_finalize(float* logits, int rows, int V, int S, int log_softmax, const int* ntok,
                        int pad_idx, int64_t* seq, void* stream);

/* bofi_attention with the two extra knobs of the training path: effective key count =
 * klen[...] + klen_bias, and key/value batch item = b / kdiv (the seq_per_img captions of one image
 * attend the image's memory without repeating it; the reference repeats it, models/utils.py:3-14).
 * drop_p > 0 (bf16, Lk <= 64 only): dropout on the attention probabilities (TransformerModel.py:1430-1431),
 * keep(b, h, q, k) = hash(drop_seed + *drop_step, ((b*H + h)*Lq + q)*Lk + k) >= drop_p * 2^32, kept ones / (1 - drop_p).
 * q_start / q_count (int32 [B] each, or both NULL): unpadded rows -- batch item b owns the q_count[b] query rows starting at
 * row q_start[b]; with k_ragged its keys / values are laid out the same way (self-attention), else (b / kdiv) * Lk as usual;
 * q_rows > 0 (bf16 kernels, the MFMA backward): total rows of the q / out buffers -- the rows behind the last item, which no item
 * owns, are written as zeros (0: left untouched);
 * klen is then indexed by the global query row; Lq / Lk are the maxima.  Same three arguments on the two backward entry points. */
int bofi_attention_ex(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* out,
                      int ldo, int dtype, int B, int H, int Lq, int Lk, int kdiv, const int* klen,
                      int klen_sb, int klen_sq, int klen_bias, float drop_p, uint64_t drop_seed,
                      const uint64_t* drop_step, const int* q_start, const int* q_count, int k_ragged, int q_rows, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training ops (float32).  The reference trains by running torch autograd over
 * TransformerModel._forward (tools/train.py:212-227); these are the hand-written backward (and the
 * few extra forward) kernels the XE step needs.  Parameter gradients that are sums over rows are
 * ACCUMULATED into the given buffers (zero them first).
 * ------------------------------------------------------------------------------------------- */
/* backward of bofi_layernorm: dx [rows, d] (+ add [rows, d] when given: the gradient that reaches x along the residual
 * connection, so that the sum of the two branches costs no extra pass); dgain, dbias [d] accumulated */
int bofi_layernorm_bwd(const float* x, const float* gain, const float* dy, const float* add, float* dx, float* dgain,
                       float* dbias, int rows, int d, void* stream);
/* the same, additionally writing dz_bf16 [rows, d] (d = 512 or 128; may be NULL) = bf16(keep(dx) / (1 - drop_p)) with the
 * dropout mask of bofi_linear_ex(drop_p, drop_seed, drop_step) over [rows, d]: when x = residual + dropout(h W^T + b) came out of
 * that linear's epilogue, dz is the gradient its backward GEMMs read, and the separate mask-and-cast pass is not needed */
int bofi_layernorm_bwd_ex(const float* x, const float* gain, const float* dy, const float* add, float* dx, float* dgain,
                          float* dbias, int rows, int d, void* dz_bf16, float drop_p, uint64_t drop_seed,
                          const uint64_t* drop_step, void* stream);
/* backward of bofi_attention_ex (Lk <= 128, any Lq: the query rows are walked in chunks of 32 or 64): dq like q, dk/dv like
 * k/v, ACCUMULATED into zeroed buffers when kdiv > 1 or the query rows take more than one chunk (Lq > 32 beyond 64 keys,
 * Lq > 64 otherwise), written otherwise; q_start / q_count / k_ragged as in bofi_attention_ex (k_ragged: Lq <= 128) */
int bofi_attention_bwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                       const float* dout, int ldo, float* dq, float* dk, float* dv, int B, int H, int Lq,
                       int Lk, int kdiv, const int* klen, int klen_sb, int klen_sq, int klen_bias,
                       const int* q_start, const int* q_count, int k_ragged, void* stream);
/* the same backward on the matrix cores: q/k/v float32 or bf16 (in_dtype), products in bf16 with fp32 accumulation,
 * operands gathered with transposing LDS reads; dq row stride lddq, dk/dv row stride lddk, float32 or bf16 (dq_dtype /
 * dkv_dtype: bf16 when the gradient feeds a GEMM directly), WRITTEN (not accumulated) also when kdiv > 1: one workgroup owns
 * an (image, head) and sums over its captions in registers / LDS; Lq <= 64 unless q_start is given with k_ragged == 0 (then
 * the key owner's rows are one contiguous run walked in chunks and Lq is only an upper bound);
 * drop_*: the dropout of the forward's attention probabilities, regenerated from the same (seed, index) */
int bofi_attention_bwd_mfma(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, int in_dtype,
                            const float* dout, int ldo, void* dq, int lddq, void* dk, void* dv, int lddk, int dq_dtype,
                            int dkv_dtype, int B, int H, int Lq, int Lk, int kdiv, const int* klen, int klen_sb, int klen_sq,
                            int klen_bias, float drop_p, uint64_t drop_seed, const uint64_t* drop_step, const int* q_start,
                            const int* q_count, int k_ragged, int q_rows, void* stream);
/* backward of log_softmax given the log-probabilities y: dx = dy - exp(y) * rowsum(dy) */
int bofi_logsoftmax_bwd(const float* y, const float* dy, float* dx, int rows, int V, void* stream);
/* The loader's phrase-aware collate (captioning/data/dataloader.py:343-428) of SAMPLED captions, semi-autoregressive half, on the device: seq int64 [N, S] (tokens),
 * phrase_length int32 / phrase_syn int64 [N, S] (slot layout, real phrases first) -> per position the decoder input token (sa_seq: the previous phrase squeezed or
 * stretched over this one, BOS before the first), the phrase's label (sa_syn) and the number of visible keys (sa_klen).  The self-critical step's per-phrase forwards
 * read these (loss_wrapper.py:193-209 behind TransformerModel.py:1903-1984); no host round trip, capturable. */
/* The self-critical step's bookkeeping behind a draw: positions of phrases [p0, p1) of every caption (phrase_length int32 [N, S]) take tok int64 [N, S] into seq, the
 * token's log-prob lp[n, t, tok] (float32 [N, S, V]) into drawn, and set mask (bool [N, S], or NULL); the other positions are left alone. */
int bofi_rl_take_draws(const float* lp, const int64_t* tok, const int* phrase_length, int N, int S, int V, int p0, int p1, int64_t* seq, float* drawn, void* mask,
                       void* stream);
int bofi_saic_collate(const int64_t* seq, const int* phrase_length, const int64_t* phrase_syn, int N, int S, int bos_idx, int64_t* sa_syn, int64_t* sa_seq,
                      int* sa_klen, void* stream);
/* backward of picked[r] = y[r][labels[r]] straight through the log_softmax that made y (the token terms of
 * LanguageModelCriterion_UIC, losses.py:341-347: gather on the log-probs): dx[r][c] = dpicked[r] * ((c == labels[r]) - exp(y[r][c])).
 * labels must lie in [0, V).  dx: float32 [rows, V] (lddx == V), or bf16 [rows, lddx] with lddx >= V and the columns V..lddx-1
 * written as zeros (the operand the vocabulary projection's backward GEMMs read, K granule 64). */
int bofi_nll_bwd(const float* y, const int64_t* labels, const float* dpicked, void* dx, int dx_dtype, int lddx, int rows, int V,
                 void* stream);

/* LanguageModelCriterion_UIC (captioning/modules/losses.py:319-369, reduction 'mean') in one launch, for the paired training
 * forward: the four slot outputs [N, Pm, c_len | c_syn] (log-probs), the loader's phrase_num [N], phrase_length / phrase_syn
 * [N, L] (int64; slot p is counted iff p < phrase_num[n], its labels sit at column p + 1), the picked token log-probs [T] with
 * the SA / NA row weights.  out8 = {sa_len, sa_tok, sa_syn, na_len, na_tok, na_syn parts, their sum (the loss), sum(w_sa)}.
 * The backward takes dL/d(loss) (device scalar) and writes dense gradients of the four slot outputs and d_picked [T]. */
int bofi_uic_criterion(const float* sa_len, const float* sa_syn, const float* na_len, const float* na_syn, int N, int Pm, int c_len,
                       int c_syn, const int64_t* phrase_num, const int64_t* phrase_length, const int64_t* phrase_syn, int L,
                       const float* picked, const float* w_sa, const float* w_na, int T, float* out8, void* stream);
int bofi_uic_criterion_bwd(const float* sa_len, const float* sa_syn, const float* na_len, const float* na_syn, int N, int Pm,
                           int c_len, int c_syn, const int64_t* phrase_num, const int64_t* phrase_length,
                           const int64_t* phrase_syn, int L, const float* picked, const float* w_sa, const float* w_na, int T,
                           const float* g_loss, const float* out8, float* d_sa_len, float* d_sa_syn, float* d_na_len,
                           float* d_na_syn, float* d_picked, void* stream);
/* out[n] += sum_m x[m][n]  (bias gradients) */
int bofi_colsum_add(const float* x, float* out, int M, int N, void* stream);
/* x[r] = sqrt(d) * (lut_tok[tok[r]] + lut_syn[syn[r]]) + pe[pos ? pos[r] : r % L]; tok or syn may be NULL, a negative id
 * leaves that term out for the row (also in bofi_embed_bwd)
 * (Embeddings + PositionalEncoding, TransformerModel.py:1484-1511) and its backward into one table */
int bofi_embed_rows(const float* lut_tok, const float* lut_syn, const float* pe, const int64_t* tok,
                    const int64_t* syn, const int64_t* pos, int rows, int L, int d, float* x, void* stream);
int bofi_embed_bwd(const float* dx, const int64_t* ids, float* dlut, int rows, int d, float scale, void* stream);
/* Weight-gradient GEMM: c[i][j] += sum_m a[m][i] * b[m][j], i < NI, j < NJ (dW = dz^T x without transposed copies).
 * a, b: bf16 row-major [M, a_cols | b_cols] (cols a multiple of 8, zero beyond NI | NJ; 16-byte aligned rows);
 * c: float32 [NI, NJ] row stride ldc, ACCUMULATED into with atomics (zero it for a plain product).
 * colsum (may be NULL): colsum[i] += sum_m a[m][i], taken from the A tiles while they sit in LDS (dz's column sums = the
 * bias gradient; a few atomics per workgroup instead of a reduction pass of its own). */
int bofi_gemm_tn_acc(const void* a, int lda, int a_cols, const void* b, int ldb, int b_cols, float* c, int ldc, int M,
                     int NI, int NJ, float* colsum, void* stream);

/* n weight-gradient GEMMs (each as bofi_gemm_tn_acc: c[e] += a[e]^T b[e], colsum[e] += column sums of a[e]; colsum or its
 * entries may be NULL) in as few launches as the kernel-argument space allows (40 problems each).  All arrays are HOST arrays
 * of n entries; the problems are passed to the kernel by value.  The training step defers the weight gradients of all its
 * Linear layers (nn.Linear's grad_weight, one addmm each in the reference) to one such call after backward. */
int bofi_gemm_tn_grouped(int n, const void* const* a, const int* lda, const int* a_cols, const void* const* b, const int* ldb,
                         const int* b_cols, float* const* c, const int* ldc, const int* M, const int* NI, const int* NJ,
                         float* const* colsum, void* stream);
/* xt[n][m] = x[m][n], zero for M <= m < Mpad, written as out_dtype: operand layout of the weight-gradient GEMM.
 * colsum (may be NULL): colsum[n] += sum_m x[m][n], the bias gradient, taken from the tiles while they are in LDS */
int bofi_transpose_pad(const float* x, int ldx, void* xt, int out_dtype, int M, int N, int Mpad, float* colsum, void* stream);

/* All weight operands of the backward's input-gradient GEMMs in one launch.  table[e] = {src_off, dst_off, N, K, Np} (int64,
 * element offsets): the bf16 matrix [N, K] at src + src_off is written transposed as [K, Np] at dst + dst_off (pad columns
 * N..Np-1 untouched).  tile_first[e] = number of 64 x 64 tiles of the entries before e (tile_first[n] = total_tiles).
 * Replaces one bofi_transpose_pad per weight and step; same role as the .t() views autograd takes of nn.Linear weights. */
int bofi_transpose_many(const void* src_bf16, void* dst_bf16, const int64_t* table, const int* tile_first, int n,
                        int total_tiles, void* stream);
/* y[m][n] = bf16(x[m][n]) for n < N, zero for N <= n < ldy: a GEMM operand in the bf16 compute dtype.
 * relu_y (may be NULL): forward output of a ReLU layer, same layout as x: x is masked where relu_y <= 0 first.
 * drop_p > 0: then the dropout mask of bofi_linear_ex(drop_p, drop_seed, drop_step) is applied (x' = keep(x) / (1 - p)).
 * colsum (may be NULL): colsum[n] += sum_m x'[m][n] on the way (the bias gradient when x is dz) */
int bofi_cast_bf16(const float* x, int ldx, void* y, int ldy, int M, int N, float* colsum, const float* relu_y, float drop_p,
                   uint64_t drop_seed, const uint64_t* drop_step, void* stream);
/* bofi_linear with every epilogue option of the training path.  Dropout (drop_p 0: off):
 * y = residual + keep(act(x w^T + bias)) / (1 - drop_p), keep(m, n) = hash(seed, m * N + n) >= drop_p * 2^32 with
 * seed = drop_seed + (drop_step ? *drop_step : 0) -- drop_step is a DEVICE word, so a captured hipGraph draws fresh masks
 * on every replay (SublayerConnection x + dropout(sublayer(norm(x))), TransformerModel.py:1361-1363; FFN dropout :1478);
 * y2 (may be NULL): a second copy of the output in the compute dtype, row stride ldy2 (N % 32 == 0) -- the operand of
 * the next GEMM / attention kernel, so that no separate cast pass is needed. */
int bofi_linear_ex(const void* x, int x_dtype, int ldx, const void* w, int w_dtype, const float* bias,
                   const float* residual, int ldr, void* y, int y_dtype, int ldy, int M, int N, int K, int relu,
                   const int* row_len, int rows_per_group, float drop_p, uint64_t drop_seed, const uint64_t* drop_step, void* y2,
                   int ldy2, void* stream);

/* The fused decode-path linear on bf16 operands (nn.Linear behind a pre-norm SublayerConnection, TransformerModel.py:1337-1363):
 * ln_stats != NULL: x is the RAW residual stream in bf16 and the LayerNorm is folded in -- w must be W * gain, bias = W . beta + b,
 * ln_colsum[n] = sum_k w[n][k], ln_stats = [M][ln_groups][2] partial (sum, sum of squares) pairs of the float32 rows (ln_groups 0: K / 32),
 * y = rstd[m] * (x w^T - mean[m] * colsum) + bias;  then ReLU, then + residual (float32, may alias y);  y2 (may be NULL): a bf16 copy,
 * stats_out (may be NULL): [M][N / 32][2] partial sums of the OUTPUT rows for the next folded LayerNorm.
 * Large shapes (>= 200 tiles of 256 x 128, N % 128 == 0) run as persistent workgroups (gemm_pers.hip), the others one tile per
 * workgroup (gemm_glds.hip): bit-identical results either way. */
int bofi_linear_fused(const void* x, int ldx, const void* w, const float* bias, const float* residual, int ldr, void* y, int y_dtype, int ldy,
                      void* y2, int ldy2, const float* ln_stats, const float* ln_colsum, int ln_groups, float* stats_out, int M, int N, int K,
                      int relu, void* stream);

/* The BOFI_* knobs of the library (the table in csrc/bofi_knobs.h) are read from the environment at first use, all of them: after changing
 * one in a running process call this to have them all read again (it also starts a new generation of the engines' graph keys).  Not to be
 * called while another thread launches. */
void bofi_reload_env(void);

/* y = mask > 0 ? (x w^T) * scale : 0 (no bias): the input gradient of a linear whose INPUT came out of relu (+ dropout with
 * scale = 1 / (1 - p)) -- mask [M, N] float32 is that forward activation (a clipped or dropped unit is 0 there), so the
 * gradient arrives already masked, e.g. in bf16 for the previous layer's backward GEMMs (nn.Linear backward followed by the
 * relu / dropout backward in the reference).  Operands in the compute dtype, N % 4 == 0. */
/* bofi_linear over a ROW LIST: rows row_idx[0 .. *n_rows) of x (both in device memory; M = capacity the launch is sized for) are
 * multiplied and written to the same rows of y (residual read at those rows); other rows of y stay untouched.  The count is read on the
 * device, so a captured launch serves any list (the semi-autoregressive decode's per-iteration rows).  x and w in one dtype, K a
 * multiple of the 128-byte slab. */
int bofi_linear_rows(const void* x, int x_dtype, int ldx, const void* w, int w_dtype, const float* bias, const float* residual, int ldr,
                     void* y, int y_dtype, int ldy, int M, int N, int K, int relu, const int* row_idx, const int* n_rows, void* stream);
int bofi_linear_masked(const void* x, int x_dtype, int ldx, const void* w, int w_dtype, const float* mask, int ldm,
                       float scale, void* y, int y_dtype, int ldy, int M, int N, int K, void* stream);

/* y = (residual or 0) + keep(x) / (1 - p), keep mask = hash(seed, index) (nn.Dropout of the sublayers,
 * TransformerModel.py:1361-1363; the backward is the same call on dy with the same seed) */
int bofi_dropout(const float* x, const float* residual, float* y, int64_t n, float p, uint64_t seed, const uint64_t* drop_step,
                 void* stream);
/* One optimiser step over a flat float32 bucket (n % 4 == 0, 16-byte aligned): g' = clamp(g * grad_scale, +-clip_value)
 * (clip_value <= 0: no clamp; train.py:225-226), then torch.optim.Adam's update with bias correction for `step` >= 1
 * (misc.py:245-251).  shadow_bf16 (may be NULL) receives a bf16 copy of the new parameters. */
int bofi_adam_step(float* p, const float* g, float* m, float* v, void* shadow_bf16, int64_t n, float lr, float beta1,
                   float beta2, float eps, int step, float clip_value, float grad_scale, void* stream);
/* dx = dy where y > 0 */
int bofi_relu_bwd(const float* y, const float* dy, float* dx, int64_t n, void* stream);

/* Per row sum_v exp(logp_v) * logp_v and logp[row, seq[row]]: the reductions behind eval's per-image entropy and
 * perplexity (captioning/utils/eval_utils.py:463-464) without reading the distribution back in user code. */
int bofi_vocab_stats(const float* logp, const int64_t* seq, int rows, int V, float* row_plogp, float* row_chosen, void* stream);
/* n draws per row from Categorical(logits = logp / temperature) (sample_next_word, CaptionModel.py:405-425; NaN counts as
 * -10): Gumbel-max with a counter-hash uniform strictly inside (0, 1) -- element i of draw c of row r uses counter
 * (r * n + c) * V + i of stream `seed`; the rule is written out in DESIGN.md section 5 and restated in
 * tests/counter_streams.py.  out int64 [(rows / S) * n, S], draw c of image b in row b * n + c
 * (the reference repeats each image n times, models/utils.py:3-14); positions >= ntok[b] get pad_idx (AttModel.py:422-423). */
int bofi_vocab_sample(const float* logp, int rows, int V, int S, int n, float temperature, uint64_t seed, const int* ntok,
                      int pad_idx, int64_t* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Engine level: the whole NAIC bound+fill decode as one call.
 * ------------------------------------------------------------------------------------------- */
typedef struct bofi_engine bofi_engine_t;

typedef struct bofi_config {
    int vocab;        /* tgt_vocab = vocab_size + 4 (AttModel.py:79) */
    int feat;         /* att_feat_size (2048) */
    int d_model;      /* 512; d_model / heads must be 64 */
    int d_ff;         /* 2048 */
    int heads;        /* 8 */
    int n_enc;        /* 6 */
    int n_dec;        /* 6 */
    int seq_length;   /* 20 (S); the bound sequence has S+2 positions */
    int pad_idx, bos_idx, eos_idx, len_idx;   /* 0 1 2 3 */
    int head_hidden;  /* 100: width of Length/Syntactic_classifier1 */
    int max_batch;    /* workspace is sized for this many images per call */
    int max_regions;  /* and this many regions per image (<= 128) */
    int dtype;        /* compute dtype: BOFI_DT_F32 (parity) or BOFI_DT_BF16 (throughput) */
    int n_len;        /* layers of the bounding network (LengthPredictor_UIC N_len, TransformerModel.py:357-375): 1 (configs/uic_sd.yml) takes
                         the row-0-only incremental form; >= 2 (configs/uic_sd_N2.yml) the dense form -- all S+2 rows through every layer
                         per iteration, as the reference computes it (a field since ABI version 2; the library is at version 5: bofi_abi_version) */
} bofi_config_t;

/* Allocates device weights + workspace for one model replica on the current HIP device. */
int bofi_engine_create(const bofi_config_t* cfg, bofi_engine_t** out);
void bofi_engine_destroy(bofi_engine_t* e);

/* Hands the engine one state_dict entry by its reference name (the 311-key schema of
 * TransformerModel.state_dict()), float32 on the HOST.  The engine keeps a copy. */
int bofi_engine_set_weight(bofi_engine_t* e, const char* name, const float* data_host, int64_t numel);

/* Packs/convert the weights for the kernels (fused QKV, stacked cross-attention K/V, bf16 copies)
 * and precomputes the input-independent tables of the bound network.  Must follow the last
 * set_weight and precede decode; may be called again after weights change.  Synchronises. */
int bofi_engine_finalize(bofi_engine_t* e);

/* A second engine that SHARES the parent's packed weights and has its own workspace, so that several
 * decodes can be in flight on different streams (the bounding loop is a latency chain that leaves most
 * CUs idle; a batch in another stream fills them).  The parent must outlive its forks and must not be
 * re-finalized while they exist.  Destroy a fork with bofi_engine_destroy. */
int bofi_engine_fork(bofi_engine_t* parent, bofi_engine_t** out);
/* The same with a workspace for up to max_batch images per call (0 = the parent's): dynamic batching puts several loader batches into one decode call
 * (bofi_call_opts_t.q1_group), which a model built for one batch per call has no workspace for -- its weights serve either size. */
int bofi_engine_fork_sized(bofi_engine_t* parent, int max_batch, bofi_engine_t** out);
/* The same with options.  BOFI_FORK_IDS_ONLY: a workspace WITHOUT the two vocabulary-wide float32 buffers (max_batch * S * (vocab + padded vocab) * 4 bytes: most of a
 * fork's memory) -- for decodes under BOFI_FLAG_IDS_ONLY that take the fused generator.  On such a fork a decode without that flag, one whose launch would need
 * the buffers after all (a small launch, the tiled kernel family), and bofi_engine_decode_saic return BOFI_ERR_STATE; bofi_engine_logprob returns NULL. */
#define BOFI_FORK_IDS_ONLY 1
int bofi_engine_fork_ex(bofi_engine_t* parent, int max_batch, int fork_flags, bofi_engine_t** out);
/* 1 when a BOFI_FLAG_IDS_ONLY decode of B images would take the fused generator (bofi_vocab_block's kernel) under the current environment knobs -- what a
 * BOFI_FORK_IDS_ONLY fork can serve; 0 otherwise. */
int bofi_engine_ids_only_fused(bofi_engine_t* e, int B);

/* Re-pack the engine's weights from float32 parameters that live on the DEVICE (reference names, as set_weight): the
 * packing of bofi_engine_finalize (q|k|v stacking, LayerNorm folding, compute-dtype cast, bound tables) as kernels on
 * `stream`, into the existing allocations -- captured graphs and forks stay valid.  For a training loop that decodes
 * with its current weights every step (the self-critical phase, periodic evaluation).  Requires a finalized engine. */
int bofi_engine_refresh_device(bofi_engine_t* e, int n, const char* const* names, const float* const* ptrs, const int64_t* numels,
                               void* stream);

/* The options of ONE call of bofi_engine_decode_naic / bofi_engine_decode_saic / bofi_engine_fill_naic, handed to it as `opts` (since ABI version 5).  Nothing of it outlives
 * the call: the next call starts from its own record.  NULL means the defaults, and so does a zero-filled record.  Every rule below is checked before anything is enqueued or
 * captured (BOFI_ERR_ARG with a message); under BOFI_FLAG_GRAPH every field but sample_seed is part of the graph key, so keep the buffers in place across replays. */
typedef struct bofi_call_opts {
    /* Several independent batches in ONE decode call (dynamic batching for serving): with q1_group > 0 the B images of a call are consecutive batches of q1_group
     * images and quirk Q1 (BOFI_FLAG_STRICT_Q1) applies inside each batch, so every batch's result equals its own separate decode.  0: the whole call is one batch. */
    int q1_group;
    /* Bounding iterations a decode_naic enqueues (core_NAIC's loop, TransformerModel.py:1843-1869; 0 = all seq_length).  The loop exits when every image is finished; enqueued
     * iterations past that point return at once but still cost their five launches.  With a cap c the decode is the reference's if and only if the loop ended within c
     * iterations: *bound_iters (iterations in which some image was live) < c.  Otherwise decode again with cap 0.  The persistent loop kernel ends by itself and ignores it. */
    int bound_iter_cap;
    /* The iterations a decode_saic enqueues: saic_it_begin .. saic_it_end of core_SAIC's loop (TransformerModel.py:1903-1984; 1-based, begin 0 reads as 1, end 0 = seq_length:
     * the whole loop).  A call with begin 1 encodes and initialises; one with begin > 1 continues the PREVIOUS call's loop on the state left in the engine's workspace (same
     * arguments, no other decode in between) and exports again: [1, c] followed by [c + 1, seq_length] is the same computation as the whole loop.  Iterations past the last
     * live one return at once but still cost their launches; *bound_iters (live iterations so far) < c after [1, c] means the loop has ended. */
    int saic_it_begin; int saic_it_end;
    /* Temperature (> 0; read only under BOFI_FLAG_SAMPLE) and seed of the token draws of a decode_saic called with BOFI_FLAG_SAMPLE.  The seed travels through device
     * memory, outside the captured launches: a replayed graph draws anew. */
    float sample_temperature; uint64_t sample_seed;
    /* With a pipeline of capped decodes whose results are consumed later: device int32 (NULL = off) that receives, by atomic max, the live-iteration count of this
     * decode_naic -- one read after the last decode tells whether ALL of them ended inside the cap (the caller clears the word first). */
    int* live_max;
    /* fp16 saturation status of the persistent bounding-loop kernel.  That kernel computes the bounding network with FP16 operands (fp16 copies of the float32 parameters,
     * activations converted on their way into the MFMAs) and clamps to +-65 504 on conversion; a model whose bounding layer leaves that range -- none here does: |y| < 30 --
     * would get a silently different slot layout where the bf16 kernels (same exponent range as float32) would not.  Device int32 (NULL = off): the decode_naic WRITES its
     * status there (beside bound_iters): 0 = nothing was clamped (always 0 when the decode ran the five-launch bf16 iterations), bit 0 = an activation (attention context or
     * hidden row of the bounding layer) was clamped during this decode, bit 1 = the fp16 weight copies were clamped when they were packed (finalize / refresh_device), bit 2 =
     * the kernel's pair exchange timed out (two workgroups share a group's feed-forward weights: a safety net against a lost workgroup, never observed).  A caller that reads a
     * non-zero word decodes that batch again under bofi_engine_set_bound_loop(e, 0) (boficap_amd/engine.py does, with a warning).  Replaces nothing in the reference
     * (TransformerModel.py:357-383 runs in float32 there); it guards this library's own precision choice. */
    int* sat_out;
    /* bofi_vocab_stats' two per-position figures straight out of a decode_naic's vocabulary epilogue (no second pass over the [B, S, V] tensor): float32 [B * S] device
     * buffers, both or neither (greedy decodes with log-softmax).  sum_v p log p is formed as sum_v e_v (x_v - max) / sum_v e_v - lse in the pass that sums the exponentials. */
    float* row_plogp; float* row_chosen;
    /* Decodes under BOFI_FLAG_MASK_PREDICT: int32 [B * S] device buffer that receives, per position, the pass (0 .. T) that emitted the token standing there (0 on the
     * pad tail); NULL: off. */
    int* refine_round;
    /* bofi_attn_maps' outputs for decoder layer attn_layer (0 .. N_dec - 1, or -1 = the last; read only when one of the four buffers is given) of a decode_naic / fill_naic's
     * filling pass -- Lq = seq_length, Lk = R, klen = att_len, qlen = tokens laid out -- device buffers attn_mean [B, S, R], attn_heads [B, H, S, R], attn_top_idx / attn_top_w
     * [B, S, K = attn_topk] as there (any of the three groups may be NULL; all NULL: off; K > 0 goes with the top pair, K = 0 with neither).  One extra launch per decode, right behind
     * the layer's cross-attention sublayer, from the queries and keys that sublayer read; it belongs to BOFI_FLAG_PHASE_FILL.  With refinement rounds only the LAST pass launches
     * it: under feed-back that is the final ids' own pass; under BOFI_FLAG_MASK_PREDICT the rows of kept positions are that pass's re-prediction, not the pass that emitted the
     * token (as seq_logprob).  Needs seq_length <= 64 and R <= 128; decode_saic with a buffer given is BOFI_ERR_STATE. */
    int attn_layer; int attn_topk;
    float* attn_mean; float* attn_heads; int* attn_top_idx; float* attn_top_w;
    /* The constrained pick of a decode_naic / fill_naic (bofi_vocab_constrain states the rule; appended within ABI version 5: a record that ends in zeros -- and a caller
     * that zero-fills it -- gets the unconstrained decode, bit for bit, and nothing is launched).  pick_ban: device uint32 [ceil(V / 32)], bit id % 32 of word id / 32 set = id
     * is never emitted (NULL: none; the caller leaves at least two ids unbanned).  pick_no_repeat (0 / 1): a position does not repeat the id of the position before it when that
     * id is >= pick_repeat_min_id (>= 0; a word id: 7 is the first one, so pad / BOS / EOS / the label ids may repeat).  On = a ban table or pick_no_repeat = 1: bofi_vocab_constrain's two launches
     * right behind the vocabulary epilogue of EVERY filling pass, part of BOFI_FLAG_PHASE_FILL -- so feed-back rounds feed the constrained ids back, and the last pass leaves seq and
     * row_chosen those of the emitted ids (row_plogp, a figure of the distribution, stays).  Every pass then stores its log-probs (the pick reads what the pass stored), and the
     * per-image counts of re-picked positions of the last pass are read with bofi_engine_pick_changed.  Under BOFI_FLAG_RAW_LOGITS the pick is over logits.
     * BOFI_ERR_ARG before anything is enqueued: pick_no_repeat outside {0, 1}, pick_repeat_min_id < 0; on together with BOFI_FLAG_IDS_ONLY (no distribution to re-pick from) or
     * BOFI_FLAG_MASK_PREDICT (a kept position would pin both neighbours), or seq_length > 64.  decode_saic with the options on is BOFI_ERR_STATE.
     * BOFI_FLAG_PICK_TRIGRAMS adds block_trigrams to the pick (and turns it on by itself): a per-call flag, not a field -- the record stays 128 bytes. */
    const uint32_t* pick_ban; int pick_no_repeat; int pick_repeat_min_id;
} bofi_call_opts_t;

/* The per-image counts of positions whose id the constrained pick of the LAST filling pass changed (bofi_call_opts_t.pick_*; bofi_vocab_constrain's `changed`), of the most
 * recent decode_naic / fill_naic of this engine that had the options on: copies the first B of them from the engine's workspace to dst (device int32 [B]) on `stream` --
 * the decode's own stream, behind it.  BOFI_ERR_ARG: a NULL engine or dst, B outside 1..max_batch. */
int bofi_engine_pick_changed(bofi_engine_t* e, int* dst, int B, void* stream);

/* A hint, not a semantic: how many decodes the caller keeps in flight on this device (engine + forks on their own streams).  1: this engine's
 * launches run with nothing beside them -- from 4 096 rows on the sublayer kernels then take 64-row blocks (more, shorter workgroups: 62 against 68 us
 * for the encoder's feed-forward sublayer at 11 520 rows) where the default, n = 0 (unknown) or n > 1, takes the 80- / 96-row blocks that move fewer weight
 * bytes per row (+3.5 % images/s with four launches in flight).  Results under either choice agree as bf16 kernels of different summation order do. */
int bofi_engine_set_decodes_in_flight(bofi_engine_t* e, int n);

/* 1 when a bofi_engine_decode_naic of R regions per image would run core_NAIC's bounding loop (TransformerModel.py:1833-1869) as the persistent
 * kernel of round 5 -- one workgroup per 16 images runs every iteration (row-0 self-attention, cross-attention, feed-forward, heads, slot bookkeeping)
 * and leaves when its images are finished; fp16 operands derived from the float32 parameters -- under the engine's current decodes-in-flight hint:
 * bf16 engine at the reference's width (d_model 512, 8 heads, d_ff <= 2048 a multiple of 512, seq_length <= 22, N_len = 1), R <= 128, and the
 * hint is not 1 (a decode that runs alone keeps the five launches per iteration: shorter latency); environment knob BOFI_BOUND_LOOP: 0 = never,
 * 2 = whatever the hint (read again by bofi_reload_env).  The bound-iteration cap (bofi_call_opts_t.bound_iter_cap) does not apply to that kernel.  0 otherwise. */
int bofi_engine_bound_loop_active(bofi_engine_t* e, int R);

/* Between two partial bofi_engine_decode_saic calls: the tokens emitted so far (positions before the end of the last placed phrase) are replaced by
 * seq int64 [B, seq_length] (device memory, the layout of the exported seq), in the emitted caption and in the bounding step's input
 * (extend_phrase_len, TransformerModel.py:1959-1966): the loop continues on the caller's words.  For a caller that draws each phrase itself over the
 * engine's layout -- the self-critical step's reference-estimator mode draws from the TRAINING forward's dropout-perturbed distribution
 * (loss_wrapper.py:193-209 samples in train mode), boficap_amd/trainer.py. */
int bofi_engine_saic_put_words(bofi_engine_t* e, const int64_t* seq, int B, void* stream);
/* Per-engine choice of the bounding loop's form for the following decodes: -1 (default, also of a fork) = BOFI_BOUND_LOOP and the decodes-in-flight hint decide
 * (bofi_engine_bound_loop_active), 0 = the five-launch bf16 iterations, 2 = the persistent fp16 loop kernel whatever the hint.  Part of the graph key. */
int bofi_engine_set_bound_loop(bofi_engine_t* e, int mode);
/* Where the decoder layers' cross K|V -- the columns of the stacked K|V behind the bounding layer's -- are projected (round 7): 1 (default) = BESIDE the bounding loop, in extra
 * workgroups of the loop kernel's own launch, wherever that pays: the loop kernel runs two workgroups per group by the library's own rule (BOFI_BL_PAIR = 1: launches of at most
 * BOFI_BL_PAIR_MAX_B images; not a decode running alone -- the decodes-in-flight hint also sizes the projection's share of the chip, 4 when there is none), at most 36 regions, the row-block encoder with the projection tail, and the decode is one call (a call with BOFI_FLAG_PHASE_* keeps the other
 * form: its ENCODE phase promises the whole stacked K|V).  The encoder's last feed-forward launch then projects the bounding layer's columns only.  0 = never: all columns
 * in front of the loop, as everywhere else.  Every result is the same bits either way: the projection beside the loop takes the LayerNorm row sums in the feed-forward tail's
 * order, so the decoder layers' K|V -- and with them the captions and their log-probabilities -- are the tail's.  A switch for A/B runs and tests, not a knob: per-engine state,
 * part of the graph key, inherited by a fork. */
int bofi_engine_set_bound_kv_beside(bofi_engine_t* e, int mode);
/* 1 when a bofi_engine_decode_naic of B images of R regions called with `flags` would take that form under the engine's current settings; 0 otherwise. */
int bofi_engine_bound_kv_beside_active(bofi_engine_t* e, int B, int R, int flags);

/* Device pointer of the engine's own [max_batch * S, V] float32 log-prob workspace: where a decode called WITHOUT a
 * seq_logprob buffer leaves the distribution (valid until the next decode on this engine) -- input of
 * bofi_vocab_stats / bofi_vocab_sample when the 48.6 MB tensor is not wanted in user memory. */
const float* bofi_engine_logprob(bofi_engine_t* e);

/* A HIP stream owned by the engine (hipStream_t as void*), for callers that keep one decode per engine in
 * flight and want each on its own hardware queue. */
void* bofi_engine_stream(bofi_engine_t* e);

#define BOFI_FLAG_STRICT_Q1 1      /* reproduce TransformerModel.py:1872-1873: every image's fill mask
                                      uses the LAST image's length.  Default ON in the Python wrapper. */
#define BOFI_FLAG_RAW_LOGITS 2     /* output_logsoftmax = 0 (AttModel.py:208-209) */
#define BOFI_FLAG_GRAPH 4          /* replay the call from a captured hipGraph when possible */
#define BOFI_FLAG_SAMPLE 16         /* decode_saic: draw each phrase's tokens from Categorical(logits / temperature) instead of
                                      the argmax (sample_method 'sample'); parameters: bofi_call_opts_t.sample_temperature / sample_seed */
#define BOFI_FLAG_REFINE_SHIFT 8   /* bits 8..11: extra filling rounds; round r > 0 feeds round r-1's ids back as the
                                      decoder input tokens (decode_NA's glat_input, TransformerModel.py:570-574).  The
                                      reference has no refinement loop: parity of rounds > 0 is pinned to the oracle only. */
/* bofi_engine_decode_naic in PHASES (none of the three bits = the whole decode).  A caller that pipelines decodes enqueues the phases of one decode
 * as separate calls on the same engine -- encode, then bound, then fill, ordered by the caller's streams / events -- so that the bounding loop (a few
 * workgroups for ~1 ms) can run on a side stream while the launch stream already encodes the next batch on another fork: */
#define BOFI_FLAG_PHASE_ENCODE 32   /* _prepare_feature + Encoder + the stacked cross K|V (TransformerModel.py:1674-1690, 1332-1336) */
#define BOFI_FLAG_PHASE_BOUND 64    /* the bounding loop of core_NAIC (:1833-1869) on the preceding encode of this engine */
#define BOFI_FLAG_SAIC_LAYOUT_ONLY 4096 /* decode_saic: every enqueued iteration lays its phrase out (bounding step + bookkeeping, TransformerModel.py:1903-1948) and stops there --
                                          no decoder pass, no tokens: the caller draws the phrase's words from its own distribution and hands them back with
                                          bofi_engine_saic_put_words before the next call (the reference-estimator self-critical step) */
#define BOFI_FLAG_PHASE_FILL 128    /* decode_NA + logit + greedy pick + the slot-state export (:570-587, 1872-1876) on the preceding two */
#define BOFI_FLAG_IDS_ONLY 8192     /* decode_naic / fill_naic (phased form included): ids, slot layout and the row statistics of bofi_call_opts_t.row_plogp / row_chosen only -- the
                                       vocabulary distribution is not wanted (seq_logprob must be NULL; not with BOFI_FLAG_RAW_LOGITS).  Where the row-block generator would run
                                       (bf16 engine at the reference's width, launches of BOFI_RB_MIN_ROWS rows or more) every filling round's generator + epilogue is one
                                       bofi_vocab_block launch: no logits in memory; the pick is the first maximum of the raw logits (it can differ from the log-softmax
                                       path's only where two log-probs round to one float32).  Elsewhere the flag is honoured by the generator into the workspace and
                                       the epilogue without its store.  Part of the graph key, as every flag. */
#define BOFI_FLAG_MASK_PREDICT 16384 /* decode_naic / fill_naic (phased form included), only with T = bits 8..11 >= 1: the T extra filling passes are MASK-PREDICT rounds instead
                                       of feed-back rounds.  n_b = last[b] - 1 tokens are laid out for image b.  The state (y, c, e, emitted_round) [B, S] holds per position the
                                       id, the log-prob of that id, sum_v p log p of the row that emitted it, and the pass that did.  Pass 0 is today's (BOS everywhere) and fills
                                       the state.  Pass t = 1 .. T: k = n_b (T + 1 - t) / (T + 1) (integer division); its mask is the k positions s < n_b with the lowest c[s] -- ties go
                                       to the lower position, a NaN ranks below every number, NaNs among themselves by position; its input ids are BOS under the mask and y[s] elsewhere
                                       (s >= n_b: pad, as feed-back); positions in the mask take the pass's id and statistics and emitted_round = t, the others keep the state; s >= n_b
                                       always takes the fresh pass's values (pad, emitted_round 0).  Outputs: seq = y after pass T; bofi_call_opts_t.row_plogp / row_chosen
                                       receive c and e of the STATE (each position's figures come from the pass that emitted its token); seq_logprob, when wanted, is the LAST pass's
                                       tensor -- the rows of kept positions are that pass's re-prediction, not the distribution that emitted the token; emitted_round goes to
                                       bofi_call_opts_t.refine_round.  Costs T + 1 launches of bofi_mask_predict_step's kernel per decode over feed-back.  BOFI_ERR_ARG before any
                                       launch: T = 0, BOFI_FLAG_RAW_LOGITS, BOFI_FLAG_SAMPLE, bofi_engine_decode_saic, seq_length > 64. */
#define BOFI_FLAG_PICK_TRIGRAMS 32768 /* decode_naic / fill_naic (phased form included): block_trigrams on the constrained pick (bofi_vocab_pick states the rule; the reference's
                                       --block_trigrams, AttModel.py:362-388, as a HARD block and on the non-autoregressive path).  The flag alone turns the constrained pick on;
                                       with it the pick of every filling pass is bofi_vocab_pick's two launches (K candidates per row in an engine workspace) with
                                       bofi_call_opts_t.pick_ban / pick_no_repeat / pick_repeat_min_id as given, at the same point and with the same outputs
                                       (bofi_engine_pick_changed included).  The caller's ban table leaves at least seq_length + 1 ids.  Refused as the pick_* fields are, before
                                       anything is enqueued: BOFI_ERR_ARG with BOFI_FLAG_IDS_ONLY, with BOFI_FLAG_MASK_PREDICT or at seq_length > 64; BOFI_ERR_STATE on
                                       bofi_engine_decode_saic.  Without the flag nothing new is launched.  Part of the graph key, as every flag. */

/* model(fc, att, att_masks, opt={'train_mode':'NAIC','sample_method':'greedy'}, mode='sample'):
 * AttModel._sample AttModel.py:307-338,419-429 -> _prepare_feature TransformerModel.py:1674-1690
 * -> Encoder :1332-1336 -> core_NAIC :1823-1876 (bound loop + decode_NA :570-587) -> logit/
 * log_softmax AttModel.py:203-210 -> greedy pick CaptionModel.py:388-390 -> pad tail.
 *   att_feats: feats_dtype [B, R, feat] contiguous;  att_len: int32 [B] regions per image or NULL
 *   seq: int64 [B, S];  seq_logprob: float32 [B, S, vocab] or NULL (then only ids are produced);
 *   phrase_num: int32 [B];  phrase_length: int32 [B, S];  phrase_syn: int64 [B, S];
 *   memory_out: float32 [B, R, d_model] or NULL (encoder output, for _prepare_feature parity);
 *   bound_iters: int32 [1] or NULL (number of bound iterations in which some image was active). */
int bofi_engine_decode_naic(bofi_engine_t* e, const void* att_feats, int feats_dtype, const int* att_len,
                            int B, int R, int flags, int64_t* seq, float* seq_logprob, int* phrase_num,
                            int* phrase_length, int64_t* phrase_syn, float* memory_out, int* bound_iters,
                            const bofi_call_opts_t* opts, void* stream);

/* model(..., opt={'train_mode':'SAIC','sample_method':'greedy'}, mode='sample'): the semi-autoregressive decode
 * core_SAIC TransformerModel.py:1878-1986 (AttModel.py:430-437) -- per phrase one bounding step on the words
 * emitted so far (:1907-1926), the position-wise copy of the previous phrase (:1928-1948), a full decoder
 * pass (decode_SA :520-530) and the copy of the new phrase's tokens and log-probs (:1968-1977); stops
 * when every image is finished or a NaN appears (:1956-1958).  Outputs as for decode_naic
 * (seq_logprob rows never written stay 0, as in the reference).  From the second phrase on only the new phrase's rows go
 * through the decoder's GEMMs (their K / V join a per-layer cache; results identical to the all-rows form).  flags:
 * BOFI_FLAG_RAW_LOGITS, BOFI_FLAG_SAMPLE (opts->sample_temperature / sample_seed; the seed lives in device memory, so a replayed graph
 * draws anew), BOFI_FLAG_GRAPH (captured once per argument set, as decode_naic). */
int bofi_engine_decode_saic(bofi_engine_t* e, const void* att_feats, int feats_dtype, const int* att_len,
                            int B, int R, int flags, int64_t* seq, float* seq_logprob, int* phrase_num,
                            int* phrase_length, int64_t* phrase_syn, int* bound_iters, const bofi_call_opts_t* opts, void* stream);

/* Stages of the call above, exposed for module-level parity tests (SURVEY.md §4 pyramid level 2). */
int bofi_engine_encode(bofi_engine_t* e, const void* att_feats, int feats_dtype, const int* att_len,
                       int B, int R, float* memory_out, void* stream);
/* One bound step from a given slot layout: ext_syn int32 [B, S+2], last int32 [B] ->
 * len_logp float32 [B, 20], syn_logp float32 [B, 10] (LengthPredictor_UIC.forward
 * TransformerModel.py:357-383 on the memory of the preceding bofi_engine_encode). */
int bofi_engine_bound_step(bofi_engine_t* e, const int* ext_syn, const int* last, int B, int R,
                           const int* att_len, float* len_logp, float* syn_logp, void* stream);

/* The row-0 stages of a bounding iteration as operators (bound_ops.hip; bf16, d_model 512, 8 heads): one activation row per image.
 * bofi_rowgemm: y[M, N] = epilogue(x[M, K] . w[N, K]^T), K = 512 * splitk.  stats (may be NULL): partial (sum, sum of squares) of the
 * float32 rows behind x, [M][stats_groups][2] -> the LayerNorm folded into w / bias / colsum (y = rstd (acc - mean colsum) + bias);
 * relu; residual float32 [M, ldr]; outputs: y float32 (splitk > 1: `splitk` partial slabs [splitk][M][ldy], bias and residual in
 * slab 0), yb bf16 copy, stats_out [M][N/16][2] partial sums of the output rows.  Without split-K any K = 512 * c is walked in chunks.
 * skip (may be NULL): the launch returns at once when *skip >= skip_threshold.  row_idx / n_rows (both or neither; device memory): the
 * GEMM covers rows row_idx[0 .. *n_rows) of x (and of residual / stats) and writes the same rows of the outputs; M is then the capacity.
 * bofi_bound_qattn: out[B, 512] = per head softmax(q k^T / 8) v with q = LayerNorm-folded Wq x (as above, stats [B][16][2]), keys and
 * values k, v [B * R, ldkv] (R <= 64 regions per image, att_len int32 [B] or NULL = R each).  row_idx / n_rows (both or neither): the query
 * rows are rows row_idx[0 .. *n_rows) of x / stats / out (B = capacity); with rows_per_image > 0 row r attends the regions of image
 * r / rows_per_image (a decoder layer's cross-attention over the rows of a list). */
int bofi_rowgemm(const void* x, int ldx, const void* w, const float* bias, const float* stats, int stats_groups, const float* colsum,
                 const float* residual, int ldr, float* y, int ldy, void* yb, int ldyb, float* stats_out, int M, int N, int K, int splitk,
                 int relu, const int* skip, int skip_threshold, const int* row_idx, const int* n_rows, void* stream);
int bofi_bound_qattn(const void* x, const float* stats, const void* wq, const float* bias, const float* colsum, const void* k, const void* v,
                     int ldkv, const int* att_len, void* out, int B, int R, const int* skip, int skip_threshold, const int* row_idx,
                     const int* n_rows, int rows_per_image, void* stream);

/* Row-block sublayer kernels (rowblock.hip; bf16 operands, d_model 512): a workgroup keeps a block of activation rows in LDS for a
 * whole sublayer and streams the weights from L2 straight into MFMA operand registers.
 * bofi_pack_frag: w [N, K] row-major bf16 -> the fragment-major layout those kernels stream
 *   ([N/64][K/32][4 tiles][64 lanes][8 bf16]; N % 64 == 0, K % 32 == 0); out holds N*K bf16.
 * bofi_ffn_block: y = x + w_2 relu(w_1 LN(x) + b_1) + b_2 -- PositionwiseFeedForward behind SublayerConnection
 *   (TransformerModel.py:1477-1478, 1361-1377), one launch.  x, y float32 [M, 512] (y may be x); w1p = bofi_pack_frag of the
 *   [dff, 512] weight with the norm's gain folded in, c1 = b_1 + w_1 b_ln, cs1 = column sums of the rounded folded weight
 *   (float32 [dff]: the fold of gemm_glds.hip); w2p = bofi_pack_frag of the [512, dff] weight, b2 float32 [512]; dff % 512 == 0,
 *   dff <= 2560.  Optional outputs (NULL to skip): yb bf16 [M, 512], stats_out float32 [M][16][2] partial (sum, sum of squares)
 *   per 32 columns of y (what a LayerNorm-folded consumer GEMM reads).
 * bofi_attn_block: y = x + W_o concat_h softmax(q_h k_h^T / 8) v_h + b_o -- MultiHeadedAttention (TransformerModel.py:1421-1432,
 *   1454-1467) behind the sublayer's residual, one launch: 8 heads of 64, q [B*Lq, ldq], k / v [B*Lk, ldk / ldv] bf16 (head h at
 *   columns h*64), Lq, Lk <= 48.  Key-prefix masks as bofi_attention: klen int32 (NULL: all Lk keys), entry
 *   klen[bi * klen_sb + q * klen_sq] + klen_bias for query row q of image b, bi = b, or with klen_shared_last = G > 0 the last
 *   image of b's group of G (quirk Q1, TransformerModel.py:1872-1873); a row without keys is NaN as in the reference.
 *   wop = bofi_pack_frag of the [512, 512] output projection, bo float32 [512]; x, y float32 [B*Lq, 512] (y may be x); yb /
 *   stats_out as bofi_ffn_block.
 * bofi_linear_block: y[M, N] = act(W' LN(x) + b) for a LayerNorm-folded projection with K = 512 (the q|k|v, cross-query, stacked cross K|V
 *   and generator projections: TransformerModel.py:1454-1456, AttModel.py:203-210 behind their pre-norms): x float32 [M, 512] -- the
 *   row statistics are computed in the kernel --, wp = bofi_pack_frag of the folded [N, 512] weight (N % 64 == 0), c / cs its folded
 *   bias and column sums, y bf16 or float32 (y_f32) [M, ldy], relu 0 / 1. */
/* bofi_vocab_block: bofi_linear_block(y_f32 = 1) on the generator's weight + bofi_vocab_finalize's log-softmax case + bofi_vocab_stats as ONE launch that never
 *   writes the [M, Npad] logits (AttModel.py:203-210, CaptionModel.py:388-390, AttModel.py:422-423, eval_utils.py:463-464): every logit is the float32 value
 *   bofi_linear_block forms, and each wavefront folds its 64-column chunks into a running (max, sum e, sum e (v - max), first maximal column) per row.
 *   x float32 [M, ldx]; wp / c / cs as bofi_linear_block's for Npad columns (Npad % 64 == 0) of which the first V are the vocabulary (the rest: zero rows, ignored);
 *   seq int64 [M] = the first maximum of the row's V logits (0 if the row holds a NaN), or pad_idx where ntok (int32 [M / S], may be NULL) says so:
 *   position t = row % S of image row / S with t >= ntok[image] + ntok_bias; row_plogp / row_chosen (float32 [M], both or neither): sum_v p log p and the
 *   log-prob of the emitted id (NaN for a NaN row); nan_flag (int32 [1], may be NULL): OR-ed with 1 when a row held a NaN; 0 <= pad_idx < V; alone: 1 = nothing
 *   runs beside this launch.  The results depend on the row alone -- not on M, `alone` or the launch's grid, bit for bit: the reduction tree is fixed by the columns.
 *   The entry keeps a small workspace of its own: calls on different streams must not overlap, and it is not for use inside a stream capture (the engine's
 *   decodes under BOFI_FLAG_IDS_ONLY use a workspace per engine). */
int bofi_vocab_block(const float* x, int ldx, const void* wp, const float* c, const float* cs, int M, int Npad, int V, int S, const int* ntok, int ntok_bias,
                     int pad_idx, int64_t* seq, float* row_plogp, float* row_chosen, int* nan_flag, int alone, void* stream);
int bofi_pack_frag(const void* w, void* out, int N, int K, void* stream);
int bofi_linear_block(const float* x, int ldx, const void* wp, const float* c, const float* cs, void* y, int ldy, int y_f32, int M, int N,
                      int relu, void* stream);
int bofi_attn_block(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, int B, int Lq, int Lk, const int* klen,
                    int klen_sb, int klen_sq, int klen_bias, int klen_shared_last, const void* wop, const float* bo, const float* x,
                    int ldx, float* y, int ldy, void* yb, float* stats_out, void* stream);
/* bofi_attn_linear_block: bofi_attn_block (in place, one key count per image, Lq <= 20, Lk <= 32: the filling pass's self-attention) followed by bofi_linear_block
 *   (N = 512) on its output, ONE launch -- the decoder layer's self-attention sublayer and the LayerNorm-folded query projection of its cross-attention
 *   (TransformerModel.py:1408-1413 around :1454-1456): x as bofi_attn_block's y, pj_y bf16 [B*Lq, pj_ldy] = W_pj' LN(x) + c_pj.  Each 80-row block (four images per
 *   workgroup) is projected while it sits in LDS; the projection differs from the two-launch form in the summation order of the row statistics. */
int bofi_attn_linear_block(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, int B, int Lq, int Lk, const int* klen, int klen_sb,
                           int klen_bias, int klen_shared_last, const void* wop, const float* bo, float* x, int ldx, const void* pj_wp, const float* pj_c,
                           const float* pj_cs, void* pj_y, int pj_ldy, void* stream);
/* (bofi_decoder_attn_block -- both attention sublayers of a decoder layer as one launch, round 5 -- lost 3 % with launches in flight and left the ABI in round 6:
 *   dev/exp/rb_dec_attn_kernel.inc, profiles/r05_dec_attn_fused.txt, last shipped at commit 45884c1.) */
int bofi_ffn_block(const float* x, int ldx, const void* w1p, const float* c1, const float* cs1, const void* w2p, const float* b2,
                   float* y, int ldy, void* yb, float* stats_out, int M, int dff, void* stream);
/* bofi_ffn_linear_block: bofi_ffn_block followed by bofi_linear_block on its output, ONE launch -- the feed-forward sublayer and the
 *   LayerNorm-folded projection that reads the stream next (the next layer's q|k|v, TransformerModel.py:1454-1456 behind :1361-1377; after the
 *   last encoder layer the stacked cross K|V): y as bofi_ffn_block, pj_y bf16 [M, pj_ldy] = W_pj' LN(y) + c_pj (pj_wp / pj_c / pj_cs as
 *   bofi_linear_block's wp / c / cs; pj_N % 64 == 0, pj_N >= 512, pj_ldy % 8 == 0).  Each 80-row block is projected while it is still in LDS. */
int bofi_ffn_linear_block(const float* x, int ldx, const void* w1p, const float* c1, const float* cs1, const void* w2p, const float* b2,
                          float* y, int ldy, int M, int dff, const void* pj_wp, const float* pj_c, const float* pj_cs, void* pj_y,
                          int pj_ldy, int pj_N, void* stream);
/* bofi_attn_out_ffn_block (round 6): the SECOND half of an attention sublayer -- output projection, bias, residual (MultiHeadedAttention.forward's last Linear
 *   TransformerModel.py:1467 behind SublayerConnection :1361-1363) -- as the HEAD segment of the feed-forward sublayer that follows it (:1477-1478; EncoderLayer :1374-1377,
 *   DecoderLayer :1408-1413), ONE launch:   x1 = x + W_o ctx + b_o;   y = x1 + w_2 relu(w_1 LN(x1) + b_1) + b_2   [; pj_y = W_pj' LN(y) + c_pj as bofi_ffn_linear_block]
 *   ctx: bf16 [M, ldc] -- the heads' attention outputs side by side, what bofi_attention writes (the attention CORE: no weights, a light kernel);  wop: W_o [512][512] in
 *   bofi_pack_frag's layout, bo float32 [512];  the rest as bofi_ffn_block / bofi_ffn_linear_block (pj_wp NULL: no projection tail).  x1 never exists in memory: the
 *   kernel's consumer wavefronts start their accumulators from x, run the W_o segment over the staged context block, and keep x1 as the feed-forward's residual.
 *   Equal to bofi_attn_block's W_o half + bofi_ffn_block up to the summation order of the row statistics behind LN(x1).  80-row blocks, one per workgroup. */
int bofi_attn_out_ffn_block(const float* x, int ldx, const void* ctx, int ldc, const void* wop, const float* bo, const void* w1p, const float* c1,
                            const float* cs1, const void* w2p, const float* b2, float* y, int ldy, int M, int dff, const void* pj_wp, const float* pj_c,
                            const float* pj_cs, void* pj_y, int pj_ldy, int pj_N, void* stream);

/* Developer aid: copy one of the engine's buffers into user memory (device to device, on `stream`).  `name` is
 *   - a workspace buffer of the bounding iteration: "by1", "byb", "st_b", "bq2", "bctx2", "by2", "bh", "by3", "dbg_part", "counters" (the caller knows the extent);
 *   - a packed operand, as the last bofi_engine_finalize / bofi_engine_refresh_device left it.  The engine knows these buffers' sizes: asking for more bytes than one
 *     holds is BOFI_ERR_ARG, and so is a field or table that this engine does not have.
 *       "<field>@<prefix>[#k]": field "w" (compute dtype [Npad][K]), "b" (float32 [Npad]: the bias, with a folded LayerNorm's offset), "cs" (float32 [Npad]: column sums,
 *         Linears with a folded LayerNorm only), "wp" (bf16 fragment-major copy of w, bofi_pack_frag's layout; bf16 engine, where kept) or "wp16" (fp16 fragment-major copy
 *         from the float32 parameters: the persistent bounding-loop kernel's operands) of the packed Linear whose FIRST stacked parameter prefix is <prefix>, e.g.
 *         "w@model.encoder.layers.0.self_attn.linears.0" is the encoder's first q|k|v.  Rows N .. Npad are zero padding.  Where several packed Linears start with the same
 *         prefix (the bound layer's self-attention K|V is packed plain for the setup-time tables and once more with sublayer.0.norm folded in), "#k" picks the k-th of them
 *         in the order they were declared, from 0; no suffix is "#0".
 *       "g@<prefix>" / "nb@<prefix>": gain and offset (float32 [d_model]) of the LayerNorm <prefix> (".a_2" / ".b_2").
 *       the bound layer's tables, L = seq_length + 2: "xt" (float32 [L*10][d]), "x0", "x0_sa", "x0b" (float32 [d]), "kvtab" (compute dtype [L*10][2d]), "q0", "q0_sa"
 *         (compute dtype [d]), "votab" (compute dtype [L*10][heads][d]), "w1t" (float32 [d][2*head_hidden]), "w1p" (compute dtype, w1t permuted), "b1" (float32
 *         [2*head_hidden]), "len_w2" / "len_b2" / "syn_w2" / "syn_b2" (float32), and -- where the persistent bounding-loop kernel's operands exist -- "q0_32" (float32 [d]),
 *         "sctab" (float32 [L*10][heads]), "vtab" (float32 [L*10][d]), "wsat" (int32 [1]: an fp16 weight copy was clamped). */
int bofi_engine_debug_copy(bofi_engine_t* e, const char* name, void* dst, int64_t bytes, void* stream);

/* Measurement aid: GEMM FLOPs (2 M N K per launch of bofi_linear* / the weight-gradient GEMMs, engine calls included) enqueued
 * by this process since the last reset; host-side tally, not thread-safe.  Launches that carry an early-out word (loop
 * iterations that return at once when every image is finished) are tallied apart, into *skippable (may be NULL).
 * bench.py prices the EXECUTED work of a step with it. */
double bofi_gemm_flops(int reset, double* skippable);

/* The filling pass alone on a GIVEN slot layout (teacher-forced): decode_NA TransformerModel.py:570-587 -> logit /
 * log_softmax AttModel.py:203-210 -> greedy pick CaptionModel.py:388-390 -> pad tail AttModel.py:422-423, on the memory of
 * the preceding bofi_engine_encode.  ext_syn int32 [B, S+2] (extend_phrase_syn of core_NAIC :1829: position 0 = [LEN],
 * placed slots = their label), last int32 [B] (1 + tokens laid out).  flags: BOFI_FLAG_STRICT_Q1 / RAW_LOGITS / refinement
 * rounds as for decode_naic.  Lets a reduced-precision engine be compared with the oracle position by position on the
 * oracle's own layout, whatever its own bounding pass would have picked. */
int bofi_engine_fill_naic(bofi_engine_t* e, const int* ext_syn, const int* last, int B, int R, const int* att_len, int flags,
                          int64_t* seq, float* seq_logprob, const bofi_call_opts_t* opts, void* stream);

/* CIDEr-D reward of the self-critical step (get_scores, captioning/utils/rewards.py:86-131, with the CiderD scorer of the
 * pyciderevalcap package), in fp64.  A row's token list is its ids up to and including the first 0, or the whole row if it has
 * none (array_to_str, rewards.py:33-39); ids lie in [0, 65534].  An n-gram (n = 1..4) is keyed by its ids packed as (id + 1) into
 * 16-bit fields of a uint64, first token in the highest used field.  df_keys uint64 [n_df] sorted ascending, unique; df_vals
 * double [n_df] = L - log(max(1, df)); an n-gram absent from the table takes the value L = log_ref_len.
 *
 * bofi_cider_refs: the records of n_refs reference rows.  ref_tok int32 [n_refs, width] (width <= 64), ref_len int32 [n_refs] =
 * each row's token count (the first-0 rule applied by the caller).  Record of row r: rec_keys [r, stride] its sorted unique
 * n-grams (unused tail = ~0), rec_w [r, stride] their weights tf * value, rec_off int32 [r, 5] the first n-gram of each order
 * and the count, rec_meta double [r, 5] the four norms and the length (number of bigrams).  stride 128 or 256, >= the n-grams
 * of a width-token row.
 *
 * bofi_cider_score: out float32 [N] (and out64 double [N] unless NULL) = weight * CIDEr-D of candidate j = row j of seq int64
 * [N, S] (S <= 64) against the references ref_start[j / seq_per_img] .. ref_start[j / seq_per_img + 1] - 1 (ref_start int32
 * [N / seq_per_img + 1], every image with at least one reference), the records of bofi_cider_refs on the same stream.
 * cand_len int32 [N] or NULL: the candidates' token counts instead of the first-0 rule.  A candidate with an id outside
 * [0, 65534] scores NaN.  Length penalty exp(-(len_h - len_r)^2 / (2 sigma^2)).  Deterministic: a fixed summation order. */
int bofi_cider_refs(const int* ref_tok, const int* ref_len, int n_refs, int width, const uint64_t* df_keys, const double* df_vals, int n_df,
                    double log_ref_len, uint64_t* rec_keys, double* rec_w, int* rec_off, double* rec_meta, int stride, void* stream);
int bofi_cider_score(const int64_t* seq, const int* cand_len, int N, int S, int seq_per_img, const int* ref_start, const uint64_t* df_keys,
                     const double* df_vals, int n_df, double log_ref_len, double sigma, double weight, const uint64_t* rec_keys,
                     const double* rec_w, const int* rec_off, const double* rec_meta, int stride, float* out, double* out64, void* stream);

/* The whole reward of get_scores: cider_weight * CIDEr-D + bleu_weight * BLEU-4 (the Bleu(4) scorer of the pycocoevalcap package,
 * option 'closest'), in fp64, on the token lists, keys and df table of the CIDEr-D pair above.
 *
 * bofi_reward_refs: the records of bofi_cider_refs, and with them rec_cnt int32 [n_refs, stride] (each unique n-gram's raw count,
 * 0 in the unused tail) and rec_len int32 [n_refs] (each row's token count).  rec_cnt and rec_len are both given or both NULL.
 *
 * bofi_reward_score: out float32 [N] (and out64 double [N] unless NULL) = cider_weight * CIDEr-D + bleu_weight * BLEU-4 of candidate j
 * against its image's references (seq, cand_len, ref_start, sigma as for bofi_cider_score), the records of bofi_reward_refs on the same
 * stream.  BLEU-4 with T candidate tokens: correct[k] = sum over the candidate's unique (k+1)-grams of min(count, max over the references
 * of their count), guess[k] = max(0, T - k), reflen = the reference length closest to T (a tie goes to the shorter); b = product over
 * orders <= k of (correct + 1e-15) / (guess + 1e-9), BLEU-(k+1) = b^(1/(k+1)), times exp(1 - 1/ratio) if ratio = (T + 1e-15) / (reflen
 * + 1e-9) < 1.  comps int32 [N, 10] or NULL: (T, reflen, guess[4], correct[4]) of every candidate, for a corpus score.
 * cider_weight 0 skips the CIDEr-D work (n_df may be 0); with bleu_weight 0 the value is bofi_cider_score's, bit for bit.  A candidate
 * with an id outside [0, 65534] scores NaN.  Deterministic: a fixed summation order. */
int bofi_reward_refs(const int* ref_tok, const int* ref_len, int n_refs, int width, const uint64_t* df_keys, const double* df_vals, int n_df,
                     double log_ref_len, uint64_t* rec_keys, double* rec_w, int* rec_off, double* rec_meta, int* rec_cnt, int* rec_len, int stride,
                     void* stream);
int bofi_reward_score(const int64_t* seq, const int* cand_len, int N, int S, int seq_per_img, const int* ref_start, const uint64_t* df_keys,
                      const double* df_vals, int n_df, double log_ref_len, double sigma, double cider_weight, double bleu_weight,
                      const uint64_t* rec_keys, const double* rec_w, const int* rec_off, const double* rec_meta, const int* rec_cnt,
                      const int* rec_len, int stride, float* out, double* out64, int* comps, void* stream);

/* ROUGE-L of the validation pass (the Rouge scorer of the pycocoevalcap package, beta = 1.2) on id token lists, in fp64.  For candidate j =
 * row j of seq int64 [N, S] (S <= 64) and the references i of its image (ref_start as for bofi_cider_score; ref_tok int32 [n_refs, width],
 * ref_len int32 [n_refs] as for bofi_cider_refs, width <= 64): lcs_i = the longest common subsequence of the two token lists,
 * p = max_i lcs_i / |c|, r = max_i lcs_i / |r_i|, out64[j] = (1 + beta^2) p r / (r + beta^2 p) if p and r are non-zero, else 0; an empty
 * candidate or reference gives its pair p = r = 0.  The candidate's token list: cand_len[j] ids, or (cand_len NULL) the ids up to and
 * including the first 0 (eval_rule 0, array_to_str) or before the first id <= 0 (eval_rule 1, decode_sequence), else the whole row.
 * lcs int32 [seq_per_img * n_refs] or NULL: lcs_i of every pair, candidate j's at ref_start[img] * seq_per_img + (j % seq_per_img) * (the
 * image's references) + i.  best int32 [N, 2] or NULL: the reference (index within the image) that gives p and the one that gives r, the
 * lowest index on ties.  All counts are integers; deterministic. */
int bofi_rouge_score(const int64_t* seq, const int* cand_len, int N, int S, int seq_per_img, const int* ref_start, const int* ref_tok,
                     const int* ref_len, int width, int eval_rule, double beta, double* out64, int* lcs, int* best, void* stream);

/* Diversity of the n sampled captions of every image (n consecutive rows of seq int64 [images * n, S], 2 <= n <= 16, S <= 64), in fp64 on the
 * records, keys and df table of the CIDEr-D pair above.  Token list of a row: eval_rule 0 = the ids up to and including the first 0
 * (array_to_str), eval_rule 1 = the ids before the first id <= 0 (decode_sequence, possibly none), else the whole row.
 *   mat double [images, n, n] or NULL: M[i][j] = 1/4 sum over the orders k of cos_k(i, j), cos_k = sum over the shared k-grams of w_i w_j /
 *     (norm_k(i) norm_k(j)), 0 if either norm is 0 -- plain CIDEr between two samples, no clipping, no length penalty; exactly symmetric.
 *   score double [images]: -log(sqrt(l_max) / sum sqrt(l)) / log n over the eigenvalues l of M clipped below at 0 (get_self_cider_scores,
 *     captioning/utils/rewards.py:119-139), by a cyclic Jacobi iteration with a fixed rotation order and a fixed cap of sweeps; NaN where every
 *     eigenvalue clips to 0, i.e. M = 0: all samples empty (eval_rule 1), or no sample with an n-gram of non-zero weight (e.g. rows of
 *     the id 0 alone under eval_rule 0 when the df table gives the n-gram (0) a document frequency of ref_len); NaN too where a sample holds
 *     an id above 65534 (or, eval_rule 0, below 0).
 *   div int32 [images, 3]: distinct unigrams, distinct bigrams and tokens over the image's samples (Div-n = distinct n-grams / tokens).
 *   comps int32 [images * n, 10] or NULL: (T, reflen, guess[4], correct[4]) of sample i as BLEU candidate against the image's other n - 1
 *     samples, the layout and rules of bofi_reward_score (mBLEU).
 * workspace: bofi_diversity_workspace(images, n, S) bytes (-1 for sizes the kernel refuses), 8-byte aligned, the records' scratch.
 * Deterministic: fixed summation and rotation orders. */
int64_t bofi_diversity_workspace(int images, int n, int S);
int bofi_diversity_score(const int64_t* seq, int images, int n, int S, int eval_rule, const uint64_t* df_keys, const double* df_vals, int n_df,
                         double log_ref_len, void* workspace, int64_t workspace_bytes, double* score, double* mat, int* div, int* comps,
                         void* stream);

/* Oracle and average language scores of every image's n sampled captions (the reference's --eval_oracle 1), in fp64, from the per-candidate
 * outputs of bofi_reward_score and bofi_rouge_score at seq_per_img = n: row m * n + i is sample i of image m, 1 <= n <= 64.
 *   comps int32 [images * n, 10]: bofi_reward_score's counts (testlen, reflen, guess[4], correct[4]); cider, rouge double [images * n].
 *   sent double [images * n, 6] or NULL: the sentence-level Bleu_1, Bleu_2, Bleu_3, Bleu_4 (bleu_scorer.py's compute_score on the row's
 *     counts, option 'closest': the arithmetic of bofi_reward_score's BLEU-4, every order kept), ROUGE_L, CIDEr.
 *   stats double [images, 6, 2]: per metric (oracle, avg) = (the maximum over the n samples, their sum in index order / n).
 *   pick int32 [images, 6]: the lowest sample index that attains the oracle.
 * A NaN among an image's n values of a metric (a CIDEr of a row with an id above 65534) makes that oracle and avg NaN and the pick -1.
 * images = 0 is BOFI_OK without a launch.  Maximum and index are exact, the sum has a fixed order: deterministic. */
int bofi_oracle_stats(const int* comps, const double* cider, const double* rouge, int images, int n, double* sent, double* stats, int* pick,
                      void* stream);

/* The region side of the loader's collate (captioning/data/dataloader.py:326-338: zero-padded features + region counts) and its optional
 * norm_att_feat (:475-476: x / ||x||_2 per region), from a batch staged ragged.
 *   rows: rows_dtype [offsets[B], F], the images' real region rows back to back; rows_dtype BOFI_DT_F32, BOFI_DT_BF16 or BOFI_DT_F16
 *   offsets: int32 [B + 1], non-decreasing, offsets[0] = 0; offsets_host: the host's copy of the same array or NULL
 *   out: out_dtype [B, out_R, F] contiguous (BOFI_DT_F32 or BOFI_DT_BF16); rows and out 16-byte aligned, F % 8 == 0
 *   att_len: int32 [B] or NULL: len_b = offsets[b + 1] - offsets[b]
 * Row r < len_b of image b is the image's row (divided by its norm when norm = 1) in out_dtype, rows len_b <= r < out_R are +0.0: EVERY
 * element of out is written.  f16 -> f32 is exact, -> bf16 rounds the float32 value to nearest even.  norm: squares summed in float32 in a
 * fixed order (no atomics: bit-identical run to run), sqrtf, one division per element; a row of zeros is NaN in every element (0 / 0, as
 * numpy).  B < 1, F % 8 != 0, an unknown dtype, and -- checked on offsets_host, when given -- offsets[0] != 0, decreasing offsets or
 * len_b > out_R are BOFI_ERR_ARG with a message and NOTHING is launched.  The kernel clamps len_b to [0, out_R] whatever the device array
 * holds, so it never writes outside out.  One launch, no synchronisation. */
int bofi_pack_regions(const void* rows, int rows_dtype, const int* offsets, const int* offsets_host, int B, int F, void* out, int out_dtype,
                      int out_R, int norm, int* att_len, void* stream);

/* bofi_pack_regions for the loader's use_box mode (dataloader.py:477-487): behind an image's F_att attention columns stand five geometry columns
 * of its boxes, and the image's rows are sorted by the last of them, largest first.  One launch, no synchronisation.
 *   rows, rows_dtype, offsets, offsets_host, att_len: as bofi_pack_regions, with F_att (a multiple of 8) columns
 *   boxes: float32 [offsets[B], 4] = (x1, y1, x2, y2) in pixels, ragged by the same offsets, 16-byte aligned
 *   wh: int32 [B, 2] = (width, height) on the device; wh_host: the host's copy of it or NULL
 *   out: out_dtype [B, out_R, F_out] contiguous, 1 <= out_R <= 1024, F_out % 8 == 0 and F_out >= F_att + 5 (2112 for 2048 + 5)
 * A real row of image b holds, in float32 before out_dtype's rounding:
 *   columns 0 .. F_att - 1: what bofi_pack_regions writes (norm_att = its norm);
 *   columns F_att .. F_att + 4: x1 / w, y1 / h, x2 / w, y2 / h, ((x2 - x1) * (y2 - y1)) / (float)((int64)w * h) -- one correctly rounded float32 operation
 *     each, in that order -- and with norm_box = 1 each of the five divided by sqrtf(((((c0^2 + c1^2) + c2^2) + c3^2) + c4^2)), every square and every
 *     sum rounded on its own (no fma, no reciprocal): numpy's float32 arithmetic for the loader's expressions;
 *   columns F_att + 5 .. F_out - 1: +0.0.
 * Order: source row i goes to row rank_i = #{j : key_j > key_i} + #{j < i : key_j == key_i}, key = the float32 value of the last box column (after
 * norm_box, never rounded to out_dtype): descending and stable, Python's sorted(..., reverse=True).  A NaN key ranks after every number, NaNs among
 * themselves in source order.  The ranks of an image are a permutation of 0 .. len_b - 1; rows len_b .. out_R - 1 are +0.0: EVERY element of out is
 * written exactly once.  Deterministic (no atomics).  BOFI_ERR_ARG with a message, nothing launched: a NULL among rows / boxes / wh / offsets / out,
 * misalignment, an unknown dtype, B < 1, F_att % 8 != 0, a bad F_out, out_R outside 1..1024, and -- on the host copies, when given -- bad offsets
 * (as bofi_pack_regions) or a width or height < 1.  The kernel clamps len_b to [0, out_R] and every rank to len_b - 1, so it never writes outside out. */
int bofi_pack_regions_box(const void* rows, int rows_dtype, const float* boxes, const int* wh, const int* wh_host, const int* offsets,
                          const int* offsets_host, int B, int F_att, void* out, int out_dtype, int out_R, int F_out, int norm_att, int norm_box,
                          int* att_len, void* stream);

/* The step between two passes of a mask-predict refinement (BOFI_FLAG_MASK_PREDICT states the rules), on given arrays; all buffers [B, S], S <= 64.
 *   ids int64, chosen / plogp float32, round int32: the state (y, c, e, emitted_round), read and written.
 *   fresh_ids / fresh_chosen / fresh_plogp: what pass t left (ids after the pad-tail rule, the log-prob of each id, sum_v p log p).
 *   mask int32: in, the mask of pass t (not read at t = 0: every position is taken); out when t < T, the mask of pass t + 1 (1 = re-predict).
 *   next_ids int64: out when t < T, the input ids of pass t + 1 (bos_idx under the mask, the state's id elsewhere).
 *   last int32 [B]: 1 + tokens laid out (n_b = last[b] - 1, clamped to 0 .. S).
 *   seq_out int64, plogp_out / chosen_out float32 (both or NULL), round_out int32 (or NULL): written when t = T only, the state after the merge.
 * B < 1, S outside 1..64, not 0 <= t <= T <= 15, a NULL among state / fresh / mask / next_ids / last, a NULL seq_out at t = T: BOFI_ERR_ARG, nothing is launched.
 * One launch, one wavefront per image, comparisons only: deterministic. */
int bofi_mask_predict_step(int64_t* ids, float* chosen, float* plogp, int* round, const int64_t* fresh_ids, const float* fresh_chosen,
                           const float* fresh_plogp, int* mask, int64_t* next_ids, const int* last, int B, int S, int t, int T, int bos_idx,
                           int pad_idx, int64_t* seq_out, float* plogp_out, float* chosen_out, int* round_out, void* stream);

/* Word-to-region attention maps: the cross-attention probabilities the fused attention sublayers never leave in memory (the reference keeps them as
 * MultiHeadedAttention.attn, TransformerModel.py:1459), from the queries and keys such a sublayer reads.  d_k = 64.
 *   q [B * Lq rows, pitch ldq elements], k [B * Lk rows, pitch ldk]: `dtype` BOFI_DT_F32 or BOFI_DT_BF16; head h is columns 64 h .. 64 h + 63 (ldq, ldk >= 64 H).
 *   klen int32 [B] or NULL: keys per image (clamped to 0 .. Lk; NULL: Lk).  qlen int32 [B] or NULL, qlen_bias: query rows that carry a word, qlen[b] + qlen_bias (NULL: Lq).
 *   A[b,h,t,r] = softmax over r < len_b of (q[b,t,h,:] . k[b,r,h,:] * scale); +0.0 for len_b <= r < Lk.  A row whose scores hold a NaN (or +infinity) is NaN in ALL
 *                its Lk entries, as the reference's softmax over the masked scores leaves it.  The engine's attention kernels apply scale = 1 / sqrt(64) themselves
 *                (it is not folded into the query projection), so that is what the engine passes.
 *   mean  float32 [B, Lq, Lk] or NULL:  M = (A[b,0] + A[b,1] + ... in head order) / H.
 *   heads float32 [B, H, Lq, Lk] or NULL:  A.
 *   top_idx int32 / top_w float32 [B, Lq, K], both or NULL, 0 <= K <= 8: the K largest entries of M[b,t,:len_b] in descending order, equal weights by lower region
 *                index, top_w = M's own floats bit for bit; slots j >= len_b: (-1, 0); a row of M with a NaN: (-1, NaN) in every slot; rows t >= qlen[b] + qlen_bias:
 *                (-1, 0) -- M and A are written for those rows all the same.
 * Every element of every given buffer is written.  float32 throughout from the inputs as stored, max-subtracted exp, fixed summation orders, no atomics: deterministic.
 * BOFI_ERR_ARG with a message and no launch: B < 1, H < 1, Lq outside 1..64, Lk outside 1..128, K outside 0..8, an unknown dtype, NULL q or k, a pitch below 64 H,
 * no output buffer, one of top_idx / top_w without the other, K > 0 without them, H so large that one query row's share of LDS exceeds 144 KB.
 * One launch: a workgroup per image, a wavefront per head. */
int bofi_attn_maps(const void* q, int ldq, const void* k, int ldk, int dtype, int B, int H, int Lq, int Lk, float scale, const int* klen,
                   const int* qlen, int qlen_bias, float* mean, float* heads, int K, int* top_idx, float* top_w, void* stream);

/* The constrained pick behind the vocabulary epilogue: banned ids (the reference's suppress_UNK, CaptionModel.py:151-153, and any id list) and "never the same word twice in a
 * row" (its decoding_constraint, AttModel.py:325-329) for the non-autoregressive filling pass, where the reference applies neither.  Re-picks every live position of every
 * image; the distribution is read only.
 *   x float32 [rows, ldx], ldx >= V: log-probs or raw logits; row b * S + s is position s of image b; rows need 4-byte alignment only.  1 <= S <= 64.
 *   n_b = clamp(ntok[b] + ntok_bias, 0, S) live positions of image b (ntok int32 [rows / S]; NULL: all S).  Rows past n_b are not read.
 *   ban_bits device uint32 [(V + 31) / 32] or NULL: bit i % 32 of word i / 32 set = id i is banned.  The caller leaves at least two ids unbanned.
 *   Order: id a comes before id c when x[a] is NaN and x[c] is not; else, neither NaN, when x[a] > x[c]; ties -- +0.0 against -0.0, NaN against NaN -- go to the lower id
 *   (torch.max's rule, as bofi_vocab_finalize).  The pick of position s < n_b is the first ELIGIBLE id in that order: not banned, and no_repeat == 0 or s == 0 or
 *   prev < repeat_min_id or id != prev, where prev is the constrained pick of position s - 1 of the same image (a sequential scan over each row's two best unbanned ids).
 *   seq int64 [rows]: read (the ids that stand there) and written: the pick for s < n_b, pad_idx for s >= n_b.
 *   row_chosen float32 [rows] or NULL: x[row, pick] for s < n_b; untouched past n_b.
 *   changed int32 [rows / S] or NULL: per image, the positions s < n_b whose pick differs from the id that stood in seq on entry.
 * Deterministic: no atomics, no float arithmetic, exact comparisons.  rows = 0 is BOFI_OK without a launch.  BOFI_ERR_ARG with a message and no launch: NULL x or seq,
 * rows % S != 0, V < 2, ldx < V, S outside 1..64, no_repeat outside {0, 1}, repeat_min_id < 0.
 * Two launches: a workgroup of four wavefronts per live row streams its V floats (16-byte loads behind a peel to the row's first 16-byte boundary, ban bits staged in LDS)
 * and leaves the row's two candidate ids packed in seq[row]; then one wavefront per image runs the scan.  No workspace. */
int bofi_vocab_constrain(const float* x, int ldx, int rows, int V, int S, const int* ntok, int ntok_bias, int pad_idx, const uint32_t* ban_bits, int no_repeat,
                         int repeat_min_id, int64_t* seq, float* row_chosen, int* changed, void* stream);

/* bofi_vocab_constrain's K-candidate form, with block_trigrams.  Arguments, order, ban table, no_repeat and repeat_min_id are bofi_vocab_constrain's; in addition, with
 * block_trigrams = 1: p[0 .. s-1] being the constrained picks of the image's earlier live positions, id c is TRIGRAM-BLOCKED at position s when s >= 3 and there is a j
 * with 2 <= j <= s - 1, p[j-2] == p[s-2], p[j-1] == p[s-1] and p[j] == c, all three ids of that trigram >= repeat_min_id (words; pad / BOS / EOS / label ids never form a
 * blocked trigram).  Position s takes the first id in the order that is not banned, not excluded by no_repeat and not trigram-blocked.  The blocked set is the reference's
 * (AttModel.py:362-388 records (seq[t-3], seq[t-2]) -> seq[t-1] from t = 3 and looks (seq[t-2], seq[t-1]) up); the block is HARD where the reference adds a penalty
 * ("alpha -> infty works best" there), which keeps the pick free of float arithmetic.
 *   work / work_bytes: a device workspace of at least bofi_vocab_pick_workspace(rows) bytes (int32 [rows, K], K a compile-time constant <= 8), 4-byte aligned.
 *   seq keeps the ids that stood there until the scan overwrites them: `changed` counts against those.
 * The result is the rule's for EVERY input: where all the candidates known of a row are ineligible the image's wavefront streams that one row again for the next ids behind them,
 * under the same order, until one is eligible.  A row with no eligible id at all gets pad_idx (never an id outside the vocabulary): the caller's ban table leaves at least
 * S + 1 ids when block_trigrams is on.  With block_trigrams = 0 the outputs equal bofi_vocab_constrain's.
 * BOFI_ERR_ARG with a message and no launch: what bofi_vocab_constrain refuses, block_trigrams outside {0, 1}, rows > 0 with a NULL or too small workspace.
 * Two launches, deterministic, no atomics, no float arithmetic. */
int64_t bofi_vocab_pick_workspace(int rows);
int bofi_vocab_pick(const float* x, int ldx, int rows, int V, int S, const int* ntok, int ntok_bias, int pad_idx, const uint32_t* ban_bits, int no_repeat,
                    int block_trigrams, int repeat_min_id, int64_t* seq, float* row_chosen, int* changed, void* work, int64_t work_bytes, void* stream);

/* Required words: the best caption that CONTAINS the given ids, from the rows of a filling pass -- the positive counterpart of the constrained pick (lexically constrained
 * captioning; an autoregressive model needs a constrained beam for it, a pass that scores every position on its own solves it exactly as an assignment of K <= 8 words to
 * n <= 64 positions).  A stand-alone launch behind the decode call: no field of bofi_call_opts_t, no engine state, the ABI version is unchanged.
 * For image b:
 *   n_b = clamp(ntok[b] + ntok_bias, 0, S) live positions (ntok NULL: S); x[p, .] the float32 row b * S + p of x [rows, ldx] (log-probs, or raw logits: the normaliser
 *   cancels within a position), read only, any 4-byte alignment; seq[p] the id standing at position p on entry (the greedy or constrained pick of the last filling pass);
 *   words[b, 0 .. K-1] an int32 row, 1 <= K <= BOFI_REQUIRE_MAX.
 * Entries of words[b, .]: an entry < 0 is EMPTY (pos -1).  An entry is SKIPPED (pos -2) when it is >= V, banned by ban_bits (bofi_vocab_constrain's table; NULL: none) or
 * repeats an earlier entry of the same row.  Every other entry is a required word f_j.
 * Gain: gain[p][j] = 0 when seq[p] == f_j; otherwise (double)x[p, f_j] - (double)x[p, seq[p]] when both operands are finite; otherwise position p is INELIGIBLE for word j
 * (NaN and +-inf on either side; a seq[p] outside 0..V-1 has no value and counts as not finite).  With no_repeat = 1 and f_j >= repeat_min_id, p is also ineligible for j
 * when seq[p] != f_j and a live neighbour on entry (seq[p-1] or seq[p+1]) equals f_j: a placement never creates an adjacent repeat.
 * Objective: a placement maps a subset of the required words injectively to eligible live positions; it first maximises the NUMBER of words placed, then the total gain,
 * formed by the backward recurrence below in float64.
 * Recurrence and tie-break: best[n_b][m] = (0 words, 0.0) for every mask m of still-unplaced words.  For p = n_b - 1 .. 0 and each mask m the options are taken in this
 * order: "position p takes word j" for j ascending over the eligible words in m, value (1 + cnt, gain[p][j] + tot) of best[p+1][m \ j]; then "position p keeps its id",
 * value best[p+1][m].  Option values compare first by count, then by total; the FIRST option that attains the maximum is choice[p][m] (update only on strictly greater, in
 * that order).  The result is the forward walk from (0, all required words) along choice -- reading left to right, a position takes a word whenever some optimal
 * completion does, the earliest-listed such word first.
 * Outputs: seq -- live positions that took a word hold it, all else is untouched, the pad tail included; row_chosen (may be NULL) -- x[p, f_j] at every position that took
 * a word, all else untouched; pos int32 [B, K] -- the position of each word, -1 empty, -2 skipped, -3 required but unplaceable; moved int32 [B] (may be NULL) -- positions
 * whose id changed.
 * One launch, no workspace, deterministic, no atomics; the only float arithmetic is the float64 differences and sums above, in the order above.  rows = 0 is BOFI_OK
 * without a launch.  BOFI_ERR_ARG with a message and no launch: NULL x, seq, words or pos; rows % S != 0; V < 2 or ldx < V; S outside 1..64; K outside 1..8; no_repeat
 * outside {0, 1}; repeat_min_id < 0. */
#define BOFI_REQUIRE_MAX 8
int bofi_vocab_require(const float* x, int ldx, int rows, int V, int S, const int* ntok, int ntok_bias, const int* words, int K, const uint32_t* ban_bits, int no_repeat,
                       int repeat_min_id, int64_t* seq, float* row_chosen, int* pos, int* moved, void* stream);

/* Required PHRASES: bofi_vocab_require with multi-word UNITS in place of single ids -- "fire hydrant", a product term, a novel-object name: the ids of a unit are placed
 * side by side and in order, on the contiguous span where they cost the least log-prob.  Still exact: a unit covers a span, so the state at position p reaches back to
 * p + len instead of p + 1.  A stand-alone launch behind the decode call, as bofi_vocab_require: no field of bofi_call_opts_t, no engine state, the ABI version is unchanged.
 * Inputs: bofi_vocab_require's (x, ldx, rows, V, S, ntok, ntok_bias, ban_bits, no_repeat, repeat_min_id, seq; n_b = clamp(ntok[b] + ntok_bias, 0, S)), except the table:
 *   units[b, 0 .. K-1, 0 .. L-1] int32, 1 <= K <= BOFI_REQUIRE_MAX, 1 <= L <= BOFI_REQUIRE_UNIT_MAX.  The length len_j of unit j is its run of leading ids >= 0; the
 *   entries after the first negative id are not read as ids.  u_0 .. u_{len_j - 1} are its ids.
 * Units of a row, classified per image: unit j is EMPTY (pos -1) when its first id is < 0.  It is SKIPPED (pos -2) when one of its ids is >= V; one of its ids is banned by
 * ban_bits; it equals an earlier unit of the row (same length, same ids); and, with no_repeat = 1: it holds two equal adjacent ids >= repeat_min_id; its first id (>=
 * repeat_min_id) equals the last id of an earlier KEPT unit of the row; or its last id (>= repeat_min_id) equals the first id of an earlier kept unit.  Every other unit is
 * kept.  The last two cases exist because two placed units could otherwise meet and form an adjacent repeat: excluding exactly that would need the previously placed unit as
 * recurrence state -- K times the state, which at K = 8 does not fit the 64 KB of LDS of a workgroup.  The host side (require_unit_table) refuses such a pair by name.
 * Span "unit j starts at p": it needs p + len_j <= n_b.  Position p + i (i < len_j) contributes 0 where seq[p+i] == u_i on entry; otherwise (double)x[p+i, u_i] -
 * (double)x[p+i, seq[p+i]] when both operands are finite; anything else makes the span INELIGIBLE (NaN, +-inf, a seq[p+i] outside 0..V-1).  With no_repeat = 1 the span
 * is also ineligible when u_0 >= repeat_min_id, seq[p] != u_0 and the live left neighbour holds u_0 on entry (p > 0, seq[p-1] == u_0), or when u_last >= repeat_min_id,
 * seq[p+len_j-1] != u_last and the live right neighbour holds u_last on entry (p + len_j < n_b, seq[p+len_j] == u_last): a placement never creates an adjacent repeat.
 * gain[p][j] is the float64 sum 0.0 + t_0 + t_1 + ... of the span's per-position terms, left to right.
 * Recurrence and tie-break: best[n_b][m] = (0 units, 0.0) for every mask m of kept units still to place.  For p = n_b - 1 .. 0 and each m the options are taken in this
 * order: "p takes unit j" for j ascending over the units of m with an eligible span, value (1 + cnt, gain[p][j] + tot) of best[p + len_j][m \ j]; then "p keeps its id",
 * value best[p+1][m].  Option values compare first by count, then by total; the FIRST option that attains the maximum is choice[p][m].  The result is the forward walk
 * from (0, all kept units) along choice, which advances by len_j over a placed span.  For L = 1 (and for units of length 1) this is bofi_vocab_require's rule, bit for bit.
 * Outputs: seq -- rewritten on the placed spans, all else untouched; row_chosen (may be NULL) -- x[p+i, u_i] at every span position, all else untouched; pos int32 [B, K]
 * -- the START position of each unit, -1 empty, -2 skipped, -3 kept but not placeable; moved int32 [B] (may be NULL) -- positions whose id changed.  x is read only.
 * The entry point is total: any table contents, any ntok and ids outside the vocabulary in seq give the rule's result, with no read out of range.
 * One launch, no workspace, deterministic, no atomics; the only float arithmetic is the float64 differences and sums above, in the order above.  rows = 0 is BOFI_OK
 * without a launch.  BOFI_ERR_ARG with a message and no launch: what bofi_vocab_require refuses (units in place of words), L outside 1..4. */
#define BOFI_REQUIRE_UNIT_MAX 4
int bofi_vocab_require_units(const float* x, int ldx, int rows, int V, int S, const int* ntok, int ntok_bias, const int* units, int K, int L, const uint32_t* ban_bits,
                             int no_repeat, int repeat_min_id, int64_t* seq, float* row_chosen, int* pos, int* moved, void* stream);

/* Required ALTERNATIVES: bofi_vocab_require_units with GROUPS of units, any one of which satisfies the group -- "dog", "dogs" or "puppy"; "fire hydrant" or "hydrant": a
 * detector tag or an object name is a set of surface forms, and the caption must hold one of them.  Still exact: the masks of the recurrence range over groups, and a
 * state has K * A options "p takes alternative a of group j" instead of K.  A stand-alone launch behind the decode call, as bofi_vocab_require_units: no field of
 * bofi_call_opts_t, no engine state, the ABI version is unchanged.
 * Inputs: bofi_vocab_require_units's (x, ldx, rows, V, S, ntok, ntok_bias, ban_bits, no_repeat, repeat_min_id, seq; n_b = clamp(ntok[b] + ntok_bias, 0, S)), except the table:
 *   alts[b, 0 .. K-1, 0 .. A-1, 0 .. L-1] int32, 1 <= K <= BOFI_REQUIRE_MAX, 1 <= A <= BOFI_REQUIRE_ALT_MAX, 1 <= L <= BOFI_REQUIRE_UNIT_MAX.  Group j is a requirement;
 *   its alternatives are units as bofi_vocab_require_units reads them: the length len_c of a unit is its run of leading ids >= 0; the entries after the first negative
 *   id are not read as ids.  The SLOT of alternative a of group j is c = j * A + a; slot order is table order.
 * Slots of a row, classified per image in slot order: slot c is EMPTY when its first id is < 0.  It is SKIPPED when one of its ids is >= V; one of its ids is banned by
 * ban_bits; it equals an earlier slot of the row (same length, same ids), of any group, kept or not; and, with no_repeat = 1: it holds two equal adjacent ids >=
 * repeat_min_id; its first id (>= repeat_min_id) equals the last id of an earlier KEPT slot of ANOTHER GROUP of the row; or its last id (>= repeat_min_id) equals the first
 * id of such a slot.  Every other slot is kept.  The last two cases exist because two placed units could otherwise meet and form an adjacent repeat (the units' rule, for
 * the units' reason); alternatives of one group are never both placed, so they cannot meet and are not checked against each other for that.  A GROUP is kept when at least
 * one of its slots is.  The host side (require_any_table) refuses a skipped alternative by name.
 * Span "slot c starts at p": it needs p + len_c <= n_b.  Position p + i (i < len_c) contributes 0 where seq[p+i] == u_i on entry; otherwise (double)x[p+i, u_i] -
 * (double)x[p+i, seq[p+i]] when both operands are finite; anything else makes the span INELIGIBLE (NaN, +-inf, a seq[p+i] outside 0..V-1).  With no_repeat = 1 the span
 * is also ineligible when u_0 >= repeat_min_id, seq[p] != u_0 and the live left neighbour holds u_0 on entry (p > 0, seq[p-1] == u_0), or when u_last >= repeat_min_id,
 * seq[p+len_c-1] != u_last and the live right neighbour holds u_last on entry (p + len_c < n_b, seq[p+len_c] == u_last): a placement never creates an adjacent repeat.
 * gain[p][c] is the float64 sum 0.0 + t_0 + t_1 + ... of the span's per-position terms, left to right.
 * Recurrence and tie-break: best[n_b][m] = (0 groups, 0.0) for every mask m of kept GROUPS still to satisfy.  For p = n_b - 1 .. 0 and each m the options are taken in
 * this order: "p takes slot c" for j ascending over the groups of m and, within j, for a ascending over its kept slots c = j * A + a with an eligible span at p, value
 * (1 + cnt, gain[p][c] + tot) of best[p + len_c][m \ j]; then "p keeps its id", value best[p+1][m].  Option values compare first by count, then by total; the FIRST option
 * that attains the maximum is choice[p][m].  The result is the forward walk from (0, all kept groups) along choice, which advances by len_c over a placed span.  For
 * A = 1 this is bofi_vocab_require_units's rule, bit for bit (seq, row_chosen, pos, moved).
 * Outputs: seq -- rewritten on the placed spans, all else untouched; row_chosen (may be NULL) -- x[p+i, u_i] at every span position, all else untouched; pos int32 [B, K]
 * -- the START position of the group's placed alternative, -1 every slot of the group empty, -2 no slot kept and at least one skipped, -3 group kept but not placeable;
 * which int32 [B, K] (may NOT be NULL) -- the index a of the placed alternative, -1 where the group was not placed; moved int32 [B] (may be NULL) -- positions whose id
 * changed.  x is read only.
 * The entry point is total: any table contents, any ntok and ids outside the vocabulary in seq give the rule's result, with no read out of range.
 * One launch, no workspace, deterministic, no atomics; the only float arithmetic is the float64 differences and sums above, in the order above.  rows = 0 is BOFI_OK
 * without a launch.  BOFI_ERR_ARG with a message and no launch: what bofi_vocab_require_units refuses (alts in place of units), a NULL which, A outside 1..4. */
#define BOFI_REQUIRE_ALT_MAX 4
int bofi_vocab_require_any(const float* x, int ldx, int rows, int V, int S, const int* ntok, int ntok_bias, const int* alts, int K, int A, int L, const uint32_t* ban_bits,
                           int no_repeat, int repeat_min_id, int64_t* seq, float* row_chosen, int* pos, int* which, int* moved, void* stream);

/* The N most probable captions of a filling pass, exactly -- the reference's sample_n_method = 'bs' (the N best of a beam) for the non-autoregressive decode, where it is
 * no search: the pass scores every position on its own, a caption's log-probability is a sum of per-position terms, the N best captions use only each row's N best ids,
 * and a width-N merge over the positions finds them.  A stand-alone call behind the decode: no field of bofi_call_opts_t, no engine state, the ABI version is unchanged.
 *   x, ldx, rows, V, S, ntok, ntok_bias, pad_idx, ban_bits: bofi_vocab_constrain's; x is read only.  n_b = clamp(ntok[b] + ntok_bias, 0, S).  1 <= N <= BOFI_NBEST_MAX.
 * Candidates: c[p][0 .. N-1] are the first N unbanned ids of row p in bofi_vocab_constrain's order; a row with fewer unbanned ids has fewer candidates.  Entry r >= 1 is
 * not a candidate when x[p, c[p][r]] is NaN or +-inf; the remaining entries keep their index r.
 * Degenerate image: a live row's x[p, c[p][0]] is not finite (or the row has no unbanned id at all: pad_idx stands for c[p][0]).  It gets count = 1, caption 0 is c[p][0]
 * at every live p, total[b, 0] = NaN.
 * Recurrence: L_0 = [(0.0, empty)]; L_{p+1} is built from all pairs (i, r), i an entry of L_p and r a candidate of row p, with total = T_i + (double)x[p, c[p][r]] -- one
 * float64 add per pair, taken left to right over p.  The pairs are ordered by total descending, then i ascending, then r ascending; the first N are kept.
 * Outputs: count int32 [B] = |L_{n_b}|; seq_n int64 [B, N, S]: the ids of entry j for p < n_b, pad_idx for p >= n_b and for j >= count[b]; total float64 [B, N]: T_j, -inf
 * for j >= count[b].  n_b = 0 gives count = 1, an all-pad row, total = 0.0.
 * Properties: entry 0 is every row's first unbanned id, so it equals the decode's own caption on a NaN-free decode.  The totals do not increase with j.  The count rows
 * are pairwise different on the live positions.  The first N' entries of the N-list are the N'-list, bit for bit (float64 addition is monotone, so an entry that is cut
 * at width N' never has a descendant among the first N').  Where no two float64 totals tie, the list is the N best of all V^n_b captions; with ties, the totals are the N
 * best totals and every caption strictly above the N-th total is in the list.
 *   work / work_bytes: a device workspace of at least bofi_vocab_nbest_workspace(rows) bytes, 4-byte aligned.
 * Two launches (bofi_vocab_pick's candidates launch, then one wavefront per image for the merge), deterministic, no atomics; the only float arithmetic is the float64 add
 * above.  The result is the rule's for every input: a row whose candidate order the first launch could not settle is streamed again by the image's wavefront.
 * rows = 0 is BOFI_OK without a launch.  BOFI_ERR_ARG with a message and no launch: what bofi_vocab_constrain refuses (S > 64 among it), N outside 1..8, a NULL seq_n,
 * total or count, rows > 0 with a NULL or too small workspace. */
#define BOFI_NBEST_MAX 8
int64_t bofi_vocab_nbest_workspace(int rows);
int bofi_vocab_nbest(const float* x, int ldx, int rows, int V, int S, const int* ntok, int ntok_bias, int pad_idx, const uint32_t* ban_bits, int N, int64_t* seq_n,
                     double* total, int* count, void* work, int64_t work_bytes, void* stream);

/* The N most probable captions of a filling pass that have NO ADJACENT REPEATED WORD, exactly.  The rule couples neighbours, so the width-N merge above no longer serves:
 * the list comes from a list-Viterbi over (position, candidate) states with K = N + 2 candidates per row.  A stand-alone call behind the decode: no field of
 * bofi_call_opts_t, no engine state, the ABI version is unchanged.
 *   x, ldx, rows, V, S, ntok, ntok_bias, pad_idx, ban_bits, n_b and the order of ids: bofi_vocab_constrain's; x is read only.  repeat_min_id: its too.
 *   1 <= N <= BOFI_NBEST_NR_MAX.
 * Valid caption: w[0 .. n_b-1] with no banned id and no p >= 1 with w[p] == w[p-1] and w[p-1] >= repeat_min_id -- exactly the eligibility test of bofi_vocab_constrain's
 * scan with no_repeat = 1.
 * Candidates: c[p][0 .. K-1], K = N + 2, are the first K unbanned ids of row p in that order; a row with fewer unbanned ids has fewer candidates.  Entry r >= 1 is not a
 * candidate when x[p, c[p][r]] is NaN or +-inf; the remaining entries keep their index r (as bofi_vocab_nbest).  N + 2 suffice: a caption that uses at p an id with r
 * better ids in front of it has at most two of those excluded by its neighbours w[p-1] and w[p+1]; each of the others gives a different valid caption whose left-to-right
 * float64 total is not smaller (float64 addition is monotone), so with r >= N + 2 there are N captions at least as good.  N + 1 are not enough.
 * Degenerate image, as in bofi_vocab_nbest: a live row's x[p, c[p][0]] is not finite (or the row has no unbanned id at all: pad_idx stands for c[p][0]).  It gets
 * count = 1, caption 0 is c[p][0] at every live p, total[b, 0] = NaN.
 * Recurrence: A_p[r] is a list of at most N (total, prefix) entries per candidate r of row p.  A_0[r] = [(0.0 + (double)x[0, c[0][r]])].  For p >= 1, A_p[r] is built from
 * all pairs (r', j), r' a candidate of row p-1 for which NOT (c[p-1][r'] == c[p][r] and c[p-1][r'] >= repeat_min_id), j an entry of A_{p-1}[r'], with
 * total = T_{r',j} + (double)x[p, c[p][r]] -- one float64 add per pair.  The pairs are ordered by total descending, then r' ascending, then j ascending; the first N are
 * kept.  The result list is all (r, j) of A_{n_b-1} in the same order (total, r, j), its first N.
 * Outputs, of bofi_vocab_nbest's shapes: count int32 [B]; seq_n int64 [B, N, S]: pad_idx for p >= n_b and for j >= count[b]; total float64 [B, N]: -inf for
 * j >= count[b].  n_b = 0 gives count = 1, an all-pad row, total = 0.0.  count may be 0 -- two adjacent rows with one candidate each, the same word: then every row is
 * pad_idx and every total -inf.
 * Properties: every listed caption is valid, and the count rows are pairwise different on the live positions.  The totals do not increase with j.  Each total is the
 * left-to-right float64 sum of its own x values.  Where no two float64 totals tie, the list is the N best of all valid captions with a finite total; with ties, the totals
 * are the N best totals and every valid caption strictly above the N-th total is in the list.  Entry 0 need not be the decode's caption, nor the scan's: its total is >=
 * both whenever theirs is valid and finite.
 *   work / work_bytes: a device workspace of at least bofi_vocab_nbest_workspace(rows) bytes, 4-byte aligned.
 * Two launches (bofi_vocab_pick's candidates launch, then one workgroup of eight wavefronts per image, a wavefront per candidate state), deterministic, no atomics; the only
 * float arithmetic is the float64 add above.  The result is the rule's for every input: a row whose candidate order the first launch could not settle is streamed again.
 * rows = 0 is BOFI_OK without a launch.  BOFI_ERR_ARG with a message "vocab_nbest_norepeat: ..." and no launch: what bofi_vocab_nbest refuses (a NULL or too small
 * workspace with rows > 0 among it), N outside 1..6, repeat_min_id < 0. */
#define BOFI_NBEST_NR_MAX 6
int bofi_vocab_nbest_norepeat(const float* x, int ldx, int rows, int V, int S, const int* ntok, int ntok_bias, int pad_idx, const uint32_t* ban_bits, int repeat_min_id,
                              int N, int64_t* seq_n, double* total, int* count, void* work, int64_t work_bytes, void* stream);

/* A Hamming-diverse SET of N captions of a filling pass, exactly -- the reference's sample_n_method = 'dbs' (diverse beam search with one beam per group and Hamming
 * diversity at the same time step: groups decoded one after another, each pushed away from the words the earlier groups put at the same position, add_diversity in
 * CaptionModel.py:51-68, diversity_lambda) for the non-autoregressive decode, where it is no search: the augmented score of a caption is a sum of per-position terms, so
 * each group's caption is the exact maximiser of its objective -- a per-position pick, or, with "no adjacent repeated word", a Viterbi over each row's few best ids.  A
 * stand-alone call behind the decode: no field of bofi_call_opts_t, no engine state, the ABI version is unchanged.
 *   x, ldx, rows, V, S, ntok, ntok_bias, pad_idx, ban_bits, work / work_bytes: bofi_vocab_nbest's, with the same meaning (the workspace is
 *   bofi_vocab_nbest_workspace(rows) bytes: there is no query of its own); x is read only.  n_b = clamp(ntok[b] + ntok_bias, 0, S).
 *   N: the groups, 1 <= N <= BOFI_DIVERSE_MAX, with no_repeat = 1 at most BOFI_DIVERSE_NR_MAX.  lambda: the diversity strength, finite and >= 0.
 *   no_repeat 0 or 1, repeat_min_id >= 0: bofi_vocab_constrain's rule on every caption of the set (an id >= repeat_min_id never follows itself).
 * Candidates: c[p][0 .. K-1] are the first K unbanned ids of row p in bofi_vocab_constrain's order; K = N with no_repeat = 0, K = N + 2 with no_repeat = 1; a row with fewer
 * unbanned ids has fewer candidates.  As in bofi_vocab_nbest, entry r >= 1 is not a candidate when x[p, c[p][r]] is NaN or +-inf; the remaining entries keep their index r.
 * Degenerate image, as in bofi_vocab_nbest: a live row's x[p, c[p][0]] is not finite (or the row has no unbanned id at all: pad_idx stands for c[p][0]).  It gets
 * count = 1, caption 0 is c[p][0] at every live p, total[b, 0] = aug[b, 0] = NaN.
 * Penalty table: pen[k] = lambda * (double)k, k = 0 .. N-1, computed ON THE HOST by this entry point (pen[0] = 0.0); the kernel receives the table and never multiplies,
 * so no fused multiply-add can change a bit.
 * Groups g = 0 .. N-1, in order.  cnt_g[p][i] is the number of earlier groups whose caption has id i at position p.  The value of candidate r at p is
 * a_g[p][r] = (double)x[p, c[p][r]] - pen[cnt_g[p][c[p][r]]]: one float64 subtraction.
 *   no_repeat = 0: position p takes the candidate with the largest a_g[p][r], ties to the lowest r; aug[b, g] = 0.0 + the taken values, a float64 sum left to right over p.
 *   no_repeat = 1, a Viterbi: V_0[r] = 0.0 + a_g[0][r]; V_p[r] = the maximum, over the candidates r' of row p-1 that have a V and for which NOT (c[p-1][r'] == c[p][r] and
 *   c[p-1][r'] >= repeat_min_id), of V_{p-1}[r'] + a_g[p][r] -- one float64 add per pair, ties to the lowest r'; a state without an admissible predecessor has no V.  The
 *   caption ends in the r with the largest V_{n_b-1}[r], ties to the lowest r, and is read back along the predecessors; aug[b, g] is that V.  Whether a valid caption
 *   exists does not depend on g: if there is none, count = 0, every row is pad_idx, every total and aug is -inf (bofi_vocab_nbest_norepeat's count = 0 case).
 * Outputs: count int32 [B] = N, or 1 or 0 in the cases above; seq_n int64 [B, N, S]: pad_idx for p >= n_b and for g >= count[b]; total float64 [B, N]: 0.0 + the caption's
 * own raw x values, a float64 sum left to right -- its log-prob, comparable to bofi_vocab_nbest's total; aug float64 [B, N]; both -inf for g >= count[b].  n_b = 0 gives
 * count = 1, an all-pad row, total = aug = 0.0.
 * Properties: group 0 with no_repeat = 0 is every row's first unbanned id, i.e. the decode's caption, and aug[b, 0] and total[b, 0] have the same bits.  Group 0 with
 * no_repeat = 1 has the total of entry 0 of bofi_vocab_nbest_norepeat, bit for bit (float64 addition is monotone, so the list-Viterbi's best total is the Viterbi's
 * value).  The captions need not be pairwise different: with lambda = 0 all N groups are equal.  With lambda larger than any spread of a row and no_repeat = 0, group g
 * takes candidate r = g wherever the row has that many candidates.  K candidates suffice: group g has at most g penalised ids at a position and at most two ids are
 * excluded by the neighbours, so among a row's first g + 3 ids (g + 1 without the repeat rule) one is neither penalised nor excluded; its value is not smaller, and by
 * monotonicity neither is the total.  g + 2 candidates are not enough under the repeat rule.  Where no group's maximum is attained by two captions, group g is the
 * maximiser over all V^n_b valid captions of the sum over p of (x - pen[cnt_g]); with ties it is a maximiser of the value.  The first N' groups of the set depend on N
 * only through K.
 * Two launches (bofi_vocab_pick's candidates launch, then one wavefront per image), deterministic, no atomics; the only float arithmetic is the float64 subtraction and
 * the float64 adds above.  The result is the rule's for every input: a row whose candidate order the first launch could not settle is streamed again.
 * rows = 0 is BOFI_OK without a launch.  BOFI_ERR_ARG with a message "vocab_diverse: ..." and no launch: what bofi_vocab_nbest refuses (a NULL aug among it), N outside
 * 1..8 -- outside 1..6 with no_repeat = 1 --, a lambda that is negative, NaN or infinite, no_repeat outside {0, 1}, repeat_min_id < 0. */
#define BOFI_DIVERSE_MAX 8
#define BOFI_DIVERSE_NR_MAX 6
int bofi_vocab_diverse(const float* x, int ldx, int rows, int V, int S, const int* ntok, int ntok_bias, int pad_idx, const uint32_t* ban_bits, int N, double lambda,
                       int no_repeat, int repeat_min_id, int64_t* seq_n, double* total, double* aug, int* count, void* work, int64_t work_bytes, void* stream);

/* The bad-ending trim of the reference's decode_sequence (captioning/utils/misc.py:75-82, REMOVE_BAD_ENDINGS) and the flag of its count_bad
 * (captioning/utils/eval_utils.py:32-37), on id rows.  seq int64 [rows, S], 1 <= S <= 64.  The caption of a row is its ids before the first id <= limit
 * (the whole row without one; 'eval' rule: limit = 0), L of them.  trim_bits / count_bits: uint32 [ceil(V / 32)] each, bit (id % 32) of word id / 32 set for
 * the ids of a word set; either may be NULL (the empty set).  An id < 0 or >= V is in neither set and is not looked up.
 *   k = the length of the run of trim_bits members that ends at position L - 1; k = L (every word a member, or L = 0) counts as k = 0: nothing is removed.
 *   out_seq int64 [rows, S]: the L - k kept ids, then `pad` to the end of the row; it may be seq itself.  out_len int32 [rows]: L - k.
 *   out_bad int32 [rows]: 1 when L - k > 0 and the last kept id is a count_bits member, else 0.
 * rows = 0 is BOFI_OK without a launch; rows < 0, S outside 1..64, V < 1, a NULL seq or output: BOFI_ERR_ARG with a message, nothing is launched.
 * One launch, one wavefront per row, comparisons only: deterministic. */
int bofi_caption_trim(const int64_t* seq, int rows, int S, int limit, const uint32_t* trim_bits, const uint32_t* count_bits, int V, int pad,
                      int64_t* out_seq, int* out_len, int* out_bad, void* stream);

/* Generated sentences among the training sentences, and the words they use (novel_sentences / vocab_size of the reference's language_eval,
 * eval_utils.py:61-69), on id rows in the canonical form bofi_caption_trim writes with pad = 0: len[r] kept ids (clamped to 0..S), then zeros.
 *   seq int64 [rows, S], len int32 [rows], 1 <= S <= 64.  train int32 [M, St]: the training sentences in the same form, distinct, sorted lexicographically
 *   by row (signed comparison, column 0 first); M >= 0 (train may be NULL when M = 0), 1 <= St <= 64.
 *   novel int32 [rows]: 0 when the row, zero-extended, equals a training row, zero-extended; else 1.  So a row with a non-zero id at a position >= St is novel, a
 *     strict prefix of a training row is novel, and the empty row is a sentence like any other.
 *   seen int32 [V], zeroed by the caller: seen[id] = 1 for every kept id in [0, V) of every row (plain stores of the same value); other ids are skipped.
 * rows = 0 is BOFI_OK without a launch; bad sizes or a NULL among seq / len / novel / seen: BOFI_ERR_ARG with a message, nothing is launched.
 * One launch, one wavefront per row: a binary search of at most ceil(log2(M + 1)) probes, each one row of train.  Deterministic. */
int bofi_sentence_lookup(const int64_t* seq, const int* len, int rows, int S, const int* train, int M, int St, int V, int* novel, int* seen,
                         void* stream);

/* Last HIP error string seen by this library on the calling thread (for exceptions in the host). */
const char* bofi_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* BOFICAP_HIP_H */
