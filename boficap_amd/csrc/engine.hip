// Host-side engine: owns one model replica's packed weights and workspace in HBM and enqueues the
// whole NAIC bound+fill decode (reference AttModel._sample AttModel.py:307-338,419-429 ->
// TransformerModel._prepare_feature :1674-1690 -> core_NAIC :1823-1876 -> logit/log_softmax ->
// greedy pick) as one stream of HIP kernels, optionally replayed from a captured hipGraph.
// No host<->device synchronisation happens inside a decode call: the slot state of the bounding
// loop lives on the device and finished batches make the remaining bound kernels return at once.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/boficap_hip.h"
#include "bofi_common.h"
#include "bofi_kernels.h"
#include "bofi_naic.h"


namespace {

thread_local std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }

#define ENG_HIP(call)                                                                          \
    do {                                                                                       \
        hipError_t e__ = (call);                                                               \
        if (e__ != hipSuccess) return fail(BOFI_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e__)); \
    } while (0)
#define ENG_OK(call)                                                                           \
    do {                                                                                       \
        int r__ = (call);                                                                      \
        if (r__ != BOFI_OK) { if (g_err.empty() || r__ != BOFI_ERR_HIP) g_err = std::string(#call) + " failed"; return r__; } \
    } while (0)

struct Lin { void* w = nullptr; float* b = nullptr; float* cs = nullptr; int N = 0, K = 0; int Npad = 0; void* wp = nullptr; void* wp16 = nullptr; };   // cs: column sums when a LayerNorm is folded in; Npad > N: rows N .. Npad of w / b / cs exist and are zero; wp: fragment-major copy of w for the row-block kernels (rowblock.hip), bf16 engine only; wp16: fragment-major FP16 copy made from the float32 parameters (bound_loop.hip), the bounding layer's Linears of a bf16 engine only
struct Norm { float* g = nullptr; float* b = nullptr; };
struct EncLayer { Lin qkv, o, w1, w2; Norm n0, n1; };
struct DecLayer { Lin qkv, o, q_src, o_src, w1, w2; Norm n0, n1, n2; };

// how a packed weight is made from the named parameters: declared by bofi_engine_finalize, carried out on the device by bofi_engine::repack
struct LinRecipe { Lin* out; std::vector<std::string> prefixes; int n_each, K; std::string fold; };

struct NormRecipe { Norm* out; std::string prefix; int d; };
// name -> (float32 parameter in device memory, element count): what bofi_engine::repack reads
using DevParams = std::map<std::string, std::pair<const float*, int64_t>>;

// A residual stream: the float32 rows, their copy in the compute dtype and the rows' partial sums [rows][groups][2] from which the consuming GEMM
// applies the pre-norm LayerNorm in its epilogue.  The float32 engine reads the stream itself and keeps no copy.
struct Stream {
    float* x = nullptr; void* xb = nullptr; float* st = nullptr;
    bool f32 = false;
    int groups = 0;                                                   // partial-sum pairs per row of st (0: d_model / 32)
    const void* in() const { return f32 ? (const void*)x : xb; }      // what a GEMM of the compute dtype reads
    void* copy() const { return f32 ? nullptr : xb; }                 // where a producer leaves the copy (none: float32 engine)
};
// Which rows of a launch run: all of them, unless an early-out word says the work is over (*skip >= thr: the launch returns at once) or a row list on
// the device names them (idx[0 .. *m_dev), the SAIC iterations).  Launches that carry either never take the row-block kernels.
struct Rows {
    const int* skip = nullptr; int thr = 0;
    const int* idx = nullptr; const int* m_dev = nullptr;
};

struct GraphEntry {
    std::vector<uintptr_t> key;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
};

}  // namespace

int bofi::fail(int code, const std::string& msg) { g_err = msg; return code; }      // the other translation units' way to bofi_last_error()

struct bofi_engine {
    bofi_config_t cfg{};
    std::map<std::string, std::vector<float>> host;
    std::vector<void*> allocs;
    bool finalized = false;
    int L = 0;                       // seq_length + 2
    size_t tsz = 4;                  // bytes per compute-dtype element

    // weights
    Lin att_embed;
    std::vector<EncLayer> enc; Norm enc_norm;
    std::vector<DecLayer> dec; Norm dec_norm;
    std::vector<DecLayer> blay;      // the bounding network's layers as full layers (dense form: N_len >= 2, or forced for a self-check)
    int n_len = 1;
    bool bound_dense = false;
    Lin kv_all;                      // stacked cross-attention K|V: bound layer, then decoder layers
    Lin gen;
    float *lut_syn = nullptr, *lut_tok = nullptr, *pe = nullptr;
    // bound layer
    Lin b_o_self, b_q_src, b_o_src, b_w1, b_w2;
    Norm b_n0, b_n1, b_n2;
    bofi::BoundHeadWeights heads{};
    void *b_q0 = nullptr, *b_kvtab = nullptr;     // compute dtype: [d], [L*10, 2d]
    float* b_x0 = nullptr;                        // [d] residual input of row 0
    void *b_votab = nullptr, *b_w1p = nullptr;    // compute dtype: Wo_self . V per (row, head) [L*10, H, d]; packed head hidden weights
    float* b_x0b = nullptr;                       // [d] x0 + bo_self
    // the persistent bounding-loop kernel (bound_loop.hip; bf16 engine at the reference's width): float32 tables of the row-0 self-attention
    Lin b_heads;                                  // hidden layers of both heads stacked, length_predictor.norm folded in (its wp16 and folded bias are what the loop kernel reads)
    float *b_q0_32 = nullptr, *b_sctab = nullptr, *b_vtab = nullptr;      // [d], [L*10][H], [L*10][d]
    // filling pass, round 0: every word is BOS (decode_NA TransformerModel.py:570-577), so the first decoder layer's input row -- and with it its q|k|v row -- depends on
    // (label, position) only: f_qkv0[(label*S + t)][3d] in the compute dtype, made by the SAME row-block projection kernel a decode would run on those rows (a row's
    // result does not depend on the launch), gathered by embed_fill instead of a 10-GFLOP projection per 320 images.  Rebuilt by every repack.
    void* f_qkv0 = nullptr; float* f_x0 = nullptr; int* f_syn = nullptr; bool fill_tab_ready = false;
    // the options of the entry-point call that is running (bofi_call_opts_t states each field): every entry point overwrites them -- with the caller's record, or
    // with the defaults -- before it enqueues anything, so nothing of one call reaches the next; key_call() puts them into the graph key
    bofi_call_opts_t opt{};
    bool attn_out_set() const { return opt.attn_mean || opt.attn_heads || opt.attn_top_idx; }
    bool pick_set(int flags) const { return opt.pick_ban || opt.pick_no_repeat || (flags & BOFI_FLAG_PICK_TRIGRAMS); }      // the constrained pick (bofi_call_opts_t.pick_*, BOFI_FLAG_PICK_TRIGRAMS) is on
    bool loop_ready = false;
    float* dbg_part = nullptr;

    // workspace
    Stream x_enc, x_fill;                // residual streams of the encoder [Bm*Rm, d] and of the filling pass / decoder rows [Bm*Sq, d]
    float* logits = nullptr;
    float* logits_pad = nullptr;         // bf16 engine: the generator's output with a pitch of gen.Npad (whole 128-column tiles: the persistent GEMM), read by vocab_finalize
    void *qkv = nullptr, *ctx = nullptr, *hdn = nullptr, *mem = nullptr, *kv = nullptr, *qs = nullptr, *xn = nullptr;
    bool no_logits = false;              // a fork made with BOFI_FORK_IDS_ONLY: neither of the two buffers above
    float* vb_part = nullptr; unsigned* vb_ctr = nullptr;             // the fused generator's per-row records and row-block counters (launch_rb_vocab; bf16 engine)
    void* feats_t = nullptr;                                          // bf16 copy of float32 input features
    float* st_fill16 = nullptr;                                       // row partial sums of the decoder rows per 16 columns [Bm*Sq][d/16][2] (row-list iterations of the SAIC decode)
    float* st_b16 = nullptr;                                          // row partial sums per 16 columns [Bm][d/16][2] (bound_ops.hip)
    Stream y1, y2;                       // row 0 of a bounding iteration [Bm, d] behind its self-attention / cross-attention sublayer (one copy and one set of statistics serve both)
    float* by3 = nullptr;                // the feed-forward sublayer's output as up to 4 partial slabs [4][Bm, d]
    void *bctx = nullptr, *bq2 = nullptr, *bctx2 = nullptr, *bh = nullptr;
    bofi::BoundState st{};
    bofi::SaicState sa{};
    Stream xw;                                                          // all L rows of the bound sequence [B*L, d]: SAIC bound input, dense bounding pass
    void* kvs = nullptr;                                                // their K|V [B*L, 2d]
    int64_t* tok64 = nullptr;                                           // greedy ids of one decoder pass [B*S]
    // mask-predict refinement (refine.hip), [Bm*Sq] each: the state (id, its log-prob, sum_v p log p, emitting pass), what a pass's epilogue left, the next pass's mask and input ids
    int64_t *mp_ids = nullptr, *mp_fresh_ids = nullptr, *mp_next_ids = nullptr;
    float *mp_chosen = nullptr, *mp_plogp = nullptr, *mp_fresh_chosen = nullptr, *mp_fresh_plogp = nullptr;
    int *mp_round = nullptr, *mp_mask = nullptr;
    int* pick_changed = nullptr;                                        // [Bm] positions the constrained pick of the last filling pass changed (bofi_engine_pick_changed)
    int* pick_work = nullptr; size_t pick_work_bytes = 0;               // bofi_vocab_pick's candidates [Bm*Sq][K] (BOFI_FLAG_PICK_TRIGRAMS; not on a fork without vocabulary buffers)
    std::vector<void*> qkv_dec;                                         // SAIC: q|k|v of every decoder layer [B*S, 3d] (the K / V cache)
    int *sa_rows = nullptr, *sa_nrows = nullptr;                        // decoder rows of the iteration's new phrases, their count
    uint64_t* d_seed = nullptr;                                         // per-call sampling seed (read by the captured sampling kernels)
    bool saic_cache = true, saic_lean = true;
    Lin b_kv_self;                                                      // bound self-attention K|V with sublayer.0.norm folded in
    Lin t_kvself, t_qself; float* d_xt = nullptr; Norm head_norm;       // setup-time operands of the bound tables, kept for refreshes
    std::vector<LinRecipe> lin_recipes; std::vector<NormRecipe> norm_recipes;
    void* b_q0_sa = nullptr; float* b_x0_sa = nullptr;                  // row-0 constants when position 0 holds tgt_embed([LEN])

    hipStream_t cap_stream = nullptr;
    int saic_B = 0;                       // images of the last semi-autoregressive decode (what bofi_engine_saic_put_words may continue)
    // what describes the engine, not one call (their setters; part of the graph key).  A fork inherits kv_beside -- a form switch for A/B runs -- and starts from the defaults otherwise
    struct Settings {
        int in_flight = 0;                // decodes the caller keeps in flight (bofi_engine_set_decodes_in_flight; 0 = unknown: throughput forms)
        int loop_mode = -1;               // bofi_engine_set_bound_loop: -1 = BOFI_BOUND_LOOP / hint decide, 0 = five-launch iterations, 2 = the persistent loop kernel
        int kv_beside = 1;                // bofi_engine_set_bound_kv_beside: 0 = never, 1 = the decoder layers' cross K|V are projected beside the bounding loop where bound_kv_beside_ok says so
        Settings forked() const { Settings s; s.kv_beside = kv_beside; return s; }
    } settings;
    float* bl_xbuf = nullptr; unsigned* bl_xctl = nullptr;      // the loop kernel's pair exchange: partial sums and control words (workspace: one set per engine / fork)
    int* b_wsat = nullptr;                // [1] set by pack_frag16 when an fp16 weight copy was clamped (shared with forks, like the weights)
    hipStream_t run_stream = nullptr;     // a stream of the engine's own, offered to callers that keep several decodes in flight
    std::vector<GraphEntry> graphs;

    template <typename U> int dalloc(U** p, size_t n_elems, size_t elem = sizeof(U)) {
        void* q = nullptr;
        const size_t bytes = (n_elems * elem + 255) & ~(size_t)255;
        ENG_HIP(hipMalloc(&q, bytes ? bytes : 256));
        ENG_HIP(hipMemset(q, 0, bytes ? bytes : 256));
        allocs.push_back(q);
        *p = (U*)q;
        return BOFI_OK;
    }
    int upload_f32(float** p, const std::vector<float>& v) {
        ENG_OK(dalloc(p, v.size()));
        ENG_HIP(hipMemcpy(*p, v.data(), v.size() * 4, hipMemcpyHostToDevice));
        return BOFI_OK;
    }
    const std::vector<float>* get(const std::string& name, size_t numel) {
        auto it = host.find(name);
        if (it == host.end()) { g_err = "missing weight " + name; return nullptr; }
        if (it->second.size() != numel) {
            g_err = "weight " + name + " has " + std::to_string(it->second.size()) + " elements, expected " + std::to_string(numel);
            return nullptr;
        }
        return &it->second;
    }
    // Declare one Lin: several [n_each, K] matrices (and their biases) stacked, with fold_norm the pre-norm LayerNorm that feeds the layer folded
    // in (gemm_glds.hip).  Shapes and buffers only: the parameters are checked to exist, the outputs are allocated -- zero-filled, which is what rows
    // N .. Npad stay -- and the recipe is recorded; repack() fills the first N rows (pack_lin_multi_kernel states the arithmetic).
    int make_lin(Lin* out, const std::vector<std::string>& prefixes, int n_each, int K, const std::string& fold_norm = "", int pad_to = 0, bool frag = false) {
        for (const auto& p : prefixes)
            if (!get(p + ".weight", (size_t)n_each * K) || !get(p + ".bias", (size_t)n_each)) return BOFI_ERR_STATE;
        if (!fold_norm.empty() && (!get(fold_norm + ".a_2", K) || !get(fold_norm + ".b_2", K))) return BOFI_ERR_STATE;
        out->N = n_each * (int)prefixes.size();
        out->K = K;
        out->Npad = pad_to > 0 ? ((out->N + pad_to - 1) / pad_to) * pad_to : out->N;
        out->cs = nullptr;
        if (!fold_norm.empty()) ENG_OK(dalloc(&out->cs, (size_t)out->Npad));
        ENG_OK(dalloc((char**)&out->w, (size_t)out->Npad * K, tsz));
        ENG_OK(dalloc(&out->b, (size_t)out->Npad));
        out->wp = nullptr;
        out->wp16 = nullptr;
        if (frag && cfg.dtype == BOFI_DT_BF16 && out->Npad % 64 == 0 && K % 32 == 0)      // the layout the row-block kernels stream (zero rows included)
            ENG_OK(dalloc((char**)&out->wp, (size_t)out->Npad * K, 2));
        lin_recipes.push_back(LinRecipe{out, prefixes, n_each, K, fold_norm});
        return BOFI_OK;
    }
    int make_norm(Norm* out, const std::string& prefix, int d) {
        if (!get(prefix + ".a_2", d) || !get(prefix + ".b_2", d)) return BOFI_ERR_STATE;
        ENG_OK(dalloc(&out->g, (size_t)d));
        ENG_OK(dalloc(&out->b, (size_t)d));
        norm_recipes.push_back(NormRecipe{out, prefix, d});
        return BOFI_OK;
    }

    // ---- kernels -------------------------------------------------------------------------------
    struct LinOpt {
        const float* residual = nullptr; int ldr = 0;
        int relu = 0;
        const int* row_len = nullptr; int rpg = 0;
        Rows rows;                           // early-out word and / or row list
        int splitk = 1;                      // K split over workgroups, float32 partial slabs out
        const Norm* ln = nullptr;            // explicit LayerNorm kernel on x first (setup-time use only)
        const float* ln_stats = nullptr;     // LayerNorm folded into the GEMM (Lin built with fold_norm)
        float* stats_out = nullptr;          // emit row partial sums of the output
        void* y2 = nullptr;                  // compute-dtype copy of the output
        int ln_groups = 0;                   // partial-sum pairs per row of ln_stats (0: K / 32)
    };
    int linear(const void* x, int x_dtype, int ldx, const Lin& l, void* y, int y_dtype, int ldy, int M, const LinOpt& o, hipStream_t s) {
        if (o.ln) {
            if (x_dtype != BOFI_DT_F32 || ldx != l.K) return BOFI_ERR_ARG;
            int rc = bofi::launch_layernorm((const float*)x, o.ln->g, o.ln->b, xn, cfg.dtype, M, l.K, s, nullptr, 0);
            if (rc != BOFI_OK) return rc;
            x = xn; x_dtype = cfg.dtype;
        }
        if (o.ln_stats && !l.cs) return BOFI_ERR_STATE;
        bofi::LinearArgs a{};
        a.x = x; a.x_dtype = x_dtype; a.ldx = ldx; a.w = l.w; a.w_dtype = cfg.dtype; a.bias = l.b;
        a.residual = o.residual; a.ldr = o.ldr; a.y = y; a.y_dtype = y_dtype; a.ldy = ldy;
        a.M = M; a.N = l.N; a.K = l.K; a.relu = o.relu; a.row_len = o.row_len; a.rows_per_group = o.rpg;
        a.ln_stats = o.ln_stats; a.ln_colsum = o.ln_stats ? l.cs : nullptr; a.ln_groups = o.ln_groups;
        a.stats_out = o.stats_out; a.y2 = o.y2; a.ldy2 = l.N; a.splitk = o.splitk;
        a.skip_if_ge = o.rows.skip; a.skip_threshold = o.rows.thr; a.row_idx = o.rows.idx; a.m_dev = o.rows.m_dev;
        return bofi::launch_linear(a, s);
    }
    // The two GEMMs a pre-norm sublayer is made of, as tiled launches on the rows r.  folded: y = l(LayerNorm(t)), the LayerNorm applied from the
    // stream's copy and statistics (Lin built with fold_norm).  close_sublayer: t = residual + l(x) -- the stream's float32 rows, its copy and its
    // statistics are all written here (residual: the stream itself unless the sublayer's input rows live elsewhere, pitch ldr).
    int folded(const Stream& t, const Lin& l, void* y, int y_dtype, int ldy, int M, const Rows& r, hipStream_t s, int relu = 0) {
        LinOpt o; o.relu = relu; o.ln_stats = t.st; o.ln_groups = t.groups; o.rows = r;
        return linear(t.in(), cfg.dtype, cfg.d_model, l, y, y_dtype, ldy, M, o, s);
    }
    int close_sublayer(const void* x, const Lin& l, const Stream& t, int M, const Rows& r, hipStream_t s, const float* residual = nullptr, int ldr = 0) {
        LinOpt o; o.residual = residual ? residual : t.x; o.ldr = residual ? ldr : cfg.d_model; o.stats_out = t.st; o.y2 = t.copy(); o.rows = r;
        return linear(x, cfg.dtype, l.K, l, t.x, BOFI_DT_F32, cfg.d_model, M, o, s);
    }
    // self-attention over a packed q|k|v buffer [B*Lq, 3d] and cross-attention over slot i of the stacked cross K|V `kv` (bound layers, then decoder
    // layers), context rows into `out`.  Callers add what differs: the key lengths (and quirk Q1's klen_shared_last), the early-out word.
    const void* kv_slot(int i) const { return (const char*)kv + (size_t)i * 2 * cfg.d_model * tsz; }
    bofi::AttnArgs attn_args(const void* q, int ldq, const void* k, int ldkv, void* out, int B, int Lq, int Lk, const Rows& r) const {
        bofi::AttnArgs a{};
        a.q = q; a.ldq = ldq; a.k = k; a.v = (const char*)k + (size_t)cfg.d_model * tsz; a.ldk = a.ldv = ldkv;
        a.out = out; a.ldo = cfg.d_model; a.dtype = cfg.dtype; a.B = B; a.H = cfg.heads; a.Lq = Lq; a.Lk = Lk;
        a.skip_if_ge = r.skip; a.skip_threshold = r.thr;
        return a;
    }
    bofi::AttnArgs self_attn_args(const void* qkv, int B, int Lq, const Rows& r = Rows{}) const {
        return attn_args(qkv, 3 * cfg.d_model, (const char*)qkv + (size_t)cfg.d_model * tsz, 3 * cfg.d_model, ctx, B, Lq, Lq, r);
    }
    bofi::AttnArgs cross_attn_args(const void* q, int i, void* out, int B, int Lq, int R, const int* att_len, const Rows& r = Rows{}) const {
        bofi::AttnArgs a = attn_args(q, cfg.d_model, kv_slot(i), kv_all.N, out, B, Lq, R, r);
        a.klen = att_len; a.klen_sb = 1;
        return a;
    }
    bool is_fork = false;
    size_t n_weight_allocs = 0;          // allocs[0 .. n) are weights (owned by the parent), the rest workspace
    // repack: descriptor tables of its batched launches (device copy, pinned staging, what was uploaded last)
    void* rt_dev = nullptr; void* rt_pin = nullptr; size_t rt_bytes = 0; std::vector<char> rt_cache;

    // the generator runs over zero-padded weight rows into a buffer of its own pitch (logits_pad; enqueue_fill)
    bool gen_padded() const { return cfg.dtype == BOFI_DT_BF16 && gen.Npad > gen.N; }
    // workspace of one in-flight decode (a forked engine has its own, and shares the weights)
    int alloc_workspace() {
    const bofi_config_t& c = cfg;
    const size_t Bm = c.max_batch, Rm = c.max_regions, Sq = c.seq_length;
    const int d = c.d_model, dff = c.d_ff;
    const size_t Lm = Sq + 2;
    const size_t rows = Bm * (Rm > Lm ? Rm : Lm);
    auto stream = [&](Stream* t, size_t n) -> int {       // a residual stream of n rows
        t->f32 = c.dtype == BOFI_DT_F32;
        ENG_OK(dalloc(&t->x, n * d)); ENG_OK(dalloc((char**)&t->xb, n * d, tsz)); ENG_OK(dalloc(&t->st, n * (d / 32) * 2));
        return BOFI_OK;
    };
    ENG_OK(stream(&x_enc, Bm * Rm)); ENG_OK(stream(&x_fill, Bm * Sq)); ENG_OK(stream(&xw, Bm * L));
    ENG_OK(stream(&y1, Bm));
    y2 = y1; ENG_OK(dalloc(&y2.x, Bm * d));
    logits = logits_pad = nullptr;
    if (!no_logits) {
        ENG_OK(dalloc(&logits, Bm * Sq * c.vocab));
        if (gen_padded()) ENG_OK(dalloc(&logits_pad, Bm * Sq * (size_t)gen.Npad));
    }
    if (c.dtype == BOFI_DT_BF16) { ENG_OK(dalloc(&vb_part, bofi::rb_vocab_part_floats(Bm * Sq))); ENG_OK(dalloc(&vb_ctr, bofi::rb_vocab_ctr_words(Bm * Sq))); }
    ENG_OK(dalloc((char**)&qkv, rows * 3 * d, tsz));
    ENG_OK(dalloc((char**)&ctx, rows * d, tsz));
    ENG_OK(dalloc((char**)&hdn, rows * dff, tsz));
    ENG_OK(dalloc((char**)&mem, Bm * Rm * d, tsz));
    ENG_OK(dalloc((char**)&kv, Bm * Rm * (size_t)kv_all.N, tsz));
    ENG_OK(dalloc((char**)&qs, Bm * Lm * d, tsz));                    // (the dense bounding pass projects queries for all L rows of an image)
    ENG_OK(dalloc((char**)&xn, (rows > (size_t)L * 10 ? rows : (size_t)L * 10) * d, tsz));
    if (c.dtype == BOFI_DT_BF16) ENG_OK(dalloc((char**)&feats_t, Bm * Rm * (size_t)c.feat, 2));
    ENG_OK(dalloc(&st_b16, Bm * (d / 16) * 2));
    ENG_OK(dalloc(&by3, 4 * Bm * d));
    ENG_OK(dalloc((char**)&bctx, Bm * d, tsz)); ENG_OK(dalloc((char**)&bq2, Bm * d, tsz));
    ENG_OK(dalloc((char**)&bctx2, Bm * d, tsz)); ENG_OK(dalloc((char**)&bh, Bm * dff, tsz));
    ENG_OK(dalloc(&st.last, Bm)); ENG_OK(dalloc(&st.finished, Bm)); ENG_OK(dalloc(&st.phrase_num, Bm));
    ENG_OK(dalloc(&st.phrase_length, Bm * L)); ENG_OK(dalloc(&st.phrase_syn, Bm * L));
    ENG_OK(dalloc(&st.ext_syn, Bm * L)); ENG_OK(dalloc(&st.counters, 8)); ENG_OK(dalloc(&st.klen, Bm * L));
    if (c.dtype == BOFI_DT_BF16) {                                  // the loop kernel's pair exchange (bound_loop.hip): per group of 16 images 2 x 2 partial tiles + 4 control words
        const size_t groups = (Bm + 15) / 16;
        ENG_OK(dalloc(&bl_xbuf, groups * 4 * 16 * 512)); ENG_OK(dalloc(&bl_xctl, groups * 4));
        st.pair_ctl = bl_xctl;
    }
    ENG_OK(dalloc(&sa.seq_last, Bm)); ENG_OK(dalloc(&sa.seq, Bm * L)); ENG_OK(dalloc(&sa.ext_len, Bm * L));
    ENG_OK(dalloc(&sa.ext_phrase, Bm * L)); ENG_OK(dalloc(&sa.klen_dec, Bm * L));
    ENG_OK(dalloc((char**)&kvs, Bm * L * 2 * (size_t)d, tsz)); ENG_OK(dalloc(&tok64, Bm * Sq));
    ENG_OK(dalloc(&sa_rows, Bm * Sq)); ENG_OK(dalloc(&sa_nrows, 4)); ENG_OK(dalloc(&d_seed, 2));
    ENG_OK(dalloc(&st_fill16, Bm * Sq * (d / 16) * 2));
    ENG_OK(dalloc(&mp_ids, Bm * Sq)); ENG_OK(dalloc(&mp_fresh_ids, Bm * Sq)); ENG_OK(dalloc(&mp_next_ids, Bm * Sq));
    ENG_OK(dalloc(&mp_chosen, Bm * Sq)); ENG_OK(dalloc(&mp_plogp, Bm * Sq)); ENG_OK(dalloc(&mp_fresh_chosen, Bm * Sq)); ENG_OK(dalloc(&mp_fresh_plogp, Bm * Sq));
    ENG_OK(dalloc(&mp_round, Bm * Sq)); ENG_OK(dalloc(&mp_mask, Bm * Sq));
    ENG_OK(dalloc(&pick_changed, Bm));
    if (!no_logits) { pick_work_bytes = bofi::vocab_pick_work_bytes((int)(Bm * Sq)); ENG_OK(dalloc(&pick_work, pick_work_bytes / sizeof(int))); }
    qkv_dec.assign(c.n_dec, nullptr);                  // allocated by the first semi-autoregressive decode

        return BOFI_OK;
    }

    // the per-image tail of a bounding iteration (naic.hip): heads on the FFN output `y`, bookkeeping, next self-attention sublayer
    int bound_tail(const float* y, int yparts, const int* ext_syn_in, const int* last_in, int B, int flags, float* len_logp, float* syn_logp,
                   hipStream_t s, bool saic = false, int iter = 0, int y_stride = 0) {
        bofi::BoundTailArgs a{};
        a.y = y; a.yparts = yparts; a.y_stride = y_stride; a.w = heads; a.st = st; a.sa = saic ? sa : bofi::SaicState{};
        a.ext_syn_in = ext_syn_in; a.last_in = last_in; a.q0 = b_q0; a.kvtab = b_kvtab; a.votab = b_votab; a.x0b = b_x0b;
        a.y1 = y1.x; a.y1t = y1.copy(); a.stats = y1.st;
        const int tail_dbg = bofi::knob(BOFI_TAIL_DBG);     // developer ablations
        a.B = B; a.L = L; a.S = cfg.seq_length; a.d = cfg.d_model; a.hh = cfg.head_hidden; a.H = cfg.heads; a.flags = flags | (tail_dbg << 8); a.iter = iter;
        a.len_logp = len_logp; a.syn_logp = syn_logp;
        const bool want_dbg = bofi::knob(BOFI_DBG_PART) != 0;
        if (want_dbg && !dbg_part) ENG_OK(dalloc(&dbg_part, (size_t)cfg.max_batch * (16 * cfg.head_hidden + cfg.d_model)));
        a.dbg_part = dbg_part;
        return bofi::launch_bound_tail(a, cfg.dtype, s);
    }
    // tables derived from the bound layer's weights once kvtab exists (repack)
    int derive_bound_tables(hipStream_t s) {
        ENG_OK(bofi::launch_pack_w1p(heads.w1t, b_w1p, cfg.dtype, cfg.d_model, 2 * cfg.head_hidden, s));
        ENG_OK(bofi::launch_votab(b_kvtab, b_o_self.w, b_x0, b_o_self.b, b_votab, b_x0b, cfg.dtype, L * 10, cfg.d_model, cfg.heads, s));
        return derive_fill_table(s);
    }
    int derive_fill_table(hipStream_t s) {
        fill_tab_ready = false;
        if (!f_qkv0 || !rb_ok() || dec.empty() || !dec[0].qkv.wp || !dec[0].qkv.cs || dec[0].qkv.Npad != 3 * cfg.d_model) return BOFI_OK;
        const int d = cfg.d_model, S = cfg.seq_length;
        // the input rows of 10 pseudo-images whose slots all carry one label, then their q|k|v by the row-block projection kernel
        ENG_OK(bofi::launch_embed_fill(lut_tok, lut_syn, pe, f_syn, nullptr, 10, S, L, d, cfg.bos_idx, f_x0, nullptr, cfg.dtype, nullptr, s));
        bofi::RbGemmArgs a{};
        a.x = f_x0; a.ldx = d; a.wp = (const bofi::u32x4*)dec[0].qkv.wp; a.c = dec[0].qkv.b; a.cs = dec[0].qkv.cs; a.y = f_qkv0; a.ldy = 3 * d; a.y_f32 = 0; a.M = 10 * S; a.N = 3 * d;
        ENG_OK(bofi::launch_rb_gemm(a, s));
        fill_tab_ready = true;
        return BOFI_OK;
    }
    // ---- the persistent bounding-loop kernel's operands: fp16 fragment-major copies of the bounding layer's Linears and the float32 self-attention
    // tables, all derived on the device from the float32 parameters (repack)
    struct BoundSrc {
        const float *wq_self, *bq_self, *wk_self, *bk_self, *wv_self, *bv_self, *n0g, *n0b;
        const float *wo_self, *wq_src, *n1g, *wo_src, *w1, *n2g, *w2, *lw1, *sw1, *hng;
    };
    bool loop_config_ok() const {
        return cfg.dtype == BOFI_DT_BF16 && cfg.d_model == 512 && cfg.heads == 8 && cfg.d_ff % 512 == 0 && cfg.d_ff <= 2048 && L <= 24 && cfg.head_hidden <= 128 &&
               n_len == 1 && !bound_dense;
    }
    int derive_bound_f16(const BoundSrc& b, hipStream_t s) {
        if (!loop_config_ok()) return BOFI_OK;
        const int d = cfg.d_model, dff = cfg.d_ff, hh = cfg.head_hidden;
        bofi::Pack16Table t{};
        auto ent = [&](const float* w0, const float* w1_, int n_each, int nsrc, int K, int Npad, const float* gain, void* out) {
            bofi::Pack16Entry& q = t.e[t.n++];
            q.w[0] = w0; q.w[1] = w1_; q.gain = gain; q.out = out; q.n_each = n_each; q.nsrc = nsrc; q.K = K; q.Npad = Npad; q.blk0 = 0;
        };
        ent(b.wo_self, nullptr, d, 1, d, d, nullptr, b_o_self.wp16);
        ent(b.wq_src, nullptr, d, 1, d, d, b.n1g, b_q_src.wp16);
        ent(b.wo_src, nullptr, d, 1, d, d, nullptr, b_o_src.wp16);
        ent(b.w1, nullptr, dff, 1, d, dff, b.n2g, b_w1.wp16);
        ent(b.w2, nullptr, d, 1, dff, d, nullptr, b_w2.wp16);
        ent(b.lw1, b.sw1, hh, 2, d, 256, b.hng, b_heads.wp16);
        t.sat = b_wsat;
        ENG_OK(bofi::launch_pack_frag16(t, s));
        bofi::BoundTablesArgs a{};
        a.xt = d_xt; a.x0 = b_x0; a.rows = L * 10; a.n0g = b.n0g; a.n0b = b.n0b;
        a.wq = b.wq_self; a.bq = b.bq_self; a.wk = b.wk_self; a.bk = b.bk_self; a.wv = b.wv_self; a.bv = b.bv_self;
        a.q0 = b_q0_32; a.sctab = b_sctab; a.vtab = b_vtab;
        ENG_OK(bofi::launch_bound_tables(a, s));
        loop_ready = true;
        return BOFI_OK;
    }
    // ---- The one implementation of weight packing: every declared Linear and Norm, the embedding tables, the bound heads and the bounding layer's
    // tables, from float32 parameters in device memory (finalize: a staged copy of the host map, null stream; refresh_device: the caller's tensors
    // and stream).  Every Linear's repack (stack, fold the pre-norm, cast, column sums), the fragment-major copies and the small float32 vectors are
    // THREE launches over descriptor tables in device memory (they were ~230 launches and copies: 1.5 ms of a training step that decodes with its
    // current weights).  The tables hold the source pointers: uploaded again only when one of them changed.
    int repack(const DevParams& src, hipStream_t s) {
        const bofi_config_t& c = cfg;
        const int d = c.d_model, dff = c.d_ff, hh = c.head_hidden;
        auto param = [&](const std::string& name, int64_t numel) -> const float* {
            auto it = src.find(name);
            if (it == src.end() || !it->second.first) { g_err = "missing weight " + name; return nullptr; }
            if (it->second.second != numel) { g_err = "weight " + name + " has " + std::to_string(it->second.second) + " elements, expected " + std::to_string(numel); return nullptr; }
            return it->second.first;
        };
        std::vector<bofi::PackLinDesc> lin_tab;
        std::vector<bofi::CopyDesc> copy_tab;
        int rows = 0, fblocks = 0, cblocks = 0;
        auto add_copy = [&](const float* src, float* dst, int n) { copy_tab.push_back(bofi::CopyDesc{src, dst, n, cblocks}); cblocks += (n + 255) / 256; };
        for (const auto& r : lin_recipes) {
            if (!r.out->w || !r.out->b || (!r.fold.empty() && !r.out->cs)) return fail(BOFI_ERR_STATE, "repack: a packed weight is missing");
            const int nsrc = (int)r.prefixes.size();
            for (int i0 = 0; i0 < nsrc; i0 += 16) {       // a table entry stacks up to 16 matrices: a longer stack is several entries, one behind the other
                bofi::PackLinDesc dsc{};
                bofi::PackLinArgs& a = dsc.a;
                a.nsrc = nsrc - i0 < 16 ? nsrc - i0 : 16; a.n_each = r.n_each; a.K = r.K;
                for (int i = 0; i < a.nsrc; ++i) {
                    a.w[i] = param(r.prefixes[i0 + i] + ".weight", (int64_t)r.n_each * r.K);
                    a.b[i] = param(r.prefixes[i0 + i] + ".bias", r.n_each);
                    if (!a.w[i] || !a.b[i]) return BOFI_ERR_STATE;
                }
                if (!r.fold.empty()) {
                    a.gain = param(r.fold + ".a_2", r.K);
                    a.bln = param(r.fold + ".b_2", r.K);
                    if (!a.gain || !a.bln) return BOFI_ERR_STATE;
                }
                const size_t at = (size_t)i0 * r.n_each;      // first output row of this entry
                a.bout = r.out->b + at; a.cs = r.out->cs ? r.out->cs + at : nullptr;
                dsc.wout = (char*)r.out->w + at * r.K * tsz; dsc.wp = i0 ? nullptr : r.out->wp; dsc.Npad = r.out->Npad;      // (the fragment-major copy: of the whole weight, with its first entry)
                dsc.row0 = rows; rows += (a.n_each * a.nsrc + 3) / 4 * 4;
                dsc.blk0 = fblocks; if (dsc.wp) fblocks += (int)(((size_t)dsc.Npad * r.K / 8 + 255) / 256);
                lin_tab.push_back(dsc);
            }
        }
        for (const auto& r : norm_recipes) {
            const float *g = param(r.prefix + ".a_2", r.d), *b = param(r.prefix + ".b_2", r.d);
            if (!g || !b) return BOFI_ERR_STATE;
            add_copy(g, r.out->g, r.d);
            add_copy(b, r.out->b, r.d);
        }
        const float *ls = param("model.syn_embed.lut.weight", (int64_t)10 * d), *lt_w = param("model.tgt_embed.lut.weight", (int64_t)c.vocab * d);
        if (!ls || !lt_w) return BOFI_ERR_STATE;
        add_copy(ls, lut_syn, 10 * d);
        const std::string lp = "model.length_predictor";
        const float *lw1 = param(lp + ".Length_classifier1.weight", (int64_t)hh * d), *lb1 = param(lp + ".Length_classifier1.bias", hh);
        const float *sw1 = param(lp + ".Syntactic_classifier1.weight", (int64_t)hh * d), *sb1 = param(lp + ".Syntactic_classifier1.bias", hh);
        const float *lw2 = param(lp + ".Length_classifier2.weight", (int64_t)20 * hh), *lb2 = param(lp + ".Length_classifier2.bias", 20);
        const float *sw2 = param(lp + ".Syntactic_classifier2.weight", (int64_t)10 * hh), *sb2 = param(lp + ".Syntactic_classifier2.bias", 10);
        if (!lw1 || !lb1 || !sw1 || !sb1 || !lw2 || !lb2 || !sw2 || !sb2) return BOFI_ERR_STATE;
        add_copy(lw2, const_cast<float*>(heads.len_w2), 20 * hh); add_copy(lb2, const_cast<float*>(heads.len_b2), 20);
        add_copy(sw2, const_cast<float*>(heads.syn_w2), 10 * hh); add_copy(sb2, const_cast<float*>(heads.syn_b2), 10);
        {   // [PackLinDesc x n][CopyDesc x m] in one buffer
            const size_t lb = lin_tab.size() * sizeof(bofi::PackLinDesc), cb = copy_tab.size() * sizeof(bofi::CopyDesc), bytes = lb + cb;
            std::vector<char> img(bytes);
            memcpy(img.data(), lin_tab.data(), lb);
            memcpy(img.data() + lb, copy_tab.data(), cb);
            if (img != rt_cache) {
                // (rare path: the pack kernels of a previous repack -- possibly issued on ANOTHER stream -- may still be reading the table, and its upload the
                // pinned buffer: the whole device is waited out before either is touched)
                ENG_HIP(hipDeviceSynchronize());
                if (bytes > rt_bytes) {
                    if (rt_dev) (void)hipFree(rt_dev);
                    if (rt_pin) (void)hipHostFree(rt_pin);
                    rt_dev = rt_pin = nullptr; rt_bytes = 0;
                    ENG_HIP(hipMalloc(&rt_dev, bytes));
                    ENG_HIP(hipHostMalloc(&rt_pin, bytes, hipHostMallocDefault));
                    rt_bytes = bytes;
                }
                memcpy(rt_pin, img.data(), bytes);
                ENG_HIP(hipMemcpyAsync(rt_dev, rt_pin, bytes, hipMemcpyHostToDevice, s));
                rt_cache.swap(img);
            }
            const auto* ltab = static_cast<const bofi::PackLinDesc*>(rt_dev);
            const auto* ctab = reinterpret_cast<const bofi::CopyDesc*>(static_cast<const char*>(rt_dev) + lb);
            ENG_OK(bofi::launch_pack_lin_multi(ltab, (int)lin_tab.size(), rows, c.dtype, s));
            ENG_OK(bofi::launch_pack_frag_multi(ltab, (int)lin_tab.size(), fblocks, s));
            ENG_OK(bofi::launch_copy_multi(ctab, (int)copy_tab.size(), cblocks, s));
        }
        ENG_HIP(hipMemcpyAsync(lut_tok, lt_w, (size_t)c.vocab * d * 4, hipMemcpyDeviceToDevice, s));
        ENG_OK(bofi::launch_pack_heads(lw1, sw1, lb1, sb1, const_cast<float*>(heads.w1t), const_cast<float*>(heads.b1), d, hh, s));
        // input-independent tables of the bound layer: its input at (position p, label s) is lut_syn[s]*sqrt(d) + pe[p] (d_xt); K|V of all L*10 rows
        // and the query of row 0, with [LEN] at position 0 as a label (b_x0) and -- SAIC (TransformerModel.py:1903, 515-518) -- as tgt_embed([LEN]) (b_x0_sa)
        ENG_OK(bofi::launch_bound_table(lut_syn, lut_tok, pe, d_xt, b_x0, b_x0_sa, L, d, c.len_idx, s));
        LinOpt o; o.ln = &b_n0;
        ENG_OK(linear(d_xt, BOFI_DT_F32, d, t_kvself, b_kvtab, c.dtype, 2 * d, L * 10, o, s));
        ENG_OK(linear(b_x0, BOFI_DT_F32, d, t_qself, b_q0, c.dtype, d, 1, o, s));
        ENG_OK(linear(b_x0_sa, BOFI_DT_F32, d, t_qself, b_q0_sa, c.dtype, d, 1, o, s));
        ENG_OK(derive_bound_tables(s));
        if (loop_config_ok()) {
            const std::string bl = "model.length_predictor.LengthPredictor.0";
            BoundSrc b{};
            b.wq_self = param(bl + ".self_attn.linears.0.weight", (int64_t)d * d); b.bq_self = param(bl + ".self_attn.linears.0.bias", d);
            b.wk_self = param(bl + ".self_attn.linears.1.weight", (int64_t)d * d); b.bk_self = param(bl + ".self_attn.linears.1.bias", d);
            b.wv_self = param(bl + ".self_attn.linears.2.weight", (int64_t)d * d); b.bv_self = param(bl + ".self_attn.linears.2.bias", d);
            b.n0g = param(bl + ".sublayer.0.norm.a_2", d); b.n0b = param(bl + ".sublayer.0.norm.b_2", d);
            b.wo_self = param(bl + ".self_attn.linears.3.weight", (int64_t)d * d);
            b.wq_src = param(bl + ".src_attn.linears.0.weight", (int64_t)d * d); b.n1g = param(bl + ".sublayer.1.norm.a_2", d);
            b.wo_src = param(bl + ".src_attn.linears.3.weight", (int64_t)d * d);
            b.w1 = param(bl + ".ff.w_1.weight", (int64_t)dff * d); b.n2g = param(bl + ".sublayer.2.norm.a_2", d);
            b.w2 = param(bl + ".ff.w_2.weight", (int64_t)d * dff);
            b.lw1 = lw1; b.sw1 = sw1; b.hng = param(lp + ".norm.a_2", d);
            if (!b.wq_self || !b.bq_self || !b.wk_self || !b.bk_self || !b.wv_self || !b.bv_self || !b.n0g || !b.n0b || !b.wo_self || !b.wq_src || !b.n1g || !b.wo_src ||
                !b.w1 || !b.n2g || !b.w2 || !b.hng)
                return BOFI_ERR_STATE;
            ENG_OK(derive_bound_f16(b, s));
        }
        return BOFI_OK;
    }
    // BOFI_BOUND_LOOP (re-read after bofi_reload_env): 0 = the five-launch iterations of rounds 2-4 always, 1 (default) = the persistent loop kernel unless the caller
    // said its decodes run alone (bofi_engine_set_decodes_in_flight(1): the five launches are the shorter chain there -- 0.65 against 0.95 ms per 320 images),
    // 2 = the loop kernel whatever the hint
    static int bound_loop_knob() { return bofi::knob(BOFI_BOUND_LOOP); }
    bool bound_loop_ok(int R) const {
        const int k = settings.loop_mode >= 0 ? settings.loop_mode : bound_loop_knob();
        return loop_ready && loop_config_ok() && R <= 128 && k != 0 && (k == 2 || settings.in_flight != 1);
    }
    // update != 0: the whole loop on the engine's slot state (after launch_bound_init); update == 0: one iteration on a given layout, log-probabilities out
    // kv_beside: the launch also projects the columns behind the bounding layers' of kv_all (the decoder layers' cross K|V) from the encoder's output, in extra workgroups
    int bound_loop(int B, int R, const int* att_len, const int* ext_syn_in, const int* last_in, int update, float* len_logp, float* syn_logp, hipStream_t s,
                   bool kv_beside_now = false) {
        bofi::BoundLoopArgs a{};
        if (kv_beside_now) {
            bofi::RbGemmArgs& p = a.kv_pj;
            p.x = x_enc.x; p.ldx = cfg.d_model; p.wp = (const bofi::u32x4*)kv_all.wp; p.c = kv_all.b; p.cs = kv_all.cs; p.y = kv; p.ldy = kv_all.N; p.M = B * R; p.N = kv_all.Npad;
            a.kv_col0 = n_len * 2 * cfg.d_model; a.kv_in_flight = settings.in_flight;
        }
        a.wo_self = (const bofi::bl_u32x4*)b_o_self.wp16; a.x0b = b_x0b;
        a.wq_src = (const bofi::bl_u32x4*)b_q_src.wp16; a.cq = b_q_src.b;
        a.wo_src = (const bofi::bl_u32x4*)b_o_src.wp16; a.bo_src = b_o_src.b;
        a.w1 = (const bofi::bl_u32x4*)b_w1.wp16; a.c1 = b_w1.b;
        a.w2 = (const bofi::bl_u32x4*)b_w2.wp16; a.b2 = b_w2.b;
        a.wh = (const bofi::bl_u32x4*)b_heads.wp16; a.ch = b_heads.b;
        a.len_w2 = heads.len_w2; a.len_b2 = heads.len_b2; a.syn_w2 = heads.syn_w2; a.syn_b2 = heads.syn_b2;
        a.sctab = b_sctab; a.vtab = b_vtab;
        a.k = (const uint16_t*)kv; a.v = (const uint16_t*)kv + cfg.d_model; a.ldkv = kv_all.N; a.att_len = att_len;
        a.st = st; a.ext_syn_in = ext_syn_in; a.last_in = last_in; a.len_logp = len_logp; a.syn_logp = syn_logp;
        a.B = B; a.R = R; a.L = L; a.S = cfg.seq_length; a.hh = cfg.head_hidden; a.dff = cfg.d_ff;
        a.max_iters = update ? cfg.seq_length : 1; a.update = update;
        a.sat = st.counters + 4; a.wsat = b_wsat;             // (zeroed by launch_bound_init; the export hands it to the caller's word)
        a.xbuf = bl_xbuf; a.xctl = bl_xctl;                    // (two workgroups per group when the launcher's conditions hold: BOFI_BL_PAIR)
        return bofi::launch_bound_loop(a, s);
    }
    // y1 -> y3 partial slabs (by3): query projection + cross-attention, Wo_src, FFN, as the direct-operand kernels
    // of bound_ops.hip.  Returns -1 when the configuration is not theirs (bound_chain then takes the general kernels), else a status;
    // *parts = number of slabs in by3.
    // The decoder layers' cross K|V BESIDE the bounding loop (round 7): with several launches in flight their loops coincide -- 40 workgroups each -- and most of the chip has
    // nothing to run meanwhile, while the projection of all of kv_all sits in front of the loop as the tail of the encoder's last feed-forward launch.  The loop reads the
    // bounding layer's columns only; nothing reads the others before the filling pass.  In this form the tail carries the first n_len * 2 * d columns and the loop launch
    // projects the rest in workgroups of its own (bound_loop_kernel<5, true>): one kernel node, one stream, no fork / join.  On exactly where the loops are exposed and
    // today's chain has the tail: the pair form of the loop kernel by the library's own rule (BOFI_BL_PAIR = 1, <= BOFI_BL_PAIR_MAX_B images), not a decode running alone (the
    // decodes-in-flight hint also sizes the projection's share of the chip), <= 36 regions, the whole decode in one call (a phased call's ENCODE promises the whole stacked
    // K|V), the row-block encoder with the projection tail.  Else today's chain, unchanged.
    bool bound_kv_beside_ok(int B, int R, int phases) const {
        if (!settings.kv_beside || phases || enc.empty() || settings.in_flight == 1 || R > 36 || !bound_loop_ok(R) || exp_skip("loop") || exp_skip("encoder")) return false;
        // (the pair as the library's own choice: BOFI_BL_PAIR = 2 forces pairs at any size for the tests of the pair itself -- they compare its bits with one workgroup per
        // group's -- and moves nothing else in the chain)
        if (bofi::knob(BOFI_BL_PAIR) != 1 || !bofi::bound_loop_pairs(B, cfg.d_ff, 1, bl_xbuf && bl_xctl)) return false;
        const int M = B * R, col0 = n_len * 2 * cfg.d_model;
        const EncLayer& l = enc.back();
        return kv_all.Npad == kv_all.N && col0 >= 512 && col0 < kv_all.N && fold_rb_ok(l.qkv, M) && fold_rb_ok(kv_all, M) && ffn_proj_ok(l.w1, l.w2, kv_all, M);
    }
    int bound_chain_lean(int B, int R, const int* att_len, const Rows& r, hipStream_t s, int* parts) {
        const bool lean_on = bofi::knob(BOFI_BOUND_LEAN) != 0;
        const int d = cfg.d_model;
        if (!(lean_on && cfg.dtype == BOFI_DT_BF16 && d == 512 && cfg.heads == 8 && R <= 64 && cfg.d_ff % 512 == 0 && cfg.d_ff / 512 <= 4)) return -1;
        {   bofi::BoundQAttnArgs a{};
            a.x = (const uint16_t*)y1.xb; a.stats = y1.st; a.wq = (const uint16_t*)b_q_src.w; a.bias = b_q_src.b; a.colsum = b_q_src.cs;
            a.k = (const uint16_t*)kv; a.v = (const uint16_t*)kv + d; a.ldkv = kv_all.N; a.att_len = att_len; a.out = (uint16_t*)bctx2;
            a.B = B; a.R = R; a.d = d; a.H = cfg.heads; a.skip_if_ge = r.skip; a.skip_threshold = r.thr;
            ENG_OK(bofi::launch_bound_qattn(a, s)); }
        {   bofi::RowGemmArgs a{};                   // y2 = y1 + Wo_src . ctx2 + bo
            a.x = (const uint16_t*)bctx2; a.ldx = d; a.w = (const uint16_t*)b_o_src.w; a.bias = b_o_src.b; a.residual = y1.x; a.ldr = d;
            a.y = y2.x; a.ldy = d; a.yb = (uint16_t*)y2.xb; a.ldyb = d; a.stats_out = st_b16; a.M = B; a.N = d; a.K = d; a.splitk = 1;
            a.skip_if_ge = r.skip; a.skip_threshold = r.thr;
            ENG_OK(bofi::launch_rowgemm(a, s)); }
        {   bofi::RowGemmArgs a{};                   // h = relu(W1 . LN(y2) + b1)
            a.x = (const uint16_t*)y2.xb; a.ldx = d; a.w = (const uint16_t*)b_w1.w; a.bias = b_w1.b; a.stats = st_b16; a.stats_groups = d / 16;
            a.colsum = b_w1.cs; a.yb = (uint16_t*)bh; a.ldyb = cfg.d_ff; a.M = B; a.N = cfg.d_ff; a.K = d; a.splitk = 1; a.relu = 1;
            a.skip_if_ge = r.skip; a.skip_threshold = r.thr;
            ENG_OK(bofi::launch_rowgemm(a, s)); }
        *parts = cfg.d_ff / 512;
        {   bofi::RowGemmArgs a{};                   // y3 = y2 + W2 . h + b2 as `parts` partial slabs
            a.x = (const uint16_t*)bh; a.ldx = cfg.d_ff; a.w = (const uint16_t*)b_w2.w; a.bias = b_w2.b; a.residual = y2.x; a.ldr = d;
            a.y = by3; a.ldy = d; a.M = B; a.N = d; a.K = cfg.d_ff; a.splitk = *parts;
            a.skip_if_ge = r.skip; a.skip_threshold = r.thr;
            ENG_OK(bofi::launch_rowgemm(a, s)); }
        return BOFI_OK;
    }
    // One bounding iteration's row 0 from y1 (left by the previous bound_tail(..., BOUND_ATTN)) to the feed-forward output as *parts partial slabs
    // in by3: the lean form when it applies, else query projection, cross-attention of the one query row over slot 0, W_o_src, w_1 and w_2 as the
    // general kernels.  r: the early-out word of the loop this iteration belongs to.
    int bound_chain(int B, int R, const int* att_len, const Rows& r, hipStream_t s, int* parts) {
        const int rc = bound_chain_lean(B, R, att_len, r, s, parts);
        if (rc >= 0) return rc;
        const int dt = cfg.dtype, d = cfg.d_model;
        ENG_OK(folded(y1, b_q_src, bq2, dt, d, B, r, s));
        ENG_OK(bofi::launch_attention(cross_attn_args(bq2, 0, bctx2, B, 1, R, att_len, r), s));
        ENG_OK(close_sublayer(bctx2, b_o_src, y2, B, r, s, y1.x, d));
        ENG_OK(folded(y2, b_w1, bh, dt, cfg.d_ff, B, r, s, 1));
        *parts = (cfg.d_ff % (4 * 128) == 0) ? 4 : 1;     // K = d_ff split 4 ways: 4x the workgroups, a quarter of the K loop
        LinOpt o; o.residual = y2.x; o.ldr = d; o.rows = r; o.splitk = *parts;
        return linear(bh, dt, cfg.d_ff, b_w2, by3, BOFI_DT_F32, d, B, o, s);
    }
    // ---- row-block sublayer kernels (rowblock.hip, bf16 engine at the reference's width): the attention sublayer (attention + output
    // projection + residual) and the feed-forward sublayer as one launch each.  rb_attn / rb_ffn / fold_linear_rb return -1 when the
    // configuration or the shape is not theirs, else a status; project / attn_sublayer / ffn_sublayer below own the fall-back to the separate
    // attention / GEMM launches.  want_copy: the next consumer is a tiled LayerNorm-folded GEMM (it reads the compute-dtype copy and the row
    // statistics); the row-block kernels read the float32 stream itself.  All of these run every row: a launch with an early-out word or a
    // row list (Rows) goes through folded / close_sublayer / decoder_layer_tiled and never reaches a row-block kernel.
    bool rb_ok() const { return cfg.dtype == BOFI_DT_BF16 && cfg.d_model == 512 && cfg.heads == 8; }
    // the row-block kernels are a fixed latency chain per workgroup (one block of rows, the sublayer's whole weight stream): they pay
    // from a few thousand rows on, where the tiled GEMMs' prologue / epilogue and the hidden tensor's round trip cost more
    // (BOFI_RB_MIN_ROWS: 0 = always, a huge value = never; re-read after bofi_reload_env.  Kernel family and launch size are then
    // decoupled: under ONE family a row's result does not depend on what else is in the launch -- bit for bit)
    static int rb_min_rows() {
        return bofi::knob(BOFI_RB_MIN_ROWS);
    }
    // timing-only ablation switches (results INVALID): compiled in only by `BOFI_EXPERIMENTS=1 python -m boficap_amd.build --force`
#ifdef BOFI_EXPERIMENTS
    static bool exp_skip(const char* what) {
        const char* v = bofi::knob_str(BOFI_EXP_SKIP);
        static bool told = false;
        if (v && !told) { told = true; fprintf(stderr, "[boficap_hip] BOFI_EXP_SKIP=%s: kernels skipped, RESULTS INVALID\n", v); }
        return v && strstr(v, what);
    }
#else
    static constexpr bool exp_skip(const char*) { return false; }
#endif
    // pj (optional): the LayerNorm-folded [512, 512] projection that reads this sublayer's output next (the decoder layer's cross-attention queries), computed by the SAME
    // launch from each block while it sits in LDS (pj_y bf16, pitch pj_ldy); attn_proj_ok says when the attention kernel takes it (BOFI_RB_ATTN_PROJ, re-read after
    // bofi_reload_env: 0 = never, 1 (default) = when launches overlap, 2 = always)
    bool attn_proj_ok(const bofi::AttnArgs& at, const Lin& o, const Lin& pj) const {
        const int v = bofi::knob(BOFI_RB_ATTN_PROJ);
        const int M = at.B * at.Lq;
        return v && (v == 2 || settings.in_flight != 1) && bofi::knob(BOFI_RB_ATTN) != 0 && bofi::knob(BOFI_RB_ATTN_W) == 0 && rb_ok() && o.wp && fold_rb_ok(pj, M) &&
               pj.Npad == 512 && !at.skip_if_ge && at.kdiv <= 1 && !at.q_start && !at.drop_thresh && !at.klen_sq && at.Lq <= bofi::RB_ATTN_PJ_MAX_LQ && at.Lk <= bofi::RB_ATTN_PJ_MAX_LK && M >= rb_min_rows() &&
               !exp_skip("attn") && !exp_skip("qkv");
    }
    int rb_attn(const bofi::AttnArgs& at, const Lin& o, const Stream& t, bool want_copy, hipStream_t s, const Lin* pj, void* pj_y, int pj_ldy) {
        const bool on = bofi::knob(BOFI_RB_ATTN) != 0;
        if (exp_skip("attn")) return BOFI_OK;
        if (!on || !rb_ok() || !o.wp || at.skip_if_ge || at.kdiv > 1 || at.q_start || at.drop_thresh || at.B * at.Lq < rb_min_rows()) return -1;
        bofi::RbAttnArgs a{};
        a.q = (const uint16_t*)at.q; a.ldq = at.ldq; a.k = (const uint16_t*)at.k; a.ldk = at.ldk; a.v = (const uint16_t*)at.v; a.ldv = at.ldv;
        a.B = at.B; a.Lq = at.Lq; a.Lk = at.Lk; a.klen = at.klen; a.klen_sb = at.klen_sb; a.klen_sq = at.klen_sq; a.klen_bias = at.klen_bias;
        a.klen_shared_last = at.klen_shared_last; a.wop = (const bofi::u32x4*)o.wp; a.bo = o.b; a.x = t.x; a.ldx = cfg.d_model; a.y = t.x; a.ldy = cfg.d_model;
        a.yb = want_copy ? (uint16_t*)t.xb : nullptr; a.stats_out = want_copy ? t.st : nullptr;
        a.alone = settings.in_flight == 1;
        if (pj) { a.pj_wp = (const bofi::u32x4*)pj->wp; a.pj_c = pj->b; a.pj_cs = pj->cs; a.pj_y = (uint16_t*)pj_y; a.pj_ldy = pj_ldy; a.yb = nullptr; a.stats_out = nullptr; }
        return bofi::launch_rb_attn(a, s);
    }
    // a LayerNorm-folded projection (K = d_model) of the residual stream x32 as a row-block kernel: it reads the float32 stream itself
    // (no compute-dtype copy, no row statistics from the producer).  -1: not its configuration.
    bool fold_rb_ok(const Lin& l, int M) const {
        const bool on = bofi::knob(BOFI_RB_GEMM) != 0;
        return on && rb_ok() && l.wp && l.cs && l.K == 512 && M >= rb_min_rows();
    }
    int fold_linear_rb(const float* x32, const Lin& l, void* y, int y_f32, int ldy, int M, hipStream_t s) {
        if (!fold_rb_ok(l, M)) return -1;
        if (exp_skip(y_f32 ? "gen" : l.Npad <= 1536 ? "qkv" : "kv")) return BOFI_OK;
        bofi::RbGemmArgs a{};
        a.x = x32; a.ldx = cfg.d_model; a.wp = (const bofi::u32x4*)l.wp; a.c = l.b; a.cs = l.cs; a.y = y; a.ldy = ldy; a.y_f32 = y_f32; a.M = M; a.N = l.Npad; a.relu = 0;
        a.alone = settings.in_flight == 1;
        return bofi::launch_rb_gemm(a, s);
    }
    // the generator as the row-block kernel over the padded weight (what enqueue_fill runs from BOFI_RB_MIN_ROWS rows on)
    bool gen_rb_ok(int M) const { return bofi::knob(BOFI_GEN_PAD) != 0 && gen_padded() && fold_rb_ok(gen, M); }
    bool ffn_sublayer_ok(const Lin& w1, const Lin& w2, int M) const {
        const bool on = bofi::knob(BOFI_RB_FFN) != 0;
        return on && rb_ok() && w1.wp && w2.wp && w1.cs && cfg.d_ff % 512 == 0 && cfg.d_ff <= 2560 && M >= rb_min_rows();
    }
    // pj (optional): the LayerNorm-folded projection that reads this sublayer's output next (the next layer's q|k|v, the stacked cross K|V), computed by
    // the SAME launch from each closed block while it sits in LDS (pj_y, pitch pj_ldy); ffn_proj_ok says when the feed-forward kernel takes it
    // (BOFI_RB_FFN_PROJ, re-read after bofi_reload_env: 0 = never, 1 (default) = when launches overlap, 2 = always)
    bool ffn_proj_ok(const Lin& w1, const Lin& w2, const Lin& pj, int M) const {
        const int v = bofi::knob(BOFI_RB_FFN_PROJ);
        // (a decode running alone keeps the separate launches of 64-row blocks: measured 0.515 against 0.523 ms per batch with the narrow projections fused,
        // 0.536 with all of them)
        const int maxn = bofi::knob(BOFI_RB_FFN_PROJ_MAXN);          // developer knob: projections wider than this stay launches of their own (0: no limit)
        return v && (v == 2 || settings.in_flight != 1) && ffn_sublayer_ok(w1, w2, M) && fold_rb_ok(pj, M) && pj.Npad >= 512 && (!maxn || pj.Npad <= maxn) && !exp_skip("ffn") &&
               !exp_skip("qkv") && !exp_skip("kv");
    }
    // The attention sublayer SPLIT (round 6): the attention core as the light kernel of attn_bf16.hip (context rows to memory as bf16: no W_o stream, no
    // 80-120 KB of LDS, many workgroups per CU) and W_o + residual as the HEAD segment of the feed-forward launch that follows (rb_ffn5_kernel<.., HEAD>: 80 rows per weight
    // byte, x1 never in memory) instead of rb_attn_kernel's attention + W_o + residual in one workgroup.  Gate (profiles/r06_gate_attn_split.txt, four streams): the encoder's
    // sublayer 21.4 -> 11.6 + 1.0 us, the filling pass's cross-attention 14.8 -> 7.9 + 2.2 us per 320 images -- four streams of ONE kernel each.  Inside the decode
    // (profiles/r06_attn_split_ab.txt, r06_split{0,1}_kernel_stats.txt) the cores save 132 us of kernel time per 320 images (30.1 -> 19.6 and 37.8 -> 22.4 us per launch
    // in flight) and the head segment costs 116 (115 -> 126 us per feed-forward launch: the producers wait while the consumers run W_o): +1.2 % at 1 024 images per
    // launch, where a launch's blocks come in several waves per CU and hide the longer chain, -1 ... -4 % at 320, where they do not.  Hence BOFI_RB_ATTN_SPLIT (re-read
    // after bofi_reload_env): 0 = never, 1 (default) = when launches overlap AND the launch holds at least BOFI_RB_ATTN_SPLIT_MIN_B (512) images, 2 = always.  Needs the
    // feed-forward sublayer directly behind the attention sublayer and no consumer of the bf16 copy / statistics.
    // Shapes the fused sublayer kernel does not take (more than 48 keys or 40 queries: real bottom-up features have up to 100 regions) are split at EVERY launch size: the
    // alternative there is the attention core + a tiled GEMM for W_o + the residual stream's round trip (profiles/r06_regions_sweep.txt).
    // which: 1 = the encoder's self-attention, 2 = the filling pass's cross-attention (developer knob BOFI_RB_ATTN_SPLIT_WHICH, a mask of these; default both).
    bool attn_split_ok(const bofi::AttnArgs& at, const Lin& o, const Lin& w1, const Lin& w2, int which) const {
        if (!(bofi::knob(BOFI_RB_ATTN_SPLIT_WHICH) & which)) return false;
        const int v = bofi::knob(BOFI_RB_ATTN_SPLIT);
        const int M = at.B * at.Lq;
        const bool beyond = (at.Lq > bofi::RB_ATTN_MAX_LQ || at.Lk > bofi::RB_ATTN_MAX_LK) && M >= rb_min_rows();
        return v && (v == 2 || beyond || (settings.in_flight != 1 && at.B >= bofi::knob(BOFI_RB_ATTN_SPLIT_MIN_B))) && bofi::knob(BOFI_RB_ATTN) != 0 && rb_ok() && o.wp &&
               ffn_sublayer_ok(w1, w2, M) && !at.skip_if_ge && at.kdiv <= 1 &&
               !at.q_start && !at.drop_thresh && at.Lq <= 128 && at.Lk <= 128 && !exp_skip("attn") && !exp_skip("ffn");
    }
    int rb_ffn(const Lin& w1, const Lin& w2, float* x, void* xb, float* stats, int M, hipStream_t s, const Lin* pj, void* pj_y, int pj_ldy, const Lin* head,
               const void* head_ctx) {
        if (!ffn_sublayer_ok(w1, w2, M)) return -1;
        if (exp_skip("ffn")) return BOFI_OK;
        bofi::RbFfnArgs a{};
        if (head) { a.head_wop = (const bofi::u32x4*)head->wp; a.head_bo = head->b; a.head_ctx = (const uint16_t*)head_ctx; a.head_ldc = cfg.d_model; }
        if (pj) { a.pj_wp = (const bofi::u32x4*)pj->wp; a.pj_c = pj->b; a.pj_cs = pj->cs; a.pj_y = pj_y; a.pj_ldy = pj_ldy; a.pj_N = pj->Npad; }
        a.x = x; a.ldx = cfg.d_model; a.w1p = (const bofi::u32x4*)w1.wp; a.c1 = w1.b; a.cs1 = w1.cs; a.w2p = (const bofi::u32x4*)w2.wp; a.b2 = w2.b;
        a.y = x; a.ldy = cfg.d_model; a.yb = (uint16_t*)xb; a.stats_out = stats; a.M = M; a.dff = cfg.d_ff;
        a.alone = settings.in_flight == 1;
        return bofi::launch_rb_ffn(a, s);
    }
    // ---- one function per sublayer kind on ALL M rows of stream t: the row-block kernel when the shape is its, else the tiled launches
    // y = l(LayerNorm(t)): y_f32 = float32 out (the generator), else the compute dtype
    int project(const Stream& t, const Lin& l, void* y, int y_f32, int ldy, int M, hipStream_t s) {
        const int rc = fold_linear_rb(t.x, l, y, y_f32, ldy, M, s);
        return rc >= 0 ? rc : folded(t, l, y, y_f32 ? BOFI_DT_F32 : cfg.dtype, ldy, M, Rows{}, s);
    }
    // t += W_o . attention(at) + b_o.  split (attn_split_ok; the caller puts the feed-forward sublayer directly behind and hands it `o` as its head):
    // only the light core runs here.  Else the fused kernel -- with pj, the projection that reads this sublayer's output next, as its tail when
    // attn_proj_ok: *pj_made -- else attention core + closing GEMM (pj is then the caller's to make).
    int attn_sublayer(const bofi::AttnArgs& at, const Lin& o, const Stream& t, bool want_copy, bool split, hipStream_t s, const Lin* pj = nullptr,
                      void* pj_y = nullptr, int pj_ldy = 0, bool* pj_made = nullptr) {
        if (split) return bofi::launch_attention(at, s);
        const bool tail = pj && attn_proj_ok(at, o, *pj);
        const int rc = rb_attn(at, o, t, want_copy, s, tail ? pj : nullptr, pj_y, pj_ldy);
        if (pj_made) *pj_made = tail && rc == BOFI_OK;
        if (rc >= 0) return rc;
        ENG_OK(bofi::launch_attention(at, s));
        return close_sublayer(at.out, o, t, at.B * at.Lq, Rows{}, s);
    }
    // t += w_2 . relu(w_1 . LayerNorm(t)).  head: the W_o of a split attention sublayer whose context rows are in ctx.  pj: the projection that reads
    // this sublayer's output next; it rides the launch when nothing needs the copy and ffn_proj_ok: *pj_made (else it is the caller's to make).
    int ffn_sublayer(const Lin& w1, const Lin& w2, const Stream& t, bool want_copy, int M, hipStream_t s, const Lin* head, const Lin* pj, void* pj_y,
                     int pj_ldy, bool* pj_made) {
        const bool tail = pj && !want_copy && ffn_proj_ok(w1, w2, *pj, M);
        *pj_made = tail;
        const int rc = rb_ffn(w1, w2, t.x, want_copy ? t.xb : nullptr, want_copy ? t.st : nullptr, M, s, tail ? pj : nullptr, tail ? pj_y : nullptr,
                              tail ? pj_ldy : 0, head, ctx);
        if (rc >= 0) return rc;
        ENG_OK(folded(t, w1, hdn, cfg.dtype, cfg.d_ff, M, Rows{}, s, 1));
        return close_sublayer(hdn, w2, t, M, Rows{}, s);
    }
    // One decoder layer as its eight tiled launches (q|k|v, self-attention, W_o, q_src, cross-attention over slot kv_i, o_src, w_1, w_2) on the rows r
    // of stream t, B images of Lq rows: the dense bounding pass and the SAIC decoder pass, whose launches carry an early-out word / a row list.
    // self_klen (+ bias): the self-attention's key prefix per (image, row) at pitch L.
    int decoder_layer_tiled(const DecLayer& l, int kv_i, const Stream& t, void* qkv_buf, int B, int Lq, int R, const int* self_klen, int self_klen_bias,
                            const int* att_len, const Rows& r, hipStream_t s) {
        const int d = cfg.d_model, dt = cfg.dtype, M = B * Lq;
        ENG_OK(folded(t, l.qkv, qkv_buf, dt, 3 * d, M, r, s));
        bofi::AttnArgs a = self_attn_args(qkv_buf, B, Lq, r);
        a.klen = self_klen; a.klen_sb = L; a.klen_sq = 1; a.klen_bias = self_klen_bias;
        ENG_OK(bofi::launch_attention(a, s));
        ENG_OK(close_sublayer(ctx, l.o, t, M, r, s));
        ENG_OK(folded(t, l.q_src, qs, dt, d, M, r, s));
        ENG_OK(bofi::launch_attention(cross_attn_args(qs, kv_i, ctx, B, Lq, R, att_len, r), s));
        ENG_OK(close_sublayer(ctx, l.o_src, t, M, r, s));
        ENG_OK(folded(t, l.w1, hdn, dt, cfg.d_ff, M, r, s, 1));
        return close_sublayer(hdn, l.w2, t, M, r, s);
    }
    int enqueue_encode(const void* feats, int feats_dtype, const int* att_len, int B, int R, float* memory_out, hipStream_t s, bool kv_bound_only = false);
    int enqueue_bound_iter(int B, int R, const int* att_len, const int* ext_syn, const int* last, int update, float* len_logp,
                           float* syn_logp, bool early, hipStream_t s);
    int enqueue_fill(const int* att_len, int B, int R, int flags, int64_t* seq, float* seq_logprob, hipStream_t s);
    int enqueue_bound_dense(const int* att_len, int B, int R, hipStream_t s);
    int enqueue_decode_saic(const void* feats, int feats_dtype, const int* att_len, int B, int R, int flags, int64_t* seq,
                            float* seq_logprob, int* phrase_num, int* phrase_length, int64_t* phrase_syn, int* bound_iters, hipStream_t s);
    int enqueue_decode(const void* feats, int feats_dtype, const int* att_len, int B, int R, int flags, int64_t* seq,
                       float* seq_logprob, int* phrase_num, int* phrase_length, int64_t* phrase_syn, float* memory_out,
                       int* bound_iters, hipStream_t s);
};

// ================================================================================================
// kv_bound_only (bound_kv_beside_ok): the last feed-forward launch's tail projects the bounding layers' columns of kv_all only -- a column's value does not depend on how
// many are projected -- and the caller's loop launch makes the rest
int bofi_engine::enqueue_encode(const void* feats, int feats_dtype, const int* att_len, int B, int R, float* memory_out,
                                hipStream_t s, bool kv_bound_only) {
    const int d = cfg.d_model, dt = cfg.dtype, M = B * R;
    if (exp_skip("encoder")) return BOFI_OK;           // (experiments build: the whole encoder phase)
    // The residual stream x_enc stays float32; every GEMM that closes a sublayer also writes a copy in
    // the compute dtype and per-row partial sums, from which the next pre-norm LayerNorm is applied
    // inside the consuming GEMM's epilogue (no LayerNorm launches).
    if (feats_dtype != dt) {                         // float32 features into a bf16 engine: one conversion pass
        ENG_OK(bofi::launch_cast_bf16((const float*)feats, feats_t, (size_t)M * cfg.feat, s));
        feats = feats_t; feats_dtype = dt;
    }
    {   // att_embed: Linear + ReLU, rows past an image's region count forced to 0 (AttModel.py:46-51)
        LinOpt o; o.relu = 1; o.row_len = att_len; o.rpg = R; o.stats_out = x_enc.st; o.y2 = x_enc.copy();
        ENG_OK(linear(feats, feats_dtype, cfg.feat, att_embed, x_enc.x, BOFI_DT_F32, d, M, o, s));
    }
    bool proj_made = false;       // this layer's q|k|v (after the last layer: the cross K|V) came out of the previous feed-forward launch
    for (size_t li = 0; li < enc.size(); ++li) {
        auto& l = enc[li];
        if (!proj_made) ENG_OK(project(x_enc, l.qkv, qkv, 0, 3 * d, M, s));
        bofi::AttnArgs a = self_attn_args(qkv, B, R);
        a.klen = att_len; a.klen_sb = 1;
        const bool ffn_rb = ffn_sublayer_ok(l.w1, l.w2, M);
        // (consumers of this layer's output that read the copy + statistics: tiled GEMMs; memory_out is a LayerNorm of the float32 stream itself)
        const bool need_copy = !(fold_rb_ok(l.qkv, M) && fold_rb_ok(kv_all, M));
        // split: the attention core now, W_o + residual as the head of the feed-forward launch
        const bool split = ffn_rb && !need_copy && attn_split_ok(a, l.o, l.w1, l.w2, 1);
        ENG_OK(attn_sublayer(a, l.o, x_enc, !ffn_rb, split, s));
        // the consumer of this layer's output: the next layer's q|k|v, or the stacked cross K|V
        const bool last = li + 1 == enc.size();
        Lin kv_bound = kv_all;                                           // (the same operands, the first columns: the bounding layers' K|V)
        if (kv_bound_only) kv_bound.N = kv_bound.Npad = n_len * 2 * d;
        const Lin& nxt = last ? (kv_bound_only ? kv_bound : kv_all) : enc[li + 1].qkv;
        ENG_OK(ffn_sublayer(l.w1, l.w2, x_enc, need_copy, M, s, split ? &l.o : nullptr, &nxt, last ? kv : qkv, last ? kv_all.N : 3 * d, &proj_made));
        if (last && kv_bound_only && !proj_made) return BOFI_ERR_STATE;  // (bound_kv_beside_ok saw this tail)
    }
    if (memory_out) ENG_OK(bofi::launch_layernorm(x_enc.x, enc_norm.g, enc_norm.b, memory_out, BOFI_DT_F32, M, d, s));
    // cross-attention K|V of the bound layer and of every decoder layer in one GEMM on memory =
    // encoder.norm(x_enc), the norm folded in
    if (!proj_made) ENG_OK(project(x_enc, kv_all, kv, 0, kv_all.N, M, s));
    return BOFI_OK;
}

int bofi_engine::enqueue_bound_iter(int B, int R, const int* att_len, const int* ext_syn, const int* last, int update,
                                    float* len_logp, float* syn_logp, bool early, hipStream_t s) {
    // One bounding iteration AFTER the row-0 self-attention sublayer output y1 (with its copy and row statistics)
    // has been produced by the previous bound_tail(..., BOUND_ATTN).
    if (exp_skip("loop")) return BOFI_OK;
    int parts = 0;
    ENG_OK(bound_chain(B, R, att_len, early ? Rows{st.counters, B} : Rows{}, s, &parts));
    // heads + bookkeeping, fused with the next iteration's row-0 self-attention
    const int flags = BOUND_HEADS | (update ? (BOUND_UPDATE | BOUND_ATTN) : 0) | (early ? BOUND_EARLY : 0);
    return bound_tail(by3, parts, update ? nullptr : ext_syn, update ? nullptr : last, B, flags, len_logp, syn_logp, s);
}

// The bounding loop in its dense form (LengthPredictor_UIC.forward TransformerModel.py:357-383 as the reference runs it): per
// iteration the whole bound sequence -- all L = S + 2 rows, pos_embed(syn_embed(extend_phrase_syn)) -- goes through every one of
// the N_len layers (self-attention under tgt_mask, whose rows are key prefixes: BoundState.klen; cross-attention over the
// memory; FFN), then the final norm, the heads and the bookkeeping on row 0 (the tail kernel without its self-attention part).
// Needed for N_len >= 2, where the upper layers read the lower layers' outputs of every visible row; with
// BOFI_BOUND_DENSE=1 it also serves N_len = 1 as a cross-check of the incremental form.
int bofi_engine::enqueue_bound_dense(const int* att_len, int B, int R, hipStream_t s) {
    const int d = cfg.d_model, S = cfg.seq_length;
    const Rows live{st.counters, B};               // every launch returns at once when all B images are finished
    for (int it = 0; it < S; ++it) {
        // input rows: the syntactic table stands where launch_embed_rows takes the word table (no second term)
        ENG_OK(bofi::launch_embed_rows(lut_syn, nullptr, pe, st.ext_syn, nullptr, L, 0, B, L, d, 0, xw.x, xw.copy(), cfg.dtype, xw.st, nullptr, s));
        for (size_t li = 0; li < blay.size(); ++li)
            ENG_OK(decoder_layer_tiled(blay[li], (int)li, xw, qkv, B, L, R, st.klen, 0, att_len, live, s));
        ENG_OK(bound_tail(xw.x, 1, nullptr, nullptr, B, BOUND_HEADS | BOUND_UPDATE | BOUND_EARLY, nullptr, nullptr, s, false, 0, L * d));
    }
    return BOFI_OK;
}

int bofi_engine::enqueue_decode(const void* feats, int feats_dtype, const int* att_len, int B, int R, int flags, int64_t* seq,
                                float* seq_logprob, int* phrase_num, int* phrase_length, int64_t* phrase_syn,
                                float* memory_out, int* bound_iters, hipStream_t s) {
    const int S = cfg.seq_length;
    // phases (BOFI_FLAG_PHASE_*): none of the bits = the whole decode; else only the named parts (a pipelining caller enqueues them as separate calls)
    const int ph = flags & (BOFI_FLAG_PHASE_ENCODE | BOFI_FLAG_PHASE_BOUND | BOFI_FLAG_PHASE_FILL);
    const bool do_enc = !ph || (ph & BOFI_FLAG_PHASE_ENCODE), do_bound = !ph || (ph & BOFI_FLAG_PHASE_BOUND), do_fill = !ph || (ph & BOFI_FLAG_PHASE_FILL);
    const bool kv_beside_now = bound_kv_beside_ok(B, R, ph);
    if (do_enc) ENG_OK(enqueue_encode(feats, feats_dtype, att_len, B, R, memory_out, s, kv_beside_now));
    // ---- bounding pass (core_NAIC TransformerModel.py:1833-1870)
    if (do_bound) {
    ENG_OK(bofi::launch_bound_init(st, B, L, cfg.pad_idx, cfg.len_idx, s));
    if (bound_dense) {
        ENG_OK(enqueue_bound_dense(att_len, B, R, s));
    } else if (bound_loop_ok(R) && !exp_skip("loop")) {
        // one launch: a workgroup per 16 images runs every iteration and leaves when its images are finished (no iteration budget to enqueue)
        ENG_OK(bound_loop(B, R, att_len, nullptr, nullptr, 1, nullptr, nullptr, s, kv_beside_now));
    } else {
        ENG_OK(bound_tail(nullptr, 1, nullptr, nullptr, B, BOUND_ATTN, nullptr, nullptr, s));
#ifdef BOFI_EXPERIMENTS
        const int exp_iters = bofi::knob(BOFI_EXP_ITERS);
        static bool told = false;
        if (bofi::knob_set(BOFI_EXP_ITERS) && !told) { told = true; fprintf(stderr, "[boficap_hip] BOFI_EXP_ITERS=%d: bounding loop truncated, RESULTS INVALID\n", exp_iters); }
#else
        constexpr int exp_iters = 0;                 // (timing experiment, experiments build only)
#endif
        // (opt.bound_iter_cap: a caller that knows how many iterations its captions take enqueues that many + a margin instead of
        // all S -- an iteration past the last live one is five launches that return at once -- and decodes again without the cap when the
        // count of live iterations, *bound_iters, reaches the cap: the loop may then not have ended)
        const int n_iters = exp_iters ? exp_iters : (opt.bound_iter_cap > 0 && opt.bound_iter_cap < S ? opt.bound_iter_cap : S);
        for (int it = 0; it < n_iters; ++it)
            ENG_OK(enqueue_bound_iter(B, R, att_len, st.ext_syn, st.last, 1, nullptr, nullptr, true, s));
    }
    }
    if (do_fill) {
        ENG_OK(enqueue_fill(att_len, B, R, flags, seq, seq_logprob, s));
        ENG_OK(bofi::launch_bound_export(st, B, L, S, phrase_num, phrase_length, phrase_syn, bound_iters, s, opt.live_max, opt.sat_out));
    }
    return BOFI_OK;
}

// ---- filling pass (decode_NA :570-587) on the slot layout in st.ext_syn / st.last and the cross K|V of the preceding
// encode; with refinement the pass is repeated with the previous round's ids as decoder input tokens (the glat_input hook
// of decode_NA :570-574 -- the reference has no refinement loop itself).  Under BOFI_FLAG_MASK_PREDICT the extra passes are mask-predict rounds: every pass's
// epilogue writes ids and row statistics into the engine's scratch, mask_predict_step (refine.hip) merges them into the state and makes the next pass's
// input ids (BOS at the least confident positions), and the last step writes the caller's seq, row statistics and emitted rounds.
int bofi_engine::enqueue_fill(const int* att_len, int B, int R, int flags, int64_t* seq, float* seq_logprob, hipStream_t s) {
    const int d = cfg.d_model, dt = cfg.dtype, S = cfg.seq_length, M = B * S;
    if (exp_skip("filling")) return BOFI_OK;           // (experiments build: the whole filling pass incl. the vocabulary epilogue)
    const int rounds = 1 + ((flags >> BOFI_FLAG_REFINE_SHIFT) & 15);
    float* lg = seq_logprob ? seq_logprob : logits;
    const int gen_pad = bofi::knob(BOFI_GEN_PAD);      // developer knob: 0 = in place, one-tile kernel
    const bool gen_rb = gen_rb_ok(M);
    // BOFI_FLAG_IDS_ONLY where the row-block generator would run: generator + epilogue as ONE launch that keeps the distribution on the CU (rb_vocab_kernel)
    const bool fused = (flags & BOFI_FLAG_IDS_ONLY) && gen_rb;
    if (no_logits && !fused) return fail(BOFI_ERR_STATE, "this fork has no vocabulary-wide buffers: BOFI_FLAG_IDS_ONLY decodes that take the fused generator only");
    const bool mp = (flags & BOFI_FLAG_MASK_PREDICT) != 0;
    // where a pass's epilogue leaves its ids and row statistics, and what the next pass's embedding reads
    int64_t* const ep_seq = mp ? mp_fresh_ids : seq;
    float* const ep_plogp = mp ? mp_fresh_plogp : opt.row_plogp;
    float* const ep_chosen = mp ? mp_fresh_chosen : opt.row_chosen;
    const int64_t* const fed = mp ? mp_next_ids : seq;
    auto refine_step = [&](int round) -> int {
        if (!mp) return BOFI_OK;
        bofi::MaskPredictArgs m{};
        m.ids = mp_ids; m.chosen = mp_chosen; m.plogp = mp_plogp; m.round = mp_round;
        m.fresh_ids = mp_fresh_ids; m.fresh_chosen = mp_fresh_chosen; m.fresh_plogp = mp_fresh_plogp; m.mask = mp_mask; m.next_ids = mp_next_ids;
        m.last = st.last; m.B = B; m.S = S; m.t = round; m.T = rounds - 1; m.bos_idx = cfg.bos_idx; m.pad_idx = cfg.pad_idx;
        m.seq_out = seq; m.plogp_out = opt.row_plogp; m.chosen_out = opt.row_chosen; m.round_out = opt.refine_round;
        return bofi::launch_mask_predict_step(m, s);
    };
    for (int round = 0; round < rounds; ++round) {
    // (round 0 under the row-block family: layer 0's q|k|v rows come out of the (label, position) table with the embedding launch -- BOFI_FILL_QKV_TAB=0: the projection)
    const bool qkv_tab = round == 0 && fill_tab_ready && !dec.empty() && fold_rb_ok(dec[0].qkv, M) && bofi::knob(BOFI_FILL_QKV_TAB) != 0 && !exp_skip("qkv");
    ENG_OK(bofi::launch_embed_fill(lut_tok, lut_syn, pe, st.ext_syn, round ? fed : nullptr, B, S, L, d, cfg.bos_idx, x_fill.x, x_fill.copy(), dt,
                                   x_fill.st, s, qkv_tab ? f_qkv0 : nullptr, qkv_tab ? qkv : nullptr, 3 * d));
    bool proj_made = qkv_tab;                            // this layer's q|k|v came out of the previous layer's feed-forward launch (layer 0: out of the table)
    for (size_t li = 0; li < dec.size(); ++li) {
        auto& l = dec[li];
        if (!proj_made) ENG_OK(project(x_fill, l.qkv, qkv, 0, 3 * d, M, s));
        bofi::AttnArgs a = self_attn_args(qkv, B, S);
        // syn_mask[i, :, :last-1] = True; strict mode reproduces the stale index of :1872-1873 (quirk Q1)
        a.klen = st.last; a.klen_sb = 1; a.klen_bias = -1;
        a.klen_shared_last = (flags & BOFI_FLAG_STRICT_Q1) ? (opt.q1_group > 0 ? opt.q1_group : B) : 0;
        const bool q_rb = fold_rb_ok(l.q_src, M);
        const bool ffn_rb = ffn_sublayer_ok(l.w1, l.w2, M);
        const bool need_copy_out = !(fold_rb_ok(l.qkv, M) && gen_rb);      // (a consumer of this layer's output reads the bf16 copy + statistics: a tiled GEMM)
        // (round 5's one-launch form of both attention sublayers, rb_dec_attn_kernel, lost 3 % in flight and left the library in round 6: dev/exp/rb_dec_attn_kernel.inc)
        // self-attention; the cross-attention's query projection rides its launch, or is a folded GEMM behind it
        bool q_made = false;
        ENG_OK(attn_sublayer(a, l.o, x_fill, !q_rb, false, s, &l.q_src, qs, d, &q_made));
        if (!q_made) ENG_OK(project(x_fill, l.q_src, qs, 0, d, M, s));
        const bofi::AttnArgs c = cross_attn_args(qs, n_len + (int)li, ctx, B, S, R, att_len);
        // split: the cross-attention's core now, its W_o + residual as the head of the feed-forward launch
        const bool cross_split = ffn_rb && !need_copy_out && attn_split_ok(c, l.o_src, l.w1, l.w2, 2);
        ENG_OK(attn_sublayer(c, l.o_src, x_fill, !ffn_rb, cross_split, s));
        // the word-to-region maps of this layer (the call's attention outputs), last pass only: from the queries and keys the sublayer above read, whatever its form --
        // qs stands until the next layer's query projection, and the kernels apply 1 / sqrt(d_k) themselves
        if (attn_out_set() && round + 1 == rounds && (int)li == (opt.attn_layer < 0 ? (int)dec.size() - 1 : opt.attn_layer)) {
            bofi::AttnMapsArgs m{};
            m.q = qs; m.ldq = d; m.k = kv_slot(n_len + (int)li); m.ldk = kv_all.N; m.dtype = dt; m.B = B; m.H = cfg.heads; m.Lq = S; m.Lk = R; m.scale = 0.125f;
            m.klen = att_len; m.qlen = st.last; m.qlen_bias = -1;
            m.mean = opt.attn_mean; m.heads = opt.attn_heads; m.K = opt.attn_topk; m.top_idx = opt.attn_top_idx; m.top_w = opt.attn_top_w;
            ENG_OK(bofi::launch_attn_maps(m, s));
        }
        // next consumer: the next layer's q|k|v (it may ride the feed-forward launch) or the generator
        const Lin* nxt = li + 1 < dec.size() ? &dec[li + 1].qkv : nullptr;
        ENG_OK(ffn_sublayer(l.w1, l.w2, x_fill, need_copy_out, M, s, cross_split ? &l.o_src : nullptr, nxt, qkv, 3 * d, &proj_made));
    }
    // ---- vocabulary projection (decoder.norm folded in), log-softmax, greedy pick, pad tail
    // generator.  V = 9 491 is not a whole number of 128-column tiles and its rows are not 16-byte aligned: the bf16 engine runs the GEMM
    // over the zero-padded weight rows into a buffer of pitch gen.Npad (persistent kernel, vector epilogue) and vocab_finalize reads
    // that, writing the log-probs at the caller's pitch V -- the same reads and writes as in place.
    if (fused) {
        if (exp_skip("gen")) continue;
        bofi::RbVocabArgs v{};
        v.x = x_fill.x; v.ldx = d; v.wp = (const bofi::u32x4*)gen.wp; v.c = gen.b; v.cs = gen.cs; v.M = M; v.N = gen.Npad; v.V = cfg.vocab; v.S = S;
        v.ntok = st.last; v.ntok_bias = -1; v.pad_idx = cfg.pad_idx; v.seq = ep_seq; v.row_plogp = ep_plogp; v.row_chosen = ep_chosen;
        v.part = vb_part; v.ctr = vb_ctr; v.alone = settings.in_flight == 1;
        ENG_OK(bofi::launch_rb_vocab(v, s));
        ENG_OK(refine_step(round));
        continue;
    }
    const float* lsrc = nullptr;
    if (gen_pad && logits_pad) {
        Lin gp = gen; gp.N = gen.Npad;                   // (the tiled form computes the zero columns too; the row-block kernel takes Npad anyway)
        ENG_OK(project(x_fill, gp, logits_pad, 1, gen.Npad, M, s));
        lsrc = logits_pad;
    } else {
        ENG_OK(folded(x_fill, gen, lg, BOFI_DT_F32, cfg.vocab, M, Rows{}, s));
    }
    // (a round that another one follows: its ids are all the next round reads -- the log-probs it would write are overwritten: not stored)
    const int ids_only_on = bofi::knob(BOFI_REFINE_IDS_ONLY);      // developer knob: 0 = every round stores its log-probs
    // (with the constrained pick on every round stores them: the pick reads what the pass stored)
    const int lsm = (flags & BOFI_FLAG_RAW_LOGITS) ? 0 : ((flags & BOFI_FLAG_IDS_ONLY) || (ids_only_on && round + 1 < rounds && lsrc && !pick_set(flags)) ? 2 : 1);
    ENG_OK(bofi::launch_vocab_finalize(lg, M, cfg.vocab, S, lsm, st.last, -1, cfg.pad_idx, ep_seq, s, nullptr, nullptr, nullptr, nullptr,
                                       lsrc, gen.Npad, lsm ? ep_plogp : nullptr, lsm ? ep_chosen : nullptr));
    // the constrained pick (bofi_call_opts_t.pick_*), every pass: banned ids and adjacent repeats re-picked from the tensor the epilogue has just written (log-probs, or the
    // logits at the caller's pitch), so a following round is fed the constrained ids and the last one leaves seq / row_chosen those of the emitted ids
    // BOFI_FLAG_PICK_TRIGRAMS: the K-candidate form (block_trigrams needs more than a row's two best ids), same point, same outputs
    if (flags & BOFI_FLAG_PICK_TRIGRAMS)
        ENG_OK(bofi::launch_vocab_pick(lg, cfg.vocab, M, cfg.vocab, S, st.last, -1, cfg.pad_idx, opt.pick_ban, opt.pick_no_repeat, 1, opt.pick_repeat_min_id, ep_seq,
                                       lsm ? ep_chosen : nullptr, pick_changed, pick_work, pick_work_bytes, s));
    else if (pick_set(flags))
        ENG_OK(bofi::launch_vocab_constrain(lg, cfg.vocab, M, cfg.vocab, S, st.last, -1, cfg.pad_idx, opt.pick_ban, opt.pick_no_repeat, opt.pick_repeat_min_id, ep_seq,
                                            lsm ? ep_chosen : nullptr, pick_changed, s));
    ENG_OK(refine_step(round));
    }
    return BOFI_OK;
}

// Semi-autoregressive decode (reference core_SAIC TransformerModel.py:1878-1986, greedy): per phrase one bounding step on
// the WORDS emitted so far, then a full decoder pass over all S positions whose new phrase is kept.
int bofi_engine::enqueue_decode_saic(const void* feats, int feats_dtype, const int* att_len, int B, int R, int flags, int64_t* seq,
                                     float* seq_logprob, int* phrase_num, int* phrase_length, int64_t* phrase_syn, int* bound_iters,
                                     hipStream_t s) {
    const int d = cfg.d_model, dt = cfg.dtype, S = cfg.seq_length, M = B * S;
    const int* halt = st.counters + 2;
    // iterations it_first .. it_last of the loop (opt.saic_it_begin / saic_it_end).  Every iteration past the last live one returns at once but still
    // costs its ~60 launches' dispatch; a caller that knows how long its captions run enqueues fewer and, when the count of live iterations
    // (bound_iters) says the loop may not be through, the REST in a second call: the loop's state lives in the workspace, so [1, c] then
    // [c + 1, S] is the same computation as [1, S]
    const int it_first = opt.saic_it_begin > 1 ? opt.saic_it_begin : 1, it_last = opt.saic_it_end > 0 && opt.saic_it_end < S ? opt.saic_it_end : S;
    if (it_first == 1) {
    ENG_OK(enqueue_encode(feats, feats_dtype, att_len, B, R, nullptr, s));
    ENG_OK(bofi::launch_saic_init(st, sa, B, L, cfg.pad_idx, cfg.bos_idx, cfg.len_idx, s));
    if (seq_logprob) ENG_OK(bofi::launch_zero_f32(seq_logprob, (size_t)M * cfg.vocab, s));   // seq_logprobs = zeros (:1883); not a memset node
    }
    const Rows halted{halt, 1};                    // every launch of an iteration returns at once when the loop has ended
    for (int it = it_first; it <= it_last; ++it) {
        // From the second iteration on only the rows of the phrases placed in this iteration go through the decoder's GEMMs and the
        // vocabulary epilogue (row list; launch_saic_rows): a placed row's input, key set and therefore its K / V in every layer
        // never change again, later rows are never attended, and only the new phrase's rows are copied out (:1968-1977).  The
        // first iteration runs every row: it is the only one in which a row without any key (an image that opened no phrase)
        // can raise the reference's "phrase nan!" return.
        const bool rowlist = saic_cache && it >= 2;
        const int* ri = rowlist ? sa_rows : nullptr;
        const int* rn = rowlist ? sa_nrows : nullptr;
        const Rows rows{halt, 1, ri, rn};
        // ---- bounding step on the words: K|V of all L rows, row-0 query attends keys < phrase_last
        ENG_OK(bofi::launch_embed_rows(lut_tok, nullptr, pe, sa.ext_len, nullptr, L, 0, B, L, d, cfg.bos_idx, xw.x, xw.copy(), dt, xw.st, halt, s));
        ENG_OK(folded(xw, b_kv_self, kvs, dt, 2 * d, B * L, halted, s));
        {
            bofi::AttnArgs a = attn_args(b_q0_sa, 0, kvs, 2 * d, bctx, B, 1, L, halted);
            a.klen = st.last; a.klen_sb = 1;
            ENG_OK(bofi::launch_attention(a, s));
        }
        ENG_OK(close_sublayer(bctx, b_o_self, y1, B, halted, s, b_x0_sa, 0));
        int w2parts = 0;
        ENG_OK(bound_chain(B, R, att_len, halted, s, &w2parts));
        ENG_OK(bound_tail(by3, w2parts, nullptr, nullptr, B, BOUND_HEADS | BOUND_UPDATE | BOUND_SAIC | BOUND_EARLY, nullptr, nullptr, s, true, it));
        if (flags & BOFI_FLAG_SAIC_LAYOUT_ONLY) {      // the caller draws this phrase's words itself (bofi_engine_saic_put_words before the next call): layout + positions only
            ENG_OK(bofi::launch_saic_halt(st, sa, B, L, it, s));
            continue;
        }
        // ---- decoder pass over all S positions (decode_SA :520-530) with the phrase-block mask as per-row key prefixes
        ENG_OK(bofi::launch_embed_rows(lut_tok, lut_syn, pe, sa.ext_phrase, st.ext_syn, L, 1, B, S, d, cfg.bos_idx, x_fill.x, x_fill.copy(), dt,
                                       x_fill.st, halt, s));
        if (rowlist) ENG_OK(bofi::launch_saic_rows(st, B, L, S, it, sa_rows, sa_nrows, s));
        // the row-list iterations in bf16 at the reference's width: a layer's six GEMMs as direct-operand row GEMMs (bound_ops.hip: no LDS
        // staging, ~5 us per launch whatever the few hundred rows), query projection + cross-attention as one launch; their row
        // statistics come in 16-column groups (st_fill16)
        const bool lean = rowlist && saic_lean && dt == BOFI_DT_BF16 && d == 512 && cfg.heads == 8 && R <= 64 && cfg.d_ff % 512 == 0;
        Stream fin = x_fill;                                           // what the generator reads: the lean launches leave statistics of their own
        if (lean) {
            const float* cst = x_fill.st; int cg = d / 32;               // statistics of the rows' current stream: where, and in how many groups
            auto rg = [&](const void* x, int ldx, const Lin& l, const float* stats, int groups, const float* residual, float* y, void* yb,
                          int ldyb, float* stats_out, int relu) {
                bofi::RowGemmArgs a{};
                a.x = (const uint16_t*)x; a.ldx = ldx; a.w = (const uint16_t*)l.w; a.bias = l.b; a.stats = stats; a.stats_groups = groups;
                a.colsum = stats ? l.cs : nullptr; a.residual = residual; a.ldr = d; a.y = y; a.ldy = d; a.yb = (uint16_t*)yb; a.ldyb = ldyb;
                a.stats_out = stats_out; a.M = M; a.N = l.N; a.K = l.K; a.splitk = 1; a.relu = relu; a.skip_if_ge = halt; a.skip_threshold = 1;
                a.row_idx = ri; a.m_dev = rn;
                return bofi::launch_rowgemm(a, s);
            };
            for (size_t li = 0; li < dec.size(); ++li) {
                auto& l = dec[li];
                void* qkv = qkv_dec[li];
                ENG_OK(rg(x_fill.xb, d, l.qkv, cst, cg, nullptr, nullptr, qkv, 3 * d, nullptr, 0));
                bofi::AttnArgs a = self_attn_args(qkv, B, S, halted);
                a.klen = sa.klen_dec + 1; a.klen_sb = L; a.klen_sq = 1; a.klen_bias = -1;      // (as in the tiled form below)
                ENG_OK(bofi::launch_attention(a, s));
                ENG_OK(rg(ctx, d, l.o, nullptr, 0, x_fill.x, x_fill.x, x_fill.xb, d, st_fill16, 0));
                cst = st_fill16; cg = d / 16;
                {   bofi::BoundQAttnArgs q{};
                    q.x = (const uint16_t*)x_fill.xb; q.stats = cst; q.stats_groups = cg; q.wq = (const uint16_t*)l.q_src.w; q.bias = l.q_src.b; q.colsum = l.q_src.cs;
                    q.k = (const uint16_t*)kv_slot(n_len + (int)li); q.v = q.k + d; q.ldkv = kv_all.N; q.att_len = att_len; q.out = (uint16_t*)ctx;
                    q.B = M; q.R = R; q.d = d; q.H = cfg.heads; q.skip_if_ge = halt; q.skip_threshold = 1;
                    q.row_idx = ri; q.n_rows = rn; q.rows_per_image = S;
                    ENG_OK(bofi::launch_bound_qattn(q, s)); }
                ENG_OK(rg(ctx, d, l.o_src, nullptr, 0, x_fill.x, x_fill.x, x_fill.xb, d, st_fill16, 0));
                ENG_OK(rg(x_fill.xb, d, l.w1, cst, cg, nullptr, nullptr, hdn, cfg.d_ff, nullptr, 1));
                ENG_OK(rg(hdn, cfg.d_ff, l.w2, nullptr, 0, x_fill.x, x_fill.x, x_fill.xb, d, st_fill16, 0));
            }
            fin.st = st_fill16; fin.groups = d / 16;
        } else {
            // phrase_mask[:, 1:-1, 1:-1] as key prefixes: row t <- row t+1, one key column dropped
            for (size_t li = 0; li < dec.size(); ++li)
                ENG_OK(decoder_layer_tiled(dec[li], n_len + (int)li, x_fill, qkv_dec[li], B, S, R, sa.klen_dec + 1, -1, att_len, rows, s));
        }
        ENG_OK(folded(fin, gen, logits, BOFI_DT_F32, cfg.vocab, M, rows, s));
        ENG_OK(bofi::launch_vocab_finalize(logits, M, cfg.vocab, S, (flags & BOFI_FLAG_RAW_LOGITS) ? 0 : 1, nullptr, 0, cfg.pad_idx, tok64, s,
                                           st.counters + 3, halt, ri, rn));
        if (flags & BOFI_FLAG_SAMPLE)          // sample_next_word 'sample' (CaptionModel.py:405-425): the drawn ids feed the next bound step
            ENG_OK(bofi::launch_vocab_sample(logits, M, cfg.vocab, S, 1, opt.sample_temperature, (uint64_t)it * 0x9E3779B97F4A7C15ull, nullptr,
                                             cfg.pad_idx, tok64, s, halt, ri, rn, d_seed));
        ENG_OK(bofi::launch_saic_copy(st, sa, tok64, logits, seq_logprob, B, L, S, cfg.vocab, it, s));
    }
    ENG_OK(bofi::launch_saic_export(st, sa, B, L, S, seq, phrase_num, phrase_length, phrase_syn, bound_iters, s));
    return BOFI_OK;
}

// Replays the captured launch sequence stored under `key`, capturing it first (through `enqueue`, on the engine's capture stream)
// when the key is new.  At most 16 captures are kept per engine (a pipeline over ragged loader batches holds two inputs x a few region buckets).
template <typename F>
static int run_graphed(bofi_engine* e, const std::vector<uintptr_t>& key, hipStream_t s, F enqueue) {
    for (auto& g : e->graphs)
        if (g.key == key) { ENG_HIP(hipGraphLaunch(g.exec, s)); return BOFI_OK; }
    GraphEntry g;
    g.key = key;
    // the capture stream is created lazily so that the run streams of an engine and its forks are
    // created back to back (they then land on different hardware queues)
    if (!e->cap_stream) ENG_HIP(hipStreamCreateWithFlags(&e->cap_stream, hipStreamNonBlocking));
    ENG_HIP(hipStreamBeginCapture(e->cap_stream, hipStreamCaptureModeThreadLocal));
    const int rc = enqueue(e->cap_stream);
    hipError_t ee = hipStreamEndCapture(e->cap_stream, &g.graph);
    if (rc != BOFI_OK) { if (g.graph) (void)hipGraphDestroy(g.graph); return rc; }
    if (ee != hipSuccess) return fail(BOFI_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(ee));
    ENG_HIP(hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0));
    if (e->graphs.size() >= 16) {                      // small cache: drop the oldest capture
        ENG_HIP(hipDeviceSynchronize());               // (a launch of it may still be in flight on any of the caller's streams: rare path, wait it out)
        (void)hipGraphExecDestroy(e->graphs.front().exec);
        (void)hipGraphDestroy(e->graphs.front().graph);
        e->graphs.erase(e->graphs.begin());
    }
    e->graphs.push_back(g);
    ENG_HIP(hipGraphLaunch(g.exec, s));
    return BOFI_OK;
}

// ================================================================================================
extern "C" {

int bofi_abi_version(void) { return 5; }
const char* bofi_last_error(void) { return g_err.c_str(); }

int bofi_engine_create(const bofi_config_t* c, bofi_engine_t** out) {
    if (!c || !out) return fail(BOFI_ERR_ARG, "null argument");
    if (c->dtype != BOFI_DT_F32 && c->dtype != BOFI_DT_BF16) return fail(BOFI_ERR_ARG, "dtype must be 0 (f32) or 1 (bf16)");
    if (c->heads <= 0 || c->d_model != c->heads * 64) return fail(BOFI_ERR_ARG, "d_model / heads must be 64");
    if (c->d_model % 128 || c->d_ff % 64 || c->feat % 64) return fail(BOFI_ERR_ARG, "d_model must be a multiple of 128, d_ff and feat of 64");
    if (c->seq_length <= 0 || c->seq_length + 2 > 64) return fail(BOFI_ERR_ARG, "seq_length must be in 1..62");
    if (c->max_batch <= 0 || c->max_regions <= 0 || c->max_regions > 128) return fail(BOFI_ERR_ARG, "max_batch > 0, 0 < max_regions <= 128");
    if (c->vocab <= 0 || c->n_enc < 0 || c->n_dec < 0 || c->head_hidden <= 0) return fail(BOFI_ERR_ARG, "bad layer/vocab counts");
    if (c->n_len < 1 || c->n_len > 8) return fail(BOFI_ERR_ARG, "n_len must be in 1..8");
    auto* e = new bofi_engine();
    e->cfg = *c;
    e->n_len = c->n_len;
    // the per-engine knobs: from the live environment, now (no reload needed), kept for the engine's life
    e->bound_dense = c->n_len > 1 || bofi::knob_live(BOFI_BOUND_DENSE).i != 0;
    { const bofi::KnobValue v = bofi::knob_live(BOFI_SAIC_CACHE); e->saic_cache = !v.set || v.i != 0; }     // 0: every row through the decoder in every iteration
    { const bofi::KnobValue v = bofi::knob_live(BOFI_SAIC_LEAN); e->saic_lean = !v.set || v.i != 0; }       // 0: the row-list iterations on the general GEMM / attention kernels
    e->L = c->seq_length + 2;
    e->tsz = c->dtype == BOFI_DT_F32 ? 4 : 2;
    *out = e;
    return BOFI_OK;
}

void bofi_engine_destroy(bofi_engine_t* e) {
    if (!e) return;
    for (auto& g : e->graphs) {
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
        if (g.graph) (void)hipGraphDestroy(g.graph);
    }
    if (e->cap_stream) (void)hipStreamDestroy(e->cap_stream);
    if (e->run_stream) (void)hipStreamDestroy(e->run_stream);
    for (void* p : e->allocs) (void)hipFree(p);
    if (!e->is_fork) { if (e->rt_dev) (void)hipFree(e->rt_dev); if (e->rt_pin) (void)hipHostFree(e->rt_pin); }
    delete e;
}

int bofi_engine_fork_sized(bofi_engine_t* parent, int max_batch, bofi_engine_t** out) { return bofi_engine_fork_ex(parent, max_batch, 0, out); }

int bofi_engine_fork_ex(bofi_engine_t* parent, int max_batch, int fork_flags, bofi_engine_t** out) {
    g_err.clear();
    if (!parent || !out) return fail(BOFI_ERR_ARG, "null argument");
    if (fork_flags & ~BOFI_FORK_IDS_ONLY) return fail(BOFI_ERR_ARG, "fork: unknown option");
    if (!parent->finalized) return fail(BOFI_ERR_STATE, "fork needs a finalized engine");
    if (max_batch < 0) return fail(BOFI_ERR_ARG, "fork: max_batch >= 0 (0 = the parent's)");
    auto* e = new bofi_engine(*parent);          // copies config and every weight pointer
    e->host.clear();
    e->allocs.clear();                           // owns nothing of the parent's
    e->graphs.clear();
    e->cap_stream = nullptr;
    e->run_stream = nullptr;
    e->is_fork = true;
    e->rt_dev = nullptr; e->rt_pin = nullptr; e->rt_bytes = 0; e->rt_cache.clear();
    e->dbg_part = nullptr;
    e->settings = parent->settings.forked();
    e->st = bofi::BoundState{};
    e->no_logits = (fork_flags & BOFI_FORK_IDS_ONLY) != 0;
    if (max_batch > 0) e->cfg.max_batch = max_batch;          // (the weights do not depend on it: only the workspace is sized by it)
    int rc = e->alloc_workspace();
    if (rc == BOFI_OK && hipStreamCreateWithFlags(&e->cap_stream, hipStreamNonBlocking) != hipSuccess) rc = fail(BOFI_ERR_HIP, "hipStreamCreate");
    if (rc != BOFI_OK) { bofi_engine_destroy(e); return rc; }
    *out = e;
    return BOFI_OK;
}

int bofi_engine_fork(bofi_engine_t* parent, bofi_engine_t** out) { return bofi_engine_fork_sized(parent, 0, out); }

int bofi_engine_refresh_device(bofi_engine_t* e, int n, const char* const* names, const float* const* ptrs, const int64_t* numels, void* stream) {
    if (!e || !names || !ptrs || !numels || n <= 0) return fail(BOFI_ERR_ARG, "null argument");
    g_err.clear();
    if (e->is_fork) return fail(BOFI_ERR_STATE, "refresh the parent engine (forks share its weights)");
    if (!e->finalized) return fail(BOFI_ERR_STATE, "engine not finalized: the first load goes through set_weight + finalize");
    DevParams src;
    for (int i = 0; i < n; ++i) src[names[i]] = {ptrs[i], numels[i]};
    ENG_OK(e->repack(src, (hipStream_t)stream));
    e->host.clear();                          // the host copies are stale now; a later finalize needs set_weight again
    return BOFI_OK;
}

// Developer aid: copy a workspace buffer of the bounding iteration, or a packed operand left by repack(), into user memory (device to device, on `stream`).
// The packed operands carry their size: *cap is set to it (left at -1 for the workspace buffers, whose extent depends on the last call).
static const void* debug_buffer(bofi_engine_t* e, const std::string& n, int64_t* cap) {
    const bofi_config_t& c = e->cfg;
    const int64_t d = c.d_model, hh = c.head_hidden, rows = (int64_t)e->L * 10, tsz = (int64_t)e->tsz;
    *cap = -1;
    const size_t at = n.find('@');
    if (at != std::string::npos) {          // "<field>@<first prefix of the recipe>[#k]": k-th (from 0) declared Linear / Norm that starts with this prefix
        const std::string field = n.substr(0, at);
        std::string prefix = n.substr(at + 1);
        int nth = 0;
        const size_t hash = prefix.rfind('#');
        if (hash != std::string::npos) {
            if (hash + 1 >= prefix.size() || prefix.find_first_not_of("0123456789", hash + 1) != std::string::npos || prefix.size() - hash > 6) return nullptr;
            nth = std::atoi(prefix.c_str() + hash + 1);
            prefix.resize(hash);
        }
        if (field == "g" || field == "nb") {
            for (const auto& r : e->norm_recipes)
                if (r.prefix == prefix && nth-- == 0) { *cap = (int64_t)r.d * 4; return field == "g" ? r.out->g : r.out->b; }
            return nullptr;
        }
        for (const auto& r : e->lin_recipes) {
            if (r.prefixes.empty() || r.prefixes[0] != prefix || nth-- != 0) continue;
            const Lin& l = *r.out;
            const int64_t np = l.Npad;
            if (field == "w") { *cap = np * l.K * tsz; return l.w; }
            if (field == "b") { *cap = np * 4; return l.b; }
            if (field == "cs") { *cap = np * 4; return l.cs; }
            if (field == "wp") { *cap = np * l.K * 2; return l.wp; }
            if (field == "wp16") { *cap = np * l.K * 2; return l.wp16; }
            return nullptr;
        }
        return nullptr;
    }
    struct Tab { const char* name; const void* p; int64_t bytes; };
    const Tab tabs[] = {
        {"xt", e->d_xt, rows * d * 4}, {"x0", e->b_x0, d * 4}, {"x0_sa", e->b_x0_sa, d * 4}, {"x0b", e->b_x0b, d * 4},
        {"kvtab", e->b_kvtab, rows * 2 * d * tsz}, {"q0", e->b_q0, d * tsz}, {"q0_sa", e->b_q0_sa, d * tsz},
        {"votab", e->b_votab, rows * c.heads * d * tsz}, {"w1p", e->b_w1p, d * 2 * hh * tsz}, {"w1t", e->heads.w1t, d * 2 * hh * 4}, {"b1", e->heads.b1, 2 * hh * 4},
        {"q0_32", e->b_q0_32, d * 4}, {"sctab", e->b_sctab, rows * c.heads * 4}, {"vtab", e->b_vtab, rows * d * 4}, {"wsat", e->b_wsat, 4},
        {"len_w2", e->heads.len_w2, 20 * hh * 4}, {"len_b2", e->heads.len_b2, 20 * 4}, {"syn_w2", e->heads.syn_w2, 10 * hh * 4}, {"syn_b2", e->heads.syn_b2, 10 * 4},
    };
    for (const Tab& t : tabs)
        if (n == t.name) { *cap = t.bytes; return t.p; }
    return n == "by1" ? (const void*)e->y1.x : n == "byb" ? (const void*)e->y1.xb : n == "st_b" ? (const void*)e->y1.st :
           n == "bq2" ? (const void*)e->bq2 : n == "bctx2" ? (const void*)e->bctx2 : n == "by2" ? (const void*)e->y2.x :
           n == "bh" ? (const void*)e->bh : n == "by3" ? (const void*)e->by3 : n == "dbg_part" ? (const void*)e->dbg_part :
           n == "counters" ? (const void*)e->st.counters :                // ("counters": int32 [8] of the last decode: [5] = groups whose bounding loop ran as a PAIR of workgroups)
           n == "kv" ? (const void*)e->kv : n == "x_enc" ? (const void*)e->x_enc.x : nullptr;      // ("kv": the stacked cross K|V rows [B*R][kv_all.N] of the last encode, compute dtype; "x_enc": the encoder's float32 output rows [B*R][d] they were projected from)
}

int bofi_engine_debug_copy(bofi_engine_t* e, const char* name, void* dst, int64_t bytes, void* stream) {
    if (!e || !name || !dst) return fail(BOFI_ERR_ARG, "null argument");
    int64_t cap = -1;
    const void* src = debug_buffer(e, name, &cap);
    if (!src) return fail(BOFI_ERR_ARG, "unknown buffer");      // (also: a field this Linear does not have, a table this configuration does not build)
    if (cap >= 0 && (bytes < 0 || bytes > cap)) return fail(BOFI_ERR_ARG, std::string(name) + " holds " + std::to_string(cap) + " bytes");
    ENG_HIP(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return BOFI_OK;
}

int bofi_engine_set_decodes_in_flight(bofi_engine_t* e, int n) {
    g_err.clear();
    if (!e || n < 0) return fail(BOFI_ERR_ARG, "decodes in flight: >= 0 (0 = unknown)");
    e->settings.in_flight = n;
    return BOFI_OK;
}

int bofi_engine_ids_only_fused(bofi_engine_t* e, int B) { return e && e->finalized && B > 0 && e->gen_rb_ok(B * e->cfg.seq_length) ? 1 : 0; }

int bofi_engine_bound_loop_active(bofi_engine_t* e, int R) { return e && e->finalized && e->bound_loop_ok(R) ? 1 : 0; }

int bofi_engine_set_bound_loop(bofi_engine_t* e, int mode) {
    g_err.clear();
    if (!e || (mode != -1 && mode != 0 && mode != 2)) return fail(BOFI_ERR_ARG, "bound loop mode: -1 (environment / hint), 0 (five-launch iterations) or 2 (persistent loop kernel)");
    e->settings.loop_mode = mode;
    return BOFI_OK;
}

int bofi_engine_set_bound_kv_beside(bofi_engine_t* e, int mode) {
    g_err.clear();
    if (!e || (mode != 0 && mode != 1)) return fail(BOFI_ERR_ARG, "cross K|V beside the bounding loop: 0 (never) or 1 (where the loops are exposed)");
    e->settings.kv_beside = mode;
    return BOFI_OK;
}

int bofi_engine_bound_kv_beside_active(bofi_engine_t* e, int B, int R, int flags) {
    return e && e->finalized && B > 0 && R > 0 && e->bound_kv_beside_ok(B, R, flags & (BOFI_FLAG_PHASE_ENCODE | BOFI_FLAG_PHASE_BOUND | BOFI_FLAG_PHASE_FILL)) ? 1 : 0;
}

int bofi_engine_saic_put_words(bofi_engine_t* e, const int64_t* seq, int B, void* stream) {
    g_err.clear();
    if (!e || !seq) return fail(BOFI_ERR_ARG, "null argument");
    if (B < 1 || B > e->cfg.max_batch || B != e->saic_B) return fail(BOFI_ERR_ARG, "saic_put_words: B must be the batch of the decode it continues");
    return bofi::launch_saic_put_words(e->st, e->sa, seq, B, e->L, e->cfg.seq_length, (hipStream_t)stream);
}

const float* bofi_engine_logprob(bofi_engine_t* e) {
    return e ? e->logits : nullptr;
}

int bofi_engine_pick_changed(bofi_engine_t* e, int* dst, int B, void* stream) {
    g_err.clear();
    if (!e || !dst || B < 1 || B > e->cfg.max_batch) return fail(BOFI_ERR_ARG, "pick_changed: an engine, a destination and B in 1..max_batch");
    ENG_HIP(hipMemcpyAsync(dst, e->pick_changed, (size_t)B * sizeof(int), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return BOFI_OK;
}

void* bofi_engine_stream(bofi_engine_t* e) {
    if (!e) return nullptr;
    if (!e->run_stream && hipStreamCreateWithFlags(&e->run_stream, hipStreamNonBlocking) != hipSuccess) return nullptr;
    return (void*)e->run_stream;
}

int bofi_engine_set_weight(bofi_engine_t* e, const char* name, const float* data, int64_t numel) {
    if (!e || !name || !data || numel < 0) return fail(BOFI_ERR_ARG, "null argument");
    if (e->is_fork) return fail(BOFI_ERR_STATE, "weights belong to the parent engine");
    e->host[name].assign(data, data + numel);
    e->finalized = false;
    return BOFI_OK;
}

int bofi_engine_finalize(bofi_engine_t* e) {
    if (!e) return fail(BOFI_ERR_ARG, "null engine");
    g_err.clear();
    if (e->is_fork) return fail(BOFI_ERR_STATE, "finalize the parent engine, then fork again");
    const bofi_config_t& c = e->cfg;
    const int d = c.d_model, dff = c.d_ff, L = e->L, hh = c.head_hidden;
    // drop everything from a previous finalize (weights may have changed)
    for (auto& g : e->graphs) { if (g.exec) (void)hipGraphExecDestroy(g.exec); if (g.graph) (void)hipGraphDestroy(g.graph); }
    e->graphs.clear();
    ENG_HIP(hipDeviceSynchronize());
    for (void* p : e->allocs) (void)hipFree(p);
    e->allocs.clear();
    e->enc.assign(c.n_enc, EncLayer());
    e->dec.assign(c.n_dec, DecLayer());
    e->lin_recipes.clear();
    e->norm_recipes.clear();

    auto S = [](const char* fmt, int a, int b = 0) { char buf[256]; std::snprintf(buf, sizeof buf, fmt, a, b); return std::string(buf); };
    ENG_OK(e->make_lin(&e->att_embed, {"att_embed.0"}, d, c.feat));
    for (int l = 0; l < c.n_enc; ++l) {
        auto& E = e->enc[l];
        const std::string p = S("model.encoder.layers.%d", l);
        ENG_OK(e->make_lin(&E.qkv, {p + ".self_attn.linears.0", p + ".self_attn.linears.1", p + ".self_attn.linears.2"}, d, d, p + ".sublayer.0.norm", 0, true));
        ENG_OK(e->make_lin(&E.o, {p + ".self_attn.linears.3"}, d, d, "", 0, true));
        ENG_OK(e->make_lin(&E.w1, {p + ".feed_forward.w_1"}, dff, d, p + ".sublayer.1.norm", 0, true));
        ENG_OK(e->make_lin(&E.w2, {p + ".feed_forward.w_2"}, d, dff, "", 0, true));
        ENG_OK(e->make_norm(&E.n0, p + ".sublayer.0.norm", d));
        ENG_OK(e->make_norm(&E.n1, p + ".sublayer.1.norm", d));
    }
    ENG_OK(e->make_norm(&e->enc_norm, "model.encoder.norm", d));
    const std::string bl = "model.length_predictor.LengthPredictor.0";
    std::vector<std::string> kvs;                 // cross-attention K|V: the bound layers first, then the decoder layers
    for (int l = 0; l < e->n_len; ++l) {
        const std::string p = S("model.length_predictor.LengthPredictor.%d", l);
        kvs.push_back(p + ".src_attn.linears.1");
        kvs.push_back(p + ".src_attn.linears.2");
    }
    e->blay.assign(e->bound_dense ? e->n_len : 0, DecLayer());
    for (size_t l = 0; l < e->blay.size(); ++l) {
        auto& D = e->blay[l];
        const std::string p = S("model.length_predictor.LengthPredictor.%d", (int)l);
        ENG_OK(e->make_lin(&D.qkv, {p + ".self_attn.linears.0", p + ".self_attn.linears.1", p + ".self_attn.linears.2"}, d, d, p + ".sublayer.0.norm"));
        ENG_OK(e->make_lin(&D.o, {p + ".self_attn.linears.3"}, d, d));
        ENG_OK(e->make_lin(&D.q_src, {p + ".src_attn.linears.0"}, d, d, p + ".sublayer.1.norm"));
        ENG_OK(e->make_lin(&D.o_src, {p + ".src_attn.linears.3"}, d, d));
        ENG_OK(e->make_lin(&D.w1, {p + ".ff.w_1"}, dff, d, p + ".sublayer.2.norm"));
        ENG_OK(e->make_lin(&D.w2, {p + ".ff.w_2"}, d, dff));
    }
    for (int l = 0; l < c.n_dec; ++l) {
        auto& D = e->dec[l];
        const std::string p = S("model.decoder.layers.%d", l);
        ENG_OK(e->make_lin(&D.qkv, {p + ".self_attn.linears.0", p + ".self_attn.linears.1", p + ".self_attn.linears.2"}, d, d, p + ".sublayer.0.norm", 0, true));
        ENG_OK(e->make_lin(&D.o, {p + ".self_attn.linears.3"}, d, d, "", 0, true));
        ENG_OK(e->make_lin(&D.q_src, {p + ".src_attn.linears.0"}, d, d, p + ".sublayer.1.norm", 0, true));
        ENG_OK(e->make_lin(&D.o_src, {p + ".src_attn.linears.3"}, d, d, "", 0, true));
        ENG_OK(e->make_lin(&D.w1, {p + ".feed_forward.w_1"}, dff, d, p + ".sublayer.2.norm", 0, true));
        ENG_OK(e->make_lin(&D.w2, {p + ".feed_forward.w_2"}, d, dff, "", 0, true));
        ENG_OK(e->make_norm(&D.n0, p + ".sublayer.0.norm", d));
        ENG_OK(e->make_norm(&D.n1, p + ".sublayer.1.norm", d));
        ENG_OK(e->make_norm(&D.n2, p + ".sublayer.2.norm", d));
        kvs.push_back(p + ".src_attn.linears.1");
        kvs.push_back(p + ".src_attn.linears.2");
    }
    ENG_OK(e->make_norm(&e->dec_norm, "model.decoder.norm", d));
    ENG_OK(e->make_lin(&e->kv_all, kvs, d, d, "model.encoder.norm", 0, true));
    ENG_OK(e->make_lin(&e->gen, {"model.generator.proj"}, c.vocab, d, "model.decoder.norm", 128, true));      // padded to whole 128-column tiles (the persistent GEMM)
    {
        const auto* ls = e->get("model.syn_embed.lut.weight", (size_t)10 * d);
        const auto* lt = e->get("model.tgt_embed.lut.weight", (size_t)c.vocab * d);
        auto it = e->host.find("model.pos_embed.pe");
        if (!ls || !lt) return BOFI_ERR_STATE;
        if (it == e->host.end() || it->second.size() < (size_t)L * d) return fail(BOFI_ERR_STATE, "missing weight model.pos_embed.pe");
        ENG_OK(e->dalloc(&e->lut_syn, ls->size()));
        ENG_OK(e->dalloc(&e->lut_tok, lt->size()));
        std::vector<float> pe(it->second.begin(), it->second.begin() + (size_t)L * d);      // a buffer, not a parameter: no repack carries it
        ENG_OK(e->upload_f32(&e->pe, pe));
    }
    // bound layer
    ENG_OK(e->make_lin(&e->b_o_self, {bl + ".self_attn.linears.3"}, d, d));
    ENG_OK(e->make_lin(&e->b_q_src, {bl + ".src_attn.linears.0"}, d, d, bl + ".sublayer.1.norm"));
    ENG_OK(e->make_lin(&e->b_o_src, {bl + ".src_attn.linears.3"}, d, d));
    ENG_OK(e->make_lin(&e->b_w1, {bl + ".ff.w_1"}, dff, d, bl + ".sublayer.2.norm"));
    ENG_OK(e->make_lin(&e->b_w2, {bl + ".ff.w_2"}, d, dff));
    ENG_OK(e->make_norm(&e->b_n0, bl + ".sublayer.0.norm", d));
    ENG_OK(e->make_norm(&e->b_n1, bl + ".sublayer.1.norm", d));
    ENG_OK(e->make_norm(&e->b_n2, bl + ".sublayer.2.norm", d));
    {
        const std::string lp = "model.length_predictor";
        Norm& nf = e->head_norm;
        ENG_OK(e->make_norm(&nf, lp + ".norm", d));
        if (!e->get(lp + ".Length_classifier1.weight", (size_t)hh * d) || !e->get(lp + ".Length_classifier1.bias", hh) ||
            !e->get(lp + ".Syntactic_classifier1.weight", (size_t)hh * d) || !e->get(lp + ".Syntactic_classifier1.bias", hh) ||
            !e->get(lp + ".Length_classifier2.weight", (size_t)20 * hh) || !e->get(lp + ".Length_classifier2.bias", 20) ||
            !e->get(lp + ".Syntactic_classifier2.weight", (size_t)10 * hh) || !e->get(lp + ".Syntactic_classifier2.bias", 10))
            return BOFI_ERR_STATE;
        float *p_w1, *p_b1, *p_lw2, *p_lb2, *p_sw2, *p_sb2;          // first layers of both heads transposed side by side [d][2*hh], their biases concatenated
        ENG_OK(e->dalloc(&p_w1, (size_t)d * 2 * hh)); ENG_OK(e->dalloc(&p_b1, (size_t)2 * hh));
        ENG_OK(e->dalloc(&p_lw2, (size_t)20 * hh)); ENG_OK(e->dalloc(&p_lb2, 20));
        ENG_OK(e->dalloc(&p_sw2, (size_t)10 * hh)); ENG_OK(e->dalloc(&p_sb2, 10));
        ENG_OK(e->dalloc((char**)&e->b_w1p, (size_t)d * 2 * hh, e->tsz));
        e->heads = bofi::BoundHeadWeights{nf.g, nf.b, p_w1, p_b1, p_lw2, p_lb2, p_sw2, p_sb2, e->b_w1p};
        e->loop_ready = false;
        if (e->loop_config_ok()) {      // the persistent loop kernel's operands (filled by derive_bound_f16)
            ENG_OK(e->make_lin(&e->b_heads, {lp + ".Length_classifier1", lp + ".Syntactic_classifier1"}, hh, d, lp + ".norm", 256));
            for (Lin* l : {&e->b_o_self, &e->b_q_src, &e->b_o_src, &e->b_w1, &e->b_w2, &e->b_heads}) ENG_OK(e->dalloc((char**)&l->wp16, (size_t)l->Npad * l->K, 2));
            ENG_OK(e->dalloc(&e->b_q0_32, (size_t)d)); ENG_OK(e->dalloc(&e->b_sctab, (size_t)L * 10 * c.heads)); ENG_OK(e->dalloc(&e->b_vtab, (size_t)L * 10 * d));
            ENG_OK(e->dalloc(&e->b_wsat, 4));
        }
        if (e->rb_ok()) {               // the filling pass's layer-0 q|k|v by (label, position) (derive_fill_table)
            ENG_OK(e->dalloc((char**)&e->f_qkv0, (size_t)10 * c.seq_length * 3 * d, e->tsz));
            ENG_OK(e->dalloc(&e->f_x0, (size_t)10 * c.seq_length * d));
            ENG_OK(e->dalloc((char**)&e->f_syn, (size_t)10 * L, sizeof(int)));
            std::vector<int> pat((size_t)10 * L);
            for (int b = 0; b < 10; ++b) for (int t = 0; t < L; ++t) pat[(size_t)b * L + t] = b;
            ENG_HIP(hipMemcpy(e->f_syn, pat.data(), pat.size() * sizeof(int), hipMemcpyHostToDevice));
        }
    }

    e->n_weight_allocs = e->allocs.size();      // everything allocated so far is weights (shared with forks)
    ENG_OK(e->alloc_workspace());

    // operands and outputs of the bound layer's input-independent tables (repack)
    ENG_OK(e->dalloc(&e->d_xt, (size_t)L * 10 * d));
    ENG_OK(e->dalloc(&e->b_x0, (size_t)d));
    ENG_OK(e->make_lin(&e->t_kvself, {bl + ".self_attn.linears.1", bl + ".self_attn.linears.2"}, d, d));
    ENG_OK(e->make_lin(&e->t_qself, {bl + ".self_attn.linears.0"}, d, d));
    ENG_OK(e->dalloc((char**)&e->b_kvtab, (size_t)L * 10 * 2 * d, e->tsz));
    ENG_OK(e->dalloc((char**)&e->b_q0, (size_t)d, e->tsz));
    ENG_OK(e->dalloc(&e->b_x0_sa, (size_t)d));
    ENG_OK(e->dalloc((char**)&e->b_q0_sa, (size_t)d, e->tsz));
    ENG_OK(e->make_lin(&e->b_kv_self, {bl + ".self_attn.linears.1", bl + ".self_attn.linears.2"}, d, d, bl + ".sublayer.0.norm"));
    ENG_OK(e->dalloc((char**)&e->b_votab, (size_t)L * 10 * c.heads * d, e->tsz));
    ENG_OK(e->dalloc(&e->b_x0b, (size_t)d));

    // Stage the float32 parameters of the host map in one temporary arena on the device (never in e->allocs) and pack from there: the same
    // kernels on the same values as a refresh_device with these weights
    DevParams src;
    size_t bytes = 256;
    for (const auto& kv : e->host) bytes += (kv.second.size() * 4 + 255) & ~(size_t)255;
    char* arena = nullptr;
    ENG_HIP(hipMalloc((void**)&arena, bytes));
    int rc = BOFI_OK;
    size_t off = 0;
    for (const auto& kv : e->host) {
        const size_t nb = kv.second.size() * 4;
        if (rc == BOFI_OK && nb && hipMemcpy(arena + off, kv.second.data(), nb, hipMemcpyHostToDevice) != hipSuccess) rc = fail(BOFI_ERR_HIP, "hipMemcpy: staging " + kv.first);
        src[kv.first] = {(const float*)(arena + off), (int64_t)kv.second.size()};
        off += (nb + 255) & ~(size_t)255;
    }
    if (rc == BOFI_OK) rc = e->repack(src, nullptr);
    const hipError_t done = hipDeviceSynchronize();
    (void)hipFree(arena);
    e->rt_cache.clear();        // the descriptor table names the arena: no later refresh_device may take it for its own
    if (rc != BOFI_OK) return rc;
    if (done != hipSuccess) return fail(BOFI_ERR_HIP, std::string("hipDeviceSynchronize: ") + hipGetErrorString(done));
    // NB: hardware-queue assignment follows stream creation order; the capture stream is created here (and in
    // fork) because that order measured best with 4 decodes in flight on torch's pooled streams
    if (!e->cap_stream) ENG_HIP(hipStreamCreateWithFlags(&e->cap_stream, hipStreamNonBlocking));
    e->finalized = true;
    return BOFI_OK;
}

// Every entry point that enqueues begins here: the call's options (NULL: the defaults, which a zero-filled record states too) replace the previous call's
static int check_call(bofi_engine_t* e, int B, int R, const bofi_call_opts_t* opts = nullptr) {
    if (!e) return fail(BOFI_ERR_ARG, "null engine");
    e->opt = opts ? *opts : bofi_call_opts_t{};
    if (!e->finalized) return fail(BOFI_ERR_STATE, "engine not finalized");
    if (B <= 0 || B > e->cfg.max_batch) return fail(BOFI_ERR_ARG, "batch outside 1..max_batch");
    if (R <= 0 || R > e->cfg.max_regions) return fail(BOFI_ERR_ARG, "regions outside 1..max_regions");
    return BOFI_OK;
}
static int check_ids_only(bofi_engine_t* e, int flags, const float* seq_logprob) {
    if ((flags & BOFI_FLAG_IDS_ONLY) && seq_logprob) return fail(BOFI_ERR_ARG, "BOFI_FLAG_IDS_ONLY: seq_logprob must be NULL");
    if ((flags & BOFI_FLAG_IDS_ONLY) && (flags & BOFI_FLAG_RAW_LOGITS)) return fail(BOFI_ERR_ARG, "BOFI_FLAG_IDS_ONLY excludes BOFI_FLAG_RAW_LOGITS");
    if (e->no_logits && !(flags & BOFI_FLAG_IDS_ONLY)) return fail(BOFI_ERR_STATE, "this fork has no vocabulary-wide buffers: decode with BOFI_FLAG_IDS_ONLY");
    return BOFI_OK;
}
// BOFI_FLAG_MASK_PREDICT: what the flag goes with, checked before anything is enqueued or captured
static int check_mask_predict(bofi_engine_t* e, int flags) {
    if (!(flags & BOFI_FLAG_MASK_PREDICT)) return BOFI_OK;
    if (((flags >> BOFI_FLAG_REFINE_SHIFT) & 15) == 0) return fail(BOFI_ERR_ARG, "BOFI_FLAG_MASK_PREDICT needs a refinement count >= 1 in bits 8..11");
    if (flags & BOFI_FLAG_RAW_LOGITS) return fail(BOFI_ERR_ARG, "BOFI_FLAG_MASK_PREDICT ranks log-probs: not with BOFI_FLAG_RAW_LOGITS");
    if (flags & BOFI_FLAG_SAMPLE) return fail(BOFI_ERR_ARG, "BOFI_FLAG_MASK_PREDICT refines greedy picks: not with BOFI_FLAG_SAMPLE");
    if (e->cfg.seq_length > 64) return fail(BOFI_ERR_ARG, "BOFI_FLAG_MASK_PREDICT: seq_length above 64 (one wavefront holds an image's positions)");
    return BOFI_OK;
}
// Every rule on a call's options (bofi_call_opts_t), checked before anything is enqueued or captured
enum { CALL_NAIC, CALL_SAIC, CALL_FILL };
static int check_opts(bofi_engine_t* e, int flags, const bofi_call_opts_t& o, int which_call, int R) {
    if (o.q1_group < 0) return fail(BOFI_ERR_ARG, "group must be >= 0");
    if (o.bound_iter_cap < 0) return fail(BOFI_ERR_ARG, "bound iteration cap: >= 0 (0 = seq_length)");
    if (which_call == CALL_SAIC && (o.saic_it_begin < 0 || o.saic_it_begin > e->cfg.seq_length || o.saic_it_end < 0 || (o.saic_it_end > 0 && o.saic_it_end < o.saic_it_begin)))
        return fail(BOFI_ERR_ARG, "saic range: 1 <= begin <= end <= seq_length, or end 0");
    if (which_call == CALL_SAIC && (flags & BOFI_FLAG_SAMPLE) && !(o.sample_temperature > 0.f)) return fail(BOFI_ERR_ARG, "temperature must be positive");
    if (!o.row_plogp != !o.row_chosen) return fail(BOFI_ERR_ARG, "row statistics: both buffers or none");
    // the constrained pick
    if (o.pick_no_repeat != 0 && o.pick_no_repeat != 1) return fail(BOFI_ERR_ARG, "constrained pick: pick_no_repeat is 0 or 1");
    if (o.pick_repeat_min_id < 0) return fail(BOFI_ERR_ARG, "constrained pick: pick_repeat_min_id >= 0");
    if (o.pick_ban || o.pick_no_repeat || (flags & BOFI_FLAG_PICK_TRIGRAMS)) {
        if (which_call == CALL_SAIC) return fail(BOFI_ERR_STATE, "a constrained pick is set: it re-picks the non-autoregressive filling pass only, not the semi-autoregressive decode");
        if (flags & BOFI_FLAG_IDS_ONLY) return fail(BOFI_ERR_ARG, "constrained pick: not with BOFI_FLAG_IDS_ONLY (no distribution to re-pick from)");
        if (flags & BOFI_FLAG_MASK_PREDICT) return fail(BOFI_ERR_ARG, "constrained pick: not with BOFI_FLAG_MASK_PREDICT (a kept position would pin both neighbours)");
        if (e->cfg.seq_length > 64) return fail(BOFI_ERR_ARG, "constrained pick: seq_length <= 64 (bofi_vocab_constrain)");
    }
    if (!o.attn_mean && !o.attn_heads && !o.attn_top_idx && !o.attn_top_w) return BOFI_OK;      // no attention output: layer and K are not read
    if (which_call == CALL_SAIC) return fail(BOFI_ERR_STATE, "an attention output is set: the maps come out of the non-autoregressive filling pass only, not the semi-autoregressive decode");
    if (o.attn_layer < -1 || o.attn_layer >= e->cfg.n_dec) return fail(BOFI_ERR_ARG, "attention output: layer in 0 .. N_dec - 1, or -1 for the last");
    if (o.attn_topk < 0 || o.attn_topk > 8) return fail(BOFI_ERR_ARG, "attention output: K in 0..8");
    if (!o.attn_top_idx != !o.attn_top_w) return fail(BOFI_ERR_ARG, "attention output: top_idx and top_w, both or neither");
    if ((o.attn_topk > 0) != (o.attn_top_idx != nullptr)) return fail(BOFI_ERR_ARG, "attention output: K > 0 goes with top_idx and top_w, K = 0 with neither");
    // the map kernel's limits
    if (e->cfg.seq_length > 64 || R > 128) return fail(BOFI_ERR_ARG, "attention output: seq_length <= 64 and at most 128 regions (bofi_attn_maps)");
    if (e->cfg.d_model != e->cfg.heads * 64) return fail(BOFI_ERR_ARG, "attention output: head dim 64");
    return BOFI_OK;
}
// What a captured launch sequence bakes in beside the entry point's own arguments: the call's options, the engine's settings and the environment's generation
static void key_call(std::vector<uintptr_t>& key, const bofi_engine_t* e) {
    const bofi_call_opts_t& o = e->opt;
    uint32_t tbits; std::memcpy(&tbits, &o.sample_temperature, 4);
    // (sample_seed is deliberately unkeyed: the capture reads it from d_seed, written outside the graph at every call)
    for (uintptr_t v : {(uintptr_t)o.q1_group, (uintptr_t)o.bound_iter_cap, (uintptr_t)o.saic_it_begin, (uintptr_t)o.saic_it_end, (uintptr_t)tbits, (uintptr_t)o.live_max,
                        (uintptr_t)o.sat_out, (uintptr_t)o.row_plogp, (uintptr_t)o.row_chosen, (uintptr_t)o.refine_round, (uintptr_t)o.attn_layer, (uintptr_t)o.attn_topk,
                        (uintptr_t)o.attn_mean, (uintptr_t)o.attn_heads, (uintptr_t)o.attn_top_idx, (uintptr_t)o.attn_top_w,
                        (uintptr_t)o.pick_ban, (uintptr_t)o.pick_no_repeat, (uintptr_t)o.pick_repeat_min_id,
                        (uintptr_t)e->settings.in_flight, (uintptr_t)(e->settings.loop_mode + 1), (uintptr_t)e->settings.kv_beside, (uintptr_t)bofi::g_env_generation})
        key.push_back(v);
}
// a new field of the record goes into key_call, or is named there as deliberately unkeyed
static_assert(sizeof(bofi_call_opts_t) == 128, "bofi_call_opts_t changed: key_call must name every field");
static int check_feats(bofi_engine_t* e, const void* feats, int feats_dtype) {
    if (!feats) return fail(BOFI_ERR_ARG, "null att_feats");
    if (feats_dtype != BOFI_DT_F32 && feats_dtype != e->cfg.dtype) return fail(BOFI_ERR_ARG, "att_feats must be float32 or the engine's compute dtype");
    return BOFI_OK;
}

int bofi_engine_encode(bofi_engine_t* e, const void* feats, int feats_dtype, const int* att_len, int B, int R,
                       float* memory_out, void* stream) {
    g_err.clear();
    ENG_OK(check_call(e, B, R));
    ENG_OK(check_feats(e, feats, feats_dtype));
    return e->enqueue_encode(feats, feats_dtype, att_len, B, R, memory_out, (hipStream_t)stream);
}

int bofi_engine_bound_step(bofi_engine_t* e, const int* ext_syn, const int* last, int B, int R, const int* att_len,
                           float* len_logp, float* syn_logp, void* stream) {
    g_err.clear();
    ENG_OK(check_call(e, B, R));
    if (!ext_syn || !last || !len_logp || !syn_logp) return fail(BOFI_ERR_ARG, "null argument");
    if (e->bound_dense) return fail(BOFI_ERR_STATE, "bound_step is the incremental (N_len = 1) form's stage; the dense bounding pass runs inside decode_naic");
    if (e->bound_loop_ok(R)) return e->bound_loop(B, R, att_len, ext_syn, last, 0, len_logp, syn_logp, (hipStream_t)stream);
    ENG_OK(e->bound_tail(nullptr, 1, ext_syn, last, B, BOUND_ATTN, nullptr, nullptr, (hipStream_t)stream));
    return e->enqueue_bound_iter(B, R, att_len, ext_syn, last, 0, len_logp, syn_logp, false, (hipStream_t)stream);
}

int bofi_engine_fill_naic(bofi_engine_t* e, const int* ext_syn, const int* last, int B, int R, const int* att_len, int flags,
                          int64_t* seq, float* seq_logprob, const bofi_call_opts_t* opts, void* stream) {
    g_err.clear();
    ENG_OK(check_call(e, B, R, opts));
    if (!ext_syn || !last || !seq) return fail(BOFI_ERR_ARG, "null argument");
    ENG_OK(check_ids_only(e, flags, seq_logprob));
    if (const int rc = check_mask_predict(e, flags)) return rc;      // (its message stays: ENG_OK would put the call's text in its place)
    if (const int rc = check_opts(e, flags, e->opt, CALL_FILL, R)) return rc;
    if (e->no_logits && !e->gen_rb_ok(B * e->cfg.seq_length)) return fail(BOFI_ERR_STATE, "this fork has no vocabulary-wide buffers and the launch would not take the fused generator");
    hipStream_t s = (hipStream_t)stream;
    ENG_HIP(hipMemcpyAsync(e->st.ext_syn, ext_syn, (size_t)B * e->L * sizeof(int), hipMemcpyDeviceToDevice, s));
    ENG_HIP(hipMemcpyAsync(e->st.last, last, (size_t)B * sizeof(int), hipMemcpyDeviceToDevice, s));
    return e->enqueue_fill(att_len, B, R, flags & ~BOFI_FLAG_GRAPH, seq, seq_logprob, s);
}

int bofi_engine_decode_saic(bofi_engine_t* e, const void* feats, int feats_dtype, const int* att_len, int B, int R, int flags,
                            int64_t* seq, float* seq_logprob, int* phrase_num, int* phrase_length, int64_t* phrase_syn,
                            int* bound_iters, const bofi_call_opts_t* opts, void* stream) {
    g_err.clear();
    ENG_OK(check_call(e, B, R, opts));
    ENG_OK(check_feats(e, feats, feats_dtype));
    if (!seq) return fail(BOFI_ERR_ARG, "null seq");
    if (flags & BOFI_FLAG_MASK_PREDICT) return fail(BOFI_ERR_ARG, "BOFI_FLAG_MASK_PREDICT refines the non-autoregressive filling pass: not with the semi-autoregressive decode");
    if (const int rc = check_opts(e, flags, e->opt, CALL_SAIC, R)) return rc;
    if (e->n_len != 1) return fail(BOFI_ERR_STATE, "the semi-autoregressive decode is built for a one-layer bounding network (N_len = 1)");
    if (e->no_logits) return fail(BOFI_ERR_STATE, "this fork has no vocabulary-wide buffers: the semi-autoregressive decode needs the distribution");
    hipStream_t s = (hipStream_t)stream;
    e->saic_B = B;
    for (auto& q : e->qkv_dec)                              // the per-layer q|k|v buffers of this mode (never inside a capture)
        if (!q) ENG_OK(e->dalloc((char**)&q, (size_t)e->cfg.max_batch * e->cfg.seq_length * 3 * e->cfg.d_model, e->tsz));
    if (flags & BOFI_FLAG_SAMPLE) ENG_OK(bofi::launch_set_u64(e->d_seed, e->opt.sample_seed, s));     // outside the graph: fresh draws per call
    if (!(flags & BOFI_FLAG_GRAPH))
        return e->enqueue_decode_saic(feats, feats_dtype, att_len, B, R, flags, seq, seq_logprob, phrase_num, phrase_length, phrase_syn,
                                      bound_iters, s);
    std::vector<uintptr_t> key = {(uintptr_t)1, (uintptr_t)feats, (uintptr_t)feats_dtype, (uintptr_t)att_len, (uintptr_t)B, (uintptr_t)R,
                                  (uintptr_t)flags, (uintptr_t)seq, (uintptr_t)seq_logprob, (uintptr_t)phrase_num,
                                  (uintptr_t)phrase_length, (uintptr_t)phrase_syn, (uintptr_t)bound_iters};
    key_call(key, e);
    return run_graphed(e, key, s, [&](hipStream_t cs) {
        return e->enqueue_decode_saic(feats, feats_dtype, att_len, B, R, flags, seq, seq_logprob, phrase_num, phrase_length, phrase_syn,
                                      bound_iters, cs);
    });
}

int bofi_engine_decode_naic(bofi_engine_t* e, const void* feats, int feats_dtype, const int* att_len, int B, int R, int flags,
                            int64_t* seq, float* seq_logprob, int* phrase_num, int* phrase_length, int64_t* phrase_syn,
                            float* memory_out, int* bound_iters, const bofi_call_opts_t* opts, void* stream) {
    g_err.clear();
    ENG_OK(check_call(e, B, R, opts));
    ENG_OK(check_feats(e, feats, feats_dtype));
    if (!seq) return fail(BOFI_ERR_ARG, "null seq");
    ENG_OK(check_ids_only(e, flags, seq_logprob));
    if (const int rc = check_mask_predict(e, flags)) return rc;      // (its message stays: ENG_OK would put the call's text in its place)
    if (const int rc = check_opts(e, flags, e->opt, CALL_NAIC, R)) return rc;
    // (before anything is enqueued or captured: such a fork's launch must be one the fused generator takes)
    if (e->no_logits && !e->gen_rb_ok(B * e->cfg.seq_length)) return fail(BOFI_ERR_STATE, "this fork has no vocabulary-wide buffers and the launch would not take the fused generator");
    hipStream_t s = (hipStream_t)stream;
    if (!(flags & BOFI_FLAG_GRAPH))
        return e->enqueue_decode(feats, feats_dtype, att_len, B, R, flags, seq, seq_logprob, phrase_num, phrase_length,
                                 phrase_syn, memory_out, bound_iters, s);
    // graph path: the captured launch sequence is keyed by every argument that is baked into it
    std::vector<uintptr_t> key = {(uintptr_t)0, (uintptr_t)feats, (uintptr_t)feats_dtype, (uintptr_t)att_len, (uintptr_t)B, (uintptr_t)R,
                                  (uintptr_t)flags, (uintptr_t)seq, (uintptr_t)seq_logprob, (uintptr_t)phrase_num,
                                  (uintptr_t)phrase_length, (uintptr_t)phrase_syn, (uintptr_t)memory_out, (uintptr_t)bound_iters};
    key_call(key, e);
    return run_graphed(e, key, s, [&](hipStream_t cs) {
        return e->enqueue_decode(feats, feats_dtype, att_len, B, R, flags, seq, seq_logprob, phrase_num, phrase_length,
                                 phrase_syn, memory_out, bound_iters, cs);
    });
}

}  // extern "C"
