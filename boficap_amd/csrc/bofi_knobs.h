// The BOFI_* environment knobs of the library: ONE table (name, kind, default, when it is read, meaning) and one reader.  This is the list of
// record -- a name the library reads is a row here and appears as a string nowhere else (tests/test_knobs.py scans the sources for that).
// Host-side only, plain C++ (no HIP): the table's storage, the reader and bofi_reload_env are knobs.hip.
//
// Semantics.  Every RELOAD row is read from the environment at the first use of ANY knob and again, all rows at once, by bofi_reload_env();
// in between, a read is a load from the table: the value a launch sees is the value of the last reload, no use site keeps a copy, and no
// value is latched for the life of the process.  bofi_reload_env() also bumps g_env_generation, which is part of every graph key of the
// engine (a graph captured under other values is not replayed).  bofi_reload_env() must not run concurrently with launches or with another
// reload (it never has: callers change the environment and reload between decodes).
// CREATE rows are per-engine: bofi_engine_create reads them from the LIVE environment (knob_live) and stores them in the engine.
//
// Kinds:  INT   atoi of the value, the default when unset.
//         INTP  the same, and whether the variable is set at all (knob_set): unset is not the same as 0 for these.
//         STR   the text (knob_str; nullptr when unset); the default column is unused.
#pragma once
#include <cstdlib>

//  X(name, kind, default, when, meaning)
#define BOFI_KNOBS(X)                                                                                                                                    \
    /* engine.hip: which kernel family a sublayer takes */                                                                                              \
    X(BOFI_RB_MIN_ROWS, INT, 4096, RELOAD, "rows of a launch from which the row-block sublayer kernels run (0: always, huge: never = tiled family)")    \
    X(BOFI_RB_ATTN, INT, 1, RELOAD, "0: no fused attention sublayer kernel (attention core + closing GEMM)")                                            \
    X(BOFI_RB_ATTN_W, INT, 0, RELOAD, "wavefronts per workgroup of the fused attention sublayer: 8 / 16; 0: 8 alone at <= 20 queries, else 16")        \
    X(BOFI_RB_ATTN_PROJ, INT, 1, RELOAD, "query-projection tail of the fused attention sublayer: 0 never, 1 when launches overlap, 2 always")           \
    X(BOFI_RB_ATTN_SPLIT, INT, 1, RELOAD, "attention sublayer split (light core + W_o as the feed-forward launch's head): 0 never, 1 by size, 2 always") \
    X(BOFI_RB_ATTN_SPLIT_MIN_B, INT, 512, RELOAD, "images per launch from which BOFI_RB_ATTN_SPLIT=1 splits")                                           \
    X(BOFI_RB_ATTN_SPLIT_WHICH, INT, 3, RELOAD, "mask of the sublayers that may split: 1 encoder self-attention, 2 filling-pass cross-attention")      \
    X(BOFI_RB_GEMM, INT, 1, RELOAD, "0: no row-block LayerNorm-folded projections (tiled GEMM)")                                                        \
    X(BOFI_RB_FFN, INT, 1, RELOAD, "0: no row-block feed-forward sublayer kernel (two tiled GEMMs)")                                                    \
    X(BOFI_RB_FFN_PROJ, INT, 1, RELOAD, "projection tail of the feed-forward kernel: 0 never, 1 when launches overlap, 2 always")                       \
    X(BOFI_RB_FFN_PROJ_MAXN, INT, 0, RELOAD, "projections wider than this stay launches of their own (0: no limit)")                                    \
    X(BOFI_GEN_PAD, INT, 1, RELOAD, "0: generator in place on the one-tile GEMM instead of the padded weight")                                          \
    X(BOFI_FILL_QKV_TAB, INT, 1, RELOAD, "0: filling pass layer 0 projects q|k|v instead of reading the (label, position) table")                       \
    X(BOFI_REFINE_IDS_ONLY, INT, 1, RELOAD, "0: every refinement round stores its log-probs")                                                           \
    X(BOFI_BOUND_LOOP, INT, 1, RELOAD, "bounding loop kernel: 0 five launches per iteration, 1 loop kernel unless the decode runs alone, 2 always")    \
    X(BOFI_BOUND_LEAN, INT, 1, RELOAD, "0: five-launch bounding iterations on the general kernels, not the direct-operand ones")                        \
    X(BOFI_TAIL_DBG, INT, 0, RELOAD, "developer ablation bits of the bounding tail kernel")                                                             \
    X(BOFI_DBG_PART, INT, 0, RELOAD, "!= 0: the bounding tail also writes its partial results to a debug buffer")                                       \
    X(BOFI_BOUND_DENSE, INT, 0, CREATE, "!= 0: dense bounding phase (always on with more than one length head)")                                        \
    X(BOFI_SAIC_CACHE, INTP, 1, CREATE, "0: SAIC sends every row through the decoder in every iteration (no K/V cache)")                                \
    X(BOFI_SAIC_LEAN, INTP, 1, CREATE, "0: SAIC's row-list iterations on the general GEMM / attention kernels")                                         \
    X(BOFI_EXP_SKIP, STR, 0, RELOAD, "experiments build only: names of kernels to skip (timing only, RESULTS INVALID)")                                 \
    X(BOFI_EXP_ITERS, INTP, 0, RELOAD, "experiments build only: five-launch bounding iterations to enqueue (timing only, RESULTS INVALID)")             \
    /* rowblock.hip */                                                                                                                                  \
    X(BOFI_RB_FFN_V, INTP, 5, RELOAD, "feed-forward kernel: 5 = 80-row blocks, 2 = 64-row rb_ffn2; SET: also when the decode runs alone")               \
    X(BOFI_RB_FFN_BPW, INT, 1, RELOAD, "row blocks a workgroup of the 80-row feed-forward kernel walks (at least 1)")                                   \
    X(BOFI_RB_FFN_ONE, INT, 1, RELOAD, "0: the block-walking build of the feed-forward kernel also at one block per workgroup")                         \
    X(BOFI_RB_FFN_V5_ROWS, INT, 0, RELOAD, "rows from which the 80-row feed-forward kernel runs (below: the 64-row kernel)")                            \
    X(BOFI_RB_GEMM_MT, INT, 6, RELOAD, "row tiles per block of the row-block projections: 4 = 64 rows everywhere, 6 = 96 rows by size")                 \
    X(BOFI_RB_GEMM_MT8_ROWS, INT, 4096, RELOAD, "rows from which the 96-row projection blocks run")                                                     \
    X(BOFI_RB_GEMM_MT_MIN_N, INT, 0, RELOAD, "output columns from which the 96-row projection blocks run")                                              \
    X(BOFI_RB_GEN_MT6, INTP, -1, RELOAD, "generator on 96-row blocks: 1 always, 0 never, unset (-1) with launches in flight")                           \
    X(BOFI_VOCAB_MT, INT, 4, RELOAD, "row tiles per block of the fused generator: 4 = 64 rows, 6 = 96 rows")                                            \
    X(BOFI_VOCAB_SPLIT, INT, 0, RELOAD, "workgroups per row block of the fused generator: 1 / 2 / 4, 0 = by grid")                                      \
    X(BOFI_RB_DBG, INT, 0, RELOAD, "developer bits of the row-block kernels (16: in-kernel stamps, bofi_rb_stamps)")                                    \
    /* gemm_glds.hip, gemm_pers.hip: the tiled GEMM */                                                                                                  \
    X(BOFI_GEMM_TILE, STR, 0, RELOAD, "<BM>x<BN>x<NS>[x<waves>]: tile override for M > 64 (sweeps; tiles beyond the heuristic's need the experiments build)") \
    X(BOFI_GEMM_HEUR2, INT, 1, RELOAD, "0: round 1's tile heuristic (128-row tiles from 400 tiles, no deeper ring at long K)")                          \
    X(BOFI_GEMM_DEEP, INT, 1, RELOAD, "0: no whole-K ring for GEMMs of <= 64 rows")                                                                     \
    X(BOFI_GEMM_BANDS, INT, 0, RELOAD, "row bands of the XCD tile order: 1 / 2 / 4 / 8, 0 = cheapest by bytes")                                         \
    X(BOFI_GEMM_DBG, INT, 0, RELOAD, "developer ablation bits of the tiled GEMMs (1 no loads, 2 no MFMA, 4 return, 8 no epilogue, 16 plain order, 64 stamps)") \
    X(BOFI_GEMM_DBG_BUF, STR, 0, RELOAD, "device address of the stamp buffer of BOFI_GEMM_DBG bit 64")                                                  \
    X(BOFI_GEMM_PERS, INT, 1, RELOAD, "0: no persistent GEMM (one tile per workgroup)")                                                                 \
    X(BOFI_GEMM_PERS_MIN, INT, 90, RELOAD, "256 x 128 tiles from which the persistent GEMM runs")                                                       \
    X(BOFI_GEMM_PERS_BM128, INT, 128, RELOAD, "persistent GEMM: 128-row tiles up to this many 256-row tiles (0: 256-row tiles only)")                   \
    X(BOFI_GEMM_PERS_GRID, INT, 256, RELOAD, "persistent GEMM: workgroups at most")                                                                     \
    X(BOFI_GEMM_PERS_ROUNDS, INT, 1, RELOAD, "persistent GEMM: tiles per workgroup at least")                                                           \
    X(BOFI_GEMM_PERS_FAST, INT, 1, RELOAD, "0: persistent GEMM with the staged epilogue everywhere")                                                    \
    /* the other launchers */                                                                                                                           \
    X(BOFI_TN_WT, INT, 0, RELOAD, "gemm_tn: 2 or 4 = one register-staged tile class for everything")                                                    \
    X(BOFI_TN_WGS, INT, 0, RELOAD, "gemm_tn: workgroups of the split (0: by shape)")                                                                    \
    X(BOFI_ROWGEMM_NT, INT, 0, RELOAD, "bound_ops row GEMM: column tiles per wavefront 1 / 2 / 4 (0: by shape)")                                        \
    X(BOFI_ATTN_GENERIC, INTP, 0, RELOAD, "SET (any value): the generic attention kernel, never the register-resident bf16 one")                        \
    X(BOFI_TAIL_SMALL_AT, INT, 65, RELOAD, "images from which the two-per-CU variant of the bounding tail runs")                                        \
    X(BOFI_BL_DBG, INT, 0, RELOAD, "developer bits of the bounding loop kernel")                                                                        \
    X(BOFI_BL_PAIR, INT, 1, RELOAD, "loop kernel, two workgroups per group: 0 never, 1 launches of <= BOFI_BL_PAIR_MAX_B images, 2 always")             \
    X(BOFI_BL_PAIR_MAX_B, INT, 384, RELOAD, "images per launch up to which BOFI_BL_PAIR=1 pairs")

enum BofiKnob : int {                                      // the row index of a knob carries its name (global, like the BOFI_* constants of the ABI)
#define BOFI_KNOB_ID(name, kind, dflt, when, doc) name,
    BOFI_KNOBS(BOFI_KNOB_ID)
#undef BOFI_KNOB_ID
    BOFI_KNOB_COUNT
};

namespace bofi {

typedef BofiKnob Knob;
constexpr int KNOB_COUNT = BOFI_KNOB_COUNT;
enum KnobKind : int { KNOB_INT, KNOB_INTP, KNOB_STR };
enum KnobWhen : int { KNOB_RELOAD, KNOB_CREATE };
struct KnobRow { const char* name; KnobKind kind; int dflt; KnobWhen when; const char* doc; };
struct KnobValue { int i; bool set; const char* s; };      // s: the variable's text when it is set, else nullptr

extern const KnobRow g_knob_rows[KNOB_COUNT];
extern KnobValue g_knob_values[KNOB_COUNT];                // as of the last knobs_load
extern bool g_knobs_loaded;
extern int g_env_generation;                               // bumped by bofi_reload_env: part of every graph key

void knobs_load();                                         // every row from the environment (first use, bofi_reload_env)
KnobValue knob_live(Knob k);                               // one row from the environment NOW (CREATE rows; s is getenv's pointer)

inline const KnobValue& knob_value(Knob k) {
    if (!g_knobs_loaded) knobs_load();
    return g_knob_values[k];
}
inline int knob(Knob k) { return knob_value(k).i; }
inline bool knob_set(Knob k) { return knob_value(k).set; }
inline const char* knob_str(Knob k) { return knob_value(k).s; }

}  // namespace bofi
