// The row-block projection's device code (round 7), shared by the translation units that run it: rowblock.hip (rb_gemm_kernel, the projection tail of
// rb_ffn5_kernel, the fused generator) and bound_loop.hip (the projection role of bound_loop_kernel<5, true>: the decoder layers' cross K|V beside the
// bounding loop).  ONE statement of the block staging, the weight-stream segment and the chunk loop: whoever runs a projection through rb_gemm_block runs
// the instructions -- and writes the bits -- of rb_gemm_kernel.  The why of the shapes is told at the top of rowblock.hip.
#pragma once
#include "bofi_common.h"
#include "bofi_kernels.h"

namespace bofi {

// developer aid (BOFI_RB_DBG & 16): s_memtime stamps of workgroup 0, [wave][slot].  rowblock.hip -- the only launches that carry the debug bit -- defines the words and
// RB_STAMP in front of this header; any other translation unit gets the shared code without stamps.
#ifndef RB_STAMP
#define RB_STAMP(dbg, wave, lane, slot) do { } while (0)
#endif

constexpr int RB_PF = 4;             // weight-stream steps in flight per wavefront (divides 16: a segment starts at slot 0)

// byte offset of 16-byte chunk c of row r in a block of 1 024-byte rows
__device__ __forceinline__ int rb_off(int r, int c) { return r * 1024 + ((c ^ (r & 15)) << 4); }

__device__ __forceinline__ bf16x8 rb_ldw(const u32x4* p) { return __builtin_bit_cast(bf16x8, *p); }

// the first RB_PF steps of a wavefront's first segment
template <int NT, int PF = RB_PF>
__device__ __forceinline__ void rb_prime(const u32x4* seg, bf16x8 (&wb)[PF * NT]) {      // (flat: slot p, fragment nt at p*NT + nt)
#pragma unroll
    for (int p = 0; p < PF; ++p)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) wb[p * NT + nt] = rb_ldw(seg + (p * 4 + nt) * 64);
}

// One SEGMENT of a wavefront's weight stream: 16 k-steps (K = 512) of 4 fragments = 64 output columns; acc[nt][mt] += W-tile nt .
// block rows mt*16 .. +15.  `cur` is the segment (lane offset included), `nxt` the one that follows (its first RB_PF steps are
// requested during this segment's last ones).  D[n][m]: the weight is the MFMA row operand, so lane (l15, g) ends with row
// mt*16 + l15, columns nt*16 + g*4 .. +3.
// A lane's MFMA-operand address in a block: row mt*16 + l15, chunk kb*4 + g swizzled by the row -> (rb_lane_base ^ (kb << 6)) + mt*16384:
// the swizzle only touches bits 4..9, so a k-step costs one v_xor with an inline constant and the tile index rides in the offset field.
__device__ __forceinline__ int rb_lane_base(int l15, int g) { return l15 * 1024 + (((l15 >> 2) << 6) | ((g ^ (l15 & 3)) << 4)); }

template <int MT, int NT = 4, int PF = RB_PF, int MH = MT, bool PIPE = false>      // NT < 4: the wavefront takes NT of a step's four 16-column tiles (cur / nxt point at its first one); PF divides 16;
                                                                  // MH: row tiles per operand batch (MH < MT: fewer operand registers live at a time);
                                                                  // PIPE: the NEXT k-step's block operands are requested before this step's MFMAs (MT * 4 more registers): the LDS
                                                                  // latency of a step no longer sits between its reads and its MFMAs
__device__ __forceinline__ void rb_segment(const u32x4* cur, const u32x4* nxt, bf16x8 (&wb)[PF * NT], const unsigned char* smem, int lbase,
                                           f32x4 (&acc)[NT][MT], int kstride = 256) {      // kstride: u32x4 per k-step of the stream (256; 0 = a diagnostic that re-reads step 0)
    static_assert(MT % MH == 0, "operand batches divide the row tiles");
    static_assert(!PIPE || MH == MT, "the pipelined form reads a whole step's operands at once");
    asm volatile("" : "+v"(lbase));                   // (keeps the sixteen k-step addresses from being hoisted out of the caller's loops and spilled)
    if constexpr (PIPE) {
        bf16x8 xa[2][MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) xa[0][mt] = *reinterpret_cast<const bf16x8*>(smem + lbase + mt * 16384);
#pragma unroll
        for (int kb = 0; kb < 16; ++kb) {
            if (kb + 1 < 16) {
                const unsigned char* xn = smem + (lbase ^ ((kb + 1) << 6));
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) xa[(kb + 1) & 1][mt] = *reinterpret_cast<const bf16x8*>(xn + mt * 16384);
                __builtin_amdgcn_sched_barrier(0);            // (the scheduler sinks these reads behind this step's MFMAs otherwise: the point is that they fly meanwhile)
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[nt][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb[(kb % PF) * NT + nt], xa[kb & 1][mt], acc[nt][mt], 0, 0, 0);
            const u32x4* src = kb + PF < 16 ? cur + (kb + PF) * kstride : nxt + (kb + PF - 16) * kstride;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) wb[(kb % PF) * NT + nt] = rb_ldw(src + nt * 64);
            __builtin_amdgcn_sched_barrier(0);
        }
        return;
    }
#pragma unroll
    for (int kb = 0; kb < 16; ++kb) {
        int ad = lbase ^ (kb << 6);
        if constexpr (MT > 6) asm volatile("" : "+v"(ad));     // (eight row tiles: offsets past the 16-bit field -- computed here, per step, not sixteen steps ahead)
        const unsigned char* xp = smem + ad;
#pragma unroll
        for (int mb = 0; mb < MT; mb += MH) {
            bf16x8 xa[MH];
#pragma unroll
            for (int mt = 0; mt < MH; ++mt) xa[mt] = *reinterpret_cast<const bf16x8*>(xp + (mb + mt) * 16384);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int mt = 0; mt < MH; ++mt) acc[nt][mb + mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb[(kb % PF) * NT + nt], xa[mt], acc[nt][mb + mt], 0, 0, 0);
        }
        const u32x4* src = kb + PF < 16 ? cur + (kb + PF) * kstride : nxt + (kb + PF - 16) * kstride;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) wb[(kb % PF) * NT + nt] = rb_ldw(src + nt * 64);
        __builtin_amdgcn_sched_barrier(0);            // the scheduler would sink the loads next to their use: the prefetch distance is the point
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// The chunk loop of the LayerNorm-folded projections (rb_gemm_kernel below; also the projection tail of rb_ffn5_kernel): a block of bf16 rows
// in LDS, its row statistics, and a wavefront's 64-column chunks of the fragment-major weight.
template <bool F32OUT, int MT>
struct RbGemmCfg {
    static constexpr int BR = MT * 16;                          // rows per block
    static constexpr int SP = F32OUT ? 272 : 144;               // staging row pitch (bytes): 64 columns + 16 B
    static constexpr int TPS = (MT == 8 || MT == 5) ? 1 : MT == 6 ? (F32OUT ? 1 : 2) : (F32OUT ? 2 : 4);      // row tiles staged at a time (divides MT)
    static constexpr int STG = TPS * 16 * SP;                   // staging bytes per wavefront
    static constexpr int XT = BR * 1024;
    static constexpr int STAT = XT + 8 * STG;                   // s_mean[BR], s_rstd[BR]
    static constexpr int CST = STAT + BR * 8;                   // per wavefront [2][64]: c | cs of the current chunk
    static constexpr int LDS = CST + 8 * 512;
};

template <bool F32OUT, int MT>
__device__ __forceinline__ void rb_gemm_chunks(const RbGemmArgs& a, const unsigned char* blk, unsigned char* stage_all, float* cst, const float* s_mean,
                                               const float* s_rstd, int m0, int wave, int lane, int ch0, int chstep, bf16x8 (&wb)[RB_PF * 4]) {
    using Cfg = RbGemmCfg<F32OUT, MT>;
    constexpr int SP = Cfg::SP, TPS = Cfg::TPS;
    const int l15 = lane & 15, g = lane >> 4, nchunks = a.N >> 6;
    auto seg = [&](int ch) { return a.wp + (size_t)ch * (16 * 256) + lane; };
    constexpr bool STATS_IN_REGS = MT <= 6;                    // (128-row blocks: the 16 statistics registers are what the accumulators need -- read per pass from LDS)
    float mu[STATS_IN_REGS ? MT : 1], rs[STATS_IN_REGS ? MT : 1];
    if constexpr (STATS_IN_REGS) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) { mu[mt] = s_mean[mt * 16 + l15]; rs[mt] = s_rstd[mt * 16 + l15]; }
    }
    const int lbase = rb_lane_base(l15, g);
    unsigned char* stage = stage_all + wave * Cfg::STG;
    int nstamp = 0;
    float* mycst = cst + wave * 128;
    const int rows_live = min(Cfg::BR, a.M - m0);

#pragma unroll 1
    for (int ch = ch0; ch < nchunks; ch += chstep) {
        // this chunk's column constants: requested now (older than the weight prefetch), parked in LDS at the epilogue
        const float cv = a.c[ch * 64 + lane], csv = a.cs[ch * 64 + lane];
        f32x4 acc[4][MT];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[nt][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
        rb_segment<MT, 4, RB_PF, (MT == 5 ? 5 : MT > 4 ? MT / 2 : MT)>(seg(ch), seg(ch + chstep < nchunks ? ch + chstep : ch), wb, blk, lbase, acc);
        if (nstamp < 8) RB_STAMP(a.dbg, wave, lane, 2 * nstamp);            // chunk's MFMAs issued
        mycst[lane] = cv; mycst[64 + lane] = csv;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // (the row pointers of the stores hang on a lane value the compiler cannot see through and advance by additions: as invariants of the chunk
        // loop they are hoisted above it -- two registers per store -- and the accumulators spill)
        constexpr int LPR = F32OUT ? 16 : 8, RPI = 64 / LPR;
        int lnv = lane;
        asm volatile("" : "+v"(lnv));
        int rrow = lnv / LPR;                                  // row of the block this lane stores next
        unsigned char* yp = static_cast<unsigned char*>(a.y) + ((size_t)(m0 + rrow) * a.ldy + ch * 64) * (F32OUT ? 4 : 2) + (lnv % LPR) * 16;
        const size_t ystep = (size_t)RPI * a.ldy * (F32OUT ? 4 : 2);
        const unsigned char* srd = stage + rrow * SP + (lnv % LPR) * 16;
#pragma unroll
        for (int pass = 0; pass < MT / TPS; ++pass) {
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const float4 cc = *reinterpret_cast<const float4*>(mycst + nt * 16 + g * 4);
                const float4 cs = *reinterpret_cast<const float4*>(mycst + 64 + nt * 16 + g * 4);
#pragma unroll
                for (int mh = 0; mh < TPS; ++mh) {
                    const int mt = pass * TPS + mh;
                    const f32x4 t = acc[nt][mt];
                    const float mu_ = STATS_IN_REGS ? mu[STATS_IN_REGS ? mt : 0] : s_mean[mt * 16 + l15], rs_ = STATS_IN_REGS ? rs[STATS_IN_REGS ? mt : 0] : s_rstd[mt * 16 + l15];
                    float v0 = rs_ * (t[0] - mu_ * cs.x) + cc.x, v1 = rs_ * (t[1] - mu_ * cs.y) + cc.y;
                    float v2 = rs_ * (t[2] - mu_ * cs.z) + cc.z, v3 = rs_ * (t[3] - mu_ * cs.w) + cc.w;
                    if (a.relu) { v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); v2 = fmaxf(v2, 0.f); v3 = fmaxf(v3, 0.f); }
                    unsigned char* sp = stage + (mh * 16 + l15) * SP + (nt * 16 + g * 4) * (F32OUT ? 4 : 2);
                    if constexpr (F32OUT) *reinterpret_cast<float4*>(sp) = make_float4(v0, v1, v2, v3);
                    else *reinterpret_cast<uint2*>(sp) = make_uint2(pack_bf16(v0, v1), pack_bf16(v2, v3));
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            // whole row pieces: bf16 8 lanes x 16 B = a row's 128 B (8 rows per instruction); float32 16 lanes x 16 B = 256 B (4 rows)
#pragma unroll
            for (int it = 0; it < TPS * 16 / RPI; ++it, yp += ystep, rrow += RPI) {
                const u32x4 v = *reinterpret_cast<const u32x4*>(srd + it * RPI * SP);
                if (rrow < rows_live) *reinterpret_cast<u32x4*>(yp) = v;
            }
            __builtin_amdgcn_wave_barrier();
        }
        if (nstamp < 8) RB_STAMP(a.dbg, wave, lane, 2 * nstamp + 1);        // chunk stored
        ++nstamp;
    }
}

// One row block of y[M][N] = epilogue(LN(x) . W^T) (rb_gemm_kernel's whole body; the why is told there): the block's rows m0 .. m0 + BR - 1 of the float32 stream staged
// as bf16 (row statistics on the way), then this wavefront's chunks ch0, ch0 + chstep, ... < N / 64.  All 512 threads of the workgroup; smem: Cfg::LDS bytes.
// TAIL_SUMS: the row sums in the order of rb_ffn5_kernel's projection tail -- a lane's four 32-column steps of each 128-column quarter, the eight lanes of the row, then
// (q0 + q1) + (q2 + q3) -- so that a projection of the feed-forward's float32 output has the TAIL's bits (the projection role of bound_loop_kernel<5, true>).
template <bool F32OUT, int MT, bool TAIL_SUMS = false>
__device__ __forceinline__ void rb_gemm_block(const RbGemmArgs& a, unsigned char* smem, int m0, int wave, int lane, int ch0, int chstep) {
    using Cfg = RbGemmCfg<F32OUT, MT>;
    unsigned char* xt = smem;
    unsigned char* stage_all = smem + Cfg::XT;
    float* s_mean = reinterpret_cast<float*>(smem + Cfg::STAT);
    float* s_rstd = s_mean + Cfg::BR;
    float* cst = reinterpret_cast<float*>(smem + Cfg::CST);
    const int nchunks = a.N >> 6;
    auto seg = [&](int ch) { return a.wp + (size_t)ch * (16 * 256) + lane; };
    RB_STAMP(a.dbg, 8 + wave, lane, 0);                        // entry (rows 8-15: this kernel has 8 wavefronts)
    bf16x8 wb[RB_PF * 4];
    if (ch0 < nchunks) rb_prime<4>(seg(ch0), wb);
    constexpr int RPW = MT * 2;                                // rows a wavefront stages
#pragma unroll
    for (int pass = 0; pass < (RPW + 7) / 8; ++pass) {         // stage the block: wavefront w takes rows RPW*w .. +RPW-1, eight at a time, eight lanes per row
        const int lr = pass * 8 + (lane >> 3), r = wave * RPW + lr, sub = lane & 7, m = m0 + r;
        const bool mine = lr < RPW;
        float4 v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j)
            v[j] = (mine && m < a.M) ? *reinterpret_cast<const float4*>(a.x + (size_t)m * a.ldx + j * 32 + sub * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        float sm = 0.f, sq = 0.f;
        // (the contraction of x.x + y.y that the compiler has always chosen for these kernels and for the tail, spelled out: left free, it chose fma(y, y, x.x) once this
        // code was inlined from a header -- other row statistics in the last bit, other bf16 outputs here and there)
        if constexpr (TAIL_SUMS) {
            float ps1[4] = {0.f, 0.f, 0.f, 0.f}, ps2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                ps1[j >> 2] += (v[j].x + v[j].y) + (v[j].z + v[j].w);
                ps2[j >> 2] += __builtin_fmaf(v[j].x, v[j].x, v[j].y * v[j].y) + __builtin_fmaf(v[j].z, v[j].z, v[j].w * v[j].w);
                if (mine) *reinterpret_cast<uint2*>(xt + rb_off(r, j * 4 + (sub >> 1)) + (sub & 1) * 8) = make_uint2(pack_bf16(v[j].x, v[j].y), pack_bf16(v[j].z, v[j].w));
            }
#pragma unroll
            for (int w = 0; w < 4; ++w) { ps1[w] = oct_sum(ps1[w]); ps2[w] = oct_sum(ps2[w]); }
            sm = (ps1[0] + ps1[1]) + (ps1[2] + ps1[3]); sq = (ps2[0] + ps2[1]) + (ps2[2] + ps2[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                sm += (v[j].x + v[j].y) + (v[j].z + v[j].w);
                sq += __builtin_fmaf(v[j].x, v[j].x, v[j].y * v[j].y) + __builtin_fmaf(v[j].z, v[j].z, v[j].w * v[j].w);
                if (mine) *reinterpret_cast<uint2*>(xt + rb_off(r, j * 4 + (sub >> 1)) + (sub & 1) * 8) = make_uint2(pack_bf16(v[j].x, v[j].y), pack_bf16(v[j].z, v[j].w));
            }
            sm = oct_sum(sm); sq = oct_sum(sq);
        }
        if (mine && sub == 0) {
            const float mean = sm * (1.0f / 512.0f);
            const float var = fmaxf((sq - sm * mean) * (1.0f / 511.0f), 0.f);
            s_mean[r] = mean;
            s_rstd[r] = 1.0f / (sqrtf(var) + 1e-6f);
        }
    }
    __syncthreads();
    RB_STAMP(a.dbg, 8 + wave, lane, 1);                        // block staged
    rb_gemm_chunks<F32OUT, MT>(a, smem, stage_all, cst, s_mean, s_rstd, m0, wave, lane, ch0, chstep, wb);
    RB_STAMP(a.dbg, 8 + wave, lane, 2);                        // exit
}

}  // namespace bofi
