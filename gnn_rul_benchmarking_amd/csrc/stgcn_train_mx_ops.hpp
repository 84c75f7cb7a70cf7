// Constant operands and small helpers of the matrix-core training chains (stgcn_train_mx.hip: num_patch <= 15, four samples per
// wavefront; stgcn_train_mxw.hip: 16 <= num_patch <= 47, one sample per wavefront in column tiles): the split-operand forms of theta,
// of the convolutions (forward and transposed) and the kernels' argument block.
#pragma once
#include <type_traits>

#include "stgcn_mx.hpp"
#include "stgcn_train_layout.hpp"
#include "stgcn_train_mx.hpp"

namespace rulgnn {
namespace {

constexpr int MXT_ZERO_FLOATS = 192;     // zeroed LDS words padded lanes read instead of a tile (largest use: 3 * 55 + 1)
constexpr int MXT_SCRATCH_FLOATS = 128;  // head: d pool / arg-max exchange between the row mapping and the D layout
constexpr int MXT_SHIFT_FLOATS = 264;    // shift tile: [64 lanes + zero slot] x (hi pair | lo pair) = 1040 bytes
// Backward phases: the transposing image of the conv weight gradient's two operands (d z, and H or V), one per wavefront.  Unit: the
// 8-byte chunk (t, g) = the f16 of column t, slots 4 g .. 4 g + 3, as one plane (hi or lo) of a Pk holds them.  Four planes of 64 chunks;
// the H / V planes carry one more chunk of zeros, which the shifted read addresses for the columns in front of the tile.
constexpr int WG_ZERO = 64;
constexpr int WG_DZ_HI = 0, WG_DZ_LO = 64, WG_H_HI = 128, WG_H_LO = WG_H_HI + 65;
constexpr int MXT_WG_FLOATS = (2 * (WG_H_LO + 65) + 3) & ~3;     // 2080 bytes; the tiles behind it stay 16-byte aligned (LDS-DMA)
constexpr int MXT_WAVES = 4;              // wavefronts per workgroup: they share the BatchNorm table and reduce their sums / gradient rows in LDS
constexpr int MXT_RED_FLOATS = 448;      // gradient row image of a phase: at most 15 x 15 + 15 + 200 floats
constexpr int MXT_BNC = BN_TABLE_ROWS;   // per-BatchNorm constants: mean, istd, gamma, beta, gamma istd, mean(dy), mean(dy xhat)

enum { PH_F = 0, PH_TOP = 1, PH_G = 2 };

// How the records cross the kernel boundaries (StorePolicy, stgcn_mx.hpp; every alternative measured: profiles/r15_record_stores.md).
// Stores: agent-scope write-through for every record -- the full tiles as whole 16-byte pieces out of the wavefront's staging tile (in
// place, as dwords, write-through costs F_2 +9 us), the small records (d X_L, predictions, mask words, gradient rows) as dwords.
// Loads: the phase that reads a record last in the step asks for it non-temporally.
constexpr int MXT_RECORD_POLICY = ST_WT;
constexpr bool MXT_LAST_READER_NT = true;

// Who reads H_l = leaky(theta(A X_l)) from its record (MxTrainK::hrec) instead of rebuilding it from X_l and the adjacency, beyond the
// round-8 readers F_{2l+1}, TOP and G_{2l+1} of the layers l >= 1.  One switch per reader, each measured on top of the ones before it
// (profiles/r18_h_records.md, us of the reader's own kernel at batch 65 536; -DMXT_H_READERS=<bits> builds a combination with
// tools/build_variants.py):
//   bit 0  G_{2l}, l >= 1 <- H_l    (no new record)                                       G_2 -2.1 (G_3, no longer the last reader, +0.4)
//   bit 1  G_1 and, at L = 1, TOP <- H_0    } any of these: F_1 WRITES the H_0 record      G_1 -5.8; F_1 +2.9 for the record
//   bit 2  G_0 <- H_0                       } (mxt_h0_record) -- never F_0, whose H_0 is   G_0 -0.65
//   bit 3  F_{2l}, l >= 1: its pass over    } computed under the per-sample 2^-k scale     F_2 -2.0
//          layer l-1 <- H_{l-1}             } and rounds differently in its lo halves
// (TOP at L = 1 shares G_1's switch and has not been timed: the flagship has two layers.)
// ON: bits 0 and 1 -- 0.3048 -> 0.2991 ms per step (a later session: 0.3040 -> 0.3015), every run faster than every run of the
// parent.  OFF: bits 2 and 3.  Their own kernels get shorter as listed, but with
// either of them the step falls into a slow mode in one run of two or three (all four: 0.3036 / 0.2988 / 0.3036 ms against the
// parent's 0.3044; under the profiler the sum of the ten kernels 305.5 or 309.3 us, F_3, G_3 and G_2 -- kernels these bits do not
// touch -- 0.3 to 0.9 us longer in the slow runs), and the opt-in single launch loses 4 us more at batch 100.  Not understood; the
// bodies stay, they are a few lines on top of bit 0's.
#ifndef MXT_H_READERS
#define MXT_H_READERS 3
#endif
constexpr bool MXT_H_READ_G_EVEN = (MXT_H_READERS & 1) != 0;
constexpr bool MXT_H0_READ_G1 = (MXT_H_READERS & 2) != 0;
constexpr bool MXT_H0_READ_TOP = MXT_H0_READ_G1;
constexpr bool MXT_H0_READ_G0 = (MXT_H_READERS & 4) != 0;
constexpr bool MXT_H_READ_F_EVEN = (MXT_H_READERS & 8) != 0;
// F_1 writes H_0 when somebody in an L-layer step reads it (F_{2l} at l = 1 reads H_0, at l >= 2 a record that exists anyway)
constexpr bool mxt_h0_record(int L) { return MXT_H0_READ_G1 || MXT_H0_READ_G0 || (L == 1 ? MXT_H0_READ_TOP : MXT_H_READ_F_EVEN); }
// G_{2l} with the H tile beside X_l, the adjacency, d(x0 + H), d X_{l+1}, Q_l and the staging tile: at l >= 1 that is 82 896 bytes at
// N = 15, L = 3 -- more than the 80 KB that keep two workgroups on a CU -- so there only the fixed-N (14) instantiations read the record
// and the generic ones keep the rebuild.  G_0 has three of those tiles and fits at every N.  (`nfix`: the kernel's NFIX.)
constexpr bool mxt_g_even_reads_h(int ly, int nfix) { return ly == 0 ? MXT_H0_READ_G0 : (MXT_H_READ_G_EVEN && nfix == 14); }

// How a full-tile record (X_l, Q_l, H_l, d(x0 + H), d X_l) gets from the D-layout registers into its staging tile and out of it
// (narrow chain; profiles/r24_record_stores.md).  One switch per piece, built cumulatively (-DMXT_RECORD_STAGING=<bits>,
// tools/build_variants.py):
//   bit 0  staged where produced: a phase writes the values into the staging tile when they exist (end of the tile body; each half of a
//          G tile its two samples) and the tile is the pending storage -- no loop-carried copy in registers.  F_{2l}, l >= 1, gets one
//          staging tile per record (three).
//   bit 1  branch-free staging writes: per register row one LDS address, the lane's word of the tile or, for a padding lane, a word of
//          the dump area (MxtLds::dump) -- no exec-mask region per write.
//   bit 2  (needs bit 0) the 16-byte LDS reads of the pending records are issued IN FRONT of the tile's s_waitcnt vmcnt(0), the
//          write-through stores back to back behind it, with a compile-time piece count.
// Measured cumulatively at batch 65 536, ms per step, three alternated runs each: parent 0.3011-0.3024, bit 0 alone 0.3014-0.3028 (no
// gain by itself), bits 0-1 0.2991-0.2994, all three 0.2952-0.2959.  ALL ON.  Bit 2 is not applied to G_{2l}, l >= 1, and to the
// generic-N single launch (scratch above the parent's: mxt_phase_body); the opt-in single launch at batch 100 loses 5 us with them.
#ifndef MXT_RECORD_STAGING
#define MXT_RECORD_STAGING 7
#endif
constexpr bool MXT_STAGE_EARLY = (MXT_RECORD_STAGING & 1) != 0;
constexpr bool MXT_STAGE_BRANCHFREE = (MXT_RECORD_STAGING & 2) != 0;
constexpr bool MXT_STAGE_READ_AHEAD = (MXT_RECORD_STAGING & 4) != 0;
static_assert(!MXT_STAGE_READ_AHEAD || MXT_STAGE_EARLY, "the reads can go in front of the wait only where the staging tile is the pending storage");
// the dump area: a padding lane writes word `lane` + s N, s < 4 -- the head's exchange words, which only TOP uses and TOP writes no tile
constexpr int MXT_DUMP_FLOATS = 64 + 3 * 15;
static_assert(MXT_DUMP_FLOATS <= MXT_SCRATCH_FLOATS, "the dump area of the staging writes lies inside the scratch words");
constexpr int MXT_MAX_PIECES = 3;        // 16-byte pieces of a [10][4 N] tile per lane: 10 N <= 150 of them on 64 lanes

// What phase (L, kind, idx) of a training chain is, once, for the bodies' `if constexpr`, the LDS layouts and the launchers.  (`nfix`: the
// kernel's NFIX; the wide chain, which has no H records, passes 0.)
struct MxtTraits {
    int LY, BLK, LIN, AF, NTH, NSTG;
    bool WITH_PREV, BWD_PREV, GRAD_IN, GRAD_TOP, NEED_SB, H_OUT, H_IN, H_TOP, H_PREV, H_GE, H_TILE, TILE_OUT, LATE;
};
__host__ __device__ constexpr MxtTraits mxt_traits(int L, int kind, int idx, int nfix) {
    MxtTraits t{};
    t.LY = kind == PH_TOP ? L - 1 : idx / 2;
    t.BLK = kind == PH_TOP ? 1 : idx % 2;
    t.WITH_PREV = kind == PH_F && t.BLK == 0 && t.LY >= 1;     // F_{2l}: layer l-1 in full first (its input is this phase's input)
    t.BWD_PREV = kind == PH_G && t.BLK == 0 && t.LY >= 1;      // G_{2l}: the sums of BatchNorm 2l-1 (its gated x-hat comes from F_{2l})
    t.LIN = t.WITH_PREV ? t.LY - 1 : t.LY;                     // the layer whose input record is the main input
    t.GRAD_IN = kind == PH_G && (t.BLK == 1 || t.LY >= 1);     // a gradient tensor enters: d X_{l+1}
    t.GRAD_TOP = t.GRAD_IN && t.LY == L - 1;                   // ... in TOP's (value, arg-max) form
    t.NEED_SB = kind == PH_G && t.BLK == 0;
    // the H_l record (MxTrainK::hrec): the first phase of the narrow chain that computes H of layer LY writes it -- F_{2l}, l >= 1; F_1 for
    // H_0 (F_0 has it only under its per-sample scale) where a reader of H_0 is switched on.  F_{2l+1} and G_{2l+1} need nothing else
    // of X_l and A, and start from it.  (The readers beyond round 8's: MXT_H_READERS)
    t.H_OUT = kind == PH_F && (t.WITH_PREV || (idx == 1 && mxt_h0_record(L)));
    t.H_IN = (kind == PH_F && t.BLK == 1 && t.LY >= 1) || (kind == PH_G && t.BLK == 1 && (t.LY >= 1 || MXT_H0_READ_G1));
    t.H_TOP = kind == PH_TOP && (t.LY >= 1 || MXT_H0_READ_TOP);    // TOP: X_l for the residual, H_l in place of the adjacency
    t.H_PREV = t.WITH_PREV && MXT_H_READ_F_EVEN;                   // F_{2l}: the pass over layer l-1 starts from H_{l-1}
    t.H_GE = kind == PH_G && t.BLK == 0 && mxt_g_even_reads_h(t.LY, nfix);    // G_{2l}: H_l beside X_l and the adjacency
    t.H_TILE = t.H_PREV || t.H_GE;                                 // ... in a tile of its own
    // every full-tile record a phase writes (F_{2l}: X_l, Q_l, H_l; G_{2l+1}: d(x0 + H); G_{2l}, l >= 1: d X_l) leaves through a staging
    // tile per wavefront: one per record where the tile is the pending storage (MXT_STAGE_EARLY), else one for all, one record after
    // the other
    t.TILE_OUT = t.WITH_PREV || t.H_OUT || (kind == PH_G && t.BLK == 1) || t.BWD_PREV;
    t.NSTG = !t.TILE_OUT ? 0 : (MXT_STAGE_EARLY && t.WITH_PREV ? 3 : 1);
    t.AF = t.H_IN ? 0 : 220;                                   // floats of the narrow chain's adjacency tile
    // wide chain.  G_{2l} carries the most state (the theta-gradient tiles): its records are read from LDS where they are used instead of
    // being held in registers across the sample, the next sample's records are requested once the region is free, and d X_l is stored
    // without the delay
    t.LATE = kind == PH_G && t.BLK == 0;
    t.NTH = 1 + (t.WITH_PREV ? 1 : 0) + (t.BWD_PREV ? 1 : 0);  // theta operand tables: theta^T(LY) | theta^T(LY-1) | theta(LY)
    return t;
}
// every phase of the chains' phase kernels, in the order TOP, F_1 .. F_{2L-1}, G_0 .. G_{2L-1}
template <typename FN>
constexpr void mxt_each_phase(int L, FN fn) {
    fn(PH_TOP, 0);
    for (int i = 1; i < 2 * L; ++i) fn(PH_F, i);
    for (int i = 0; i < 2 * L; ++i) fn(PH_G, i);
}

struct Op2 { u32x4 h, l; };              // a D-layout tensor as the ({hi | hi}, {lo | lo}) operand pair against a {hi | lo} partner
struct Pk { u32x2 hi, lo; };             // its packed halves: slots 4 g .. 4 g + 3 of this lane's column

__device__ __forceinline__ Pk pack3(float a, float b, float c, float d) {
    const Split2 p01 = split2(a, b), p23 = split2(c, d);
    return Pk{u32x2{p01.hi, p23.hi}, u32x2{p01.lo, p23.lo}};
}
__device__ __forceinline__ u32x4 cat(const u32x2& a, const u32x2& b) { return u32x4{a.x, a.y, b.x, b.y}; }
__device__ __forceinline__ f32x4 mfma16z(const u32x4& a, const u32x4& b) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    return mfma16(a, b, zero);
}
__device__ __forceinline__ bool finite_f(float v) { return __builtin_fabsf(v) <= 3.0e38f; }

// shift tile access for both directions: column t - d (forward taps) or t + d (transposed convolution); `rd` = the lane to read or 64
__device__ __forceinline__ Shifted shift_read(u32x2* tile, int rd, int rd_lo, int lane, const Pk& p) {
    return shift_columns(tile, rd, rd_lo, lane, p.hi, p.lo);
}

// Where chunk (t, g) of a plane sits.  Writes (ds_write_b64: groups of 16 lanes = the 16 columns of one g, 32 banks of 4 bytes) and the
// transposed read (groups of 32 lanes = 8 consecutive rows x 4 chunks, 64 banks) are both free of bank conflicts: within 8 rows the
// chunks of a row are 8 apart, and the upper 8 rows rotate g by one so that columns t and t + 8 of one g land 64 bytes apart.
__host__ __device__ constexpr int wg_chunk(int t, int g) { return (t & 7) + 8 * ((g + (t >> 3)) & 3) + 32 * (t >> 3); }
// ds_read_b64_tr_b16: lane i of a 16-lane group receives 16-bit column i of the four 8-byte rows the group's lanes 4 q + p address
// (row q, columns 4 p .. 4 p + 3), row q in element q.  Every lane must be active and supply an 8-byte aligned address.
typedef short s16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ u32x2 lds_read_tr16(const u32x2* p) {
    return __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p));
}

struct ConvOp { u32x4 hi, lo; };

// A operand of a forward convolution: row m = col <-> output channel; k-slots [0..3] = tap at t, [4..7] = tap at t - d, each x input
// slot 4 g + r; `scale` multiplies the weights of this lane's output channel, `pre` undoes a factor carried by the data (V = 4 o0),
// `shift` rides in slot 3 of lane group 0 against the constant 1 of the data operand.  In two steps: the raw taps are loaded in front of
// the BatchNorm-table hand-over of the prologue (they do not depend on it), scaled and split behind it.
struct ConvRaw { float wc[4], wd[4]; };
__device__ __forceinline__ ConvRaw conv_fwd_raw(const float* cw, int g, int col) {
    const int co = slot_chan(col), coc = co >= 0 ? co : 0;
    ConvRaw w;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int ci = slot_chan(4 * g + r);
        const bool ok = co >= 0 && ci >= 0;
        const float2 taps2 = *reinterpret_cast<const float2*>(cw + (coc * F + (ci >= 0 ? ci : 0)) * 2);
        w.wc[r] = ok ? taps2.y : 0.f;
        w.wd[r] = ok ? taps2.x : 0.f;
    }
    return w;
}
__device__ __forceinline__ ConvOp conv_fwd_operand(const ConvRaw& w, float scale, float shift, float pre, int g, int col) {
    const int co = slot_chan(col);
    float wc[4], wd[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        wc[r] = w.wc[r] * (scale * pre);
        wd[r] = w.wd[r] * (scale * pre);
    }
    if (g == 0) wc[3] = co >= 0 ? shift : 0.f;
    const Split2 c01 = split2(wc[0], wc[1]), c23 = split2(wc[2], wc[3]), d01 = split2(wd[0], wd[1]), d23 = split2(wd[2], wd[3]);
    return ConvOp{u32x4{c01.hi, c23.hi, d01.hi, d23.hi}, u32x4{c01.lo, c23.lo, d01.lo, d23.lo}};
}
// A operand of the TRANSPOSED convolution: row m = col <-> input channel ci; k-slots [0..3] = w[co][ci][tap at t] against d z of
// column t, [4..7] = w[co][ci][tap at t - d] against d z of column t + d, co = slot 4 g + r.
// (loads and conversion apart: a prologue issues every load before it converts anything -- one memory round trip)
__device__ __forceinline__ ConvRaw conv_bwd_raw(const float* cw, int g, int col) {
    const int ci = slot_chan(col), cic = ci >= 0 ? ci : 0;
    ConvRaw w;                               // wc: tap at t, wd: tap at t - d
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int co = slot_chan(4 * g + r);
        const bool ok = co >= 0 && ci >= 0;
        const float2 taps2 = *reinterpret_cast<const float2*>(cw + ((co >= 0 ? co : 0) * F + cic) * 2);
        w.wc[r] = ok ? taps2.y : 0.f;
        w.wd[r] = ok ? taps2.x : 0.f;
    }
    return w;
}
__device__ __forceinline__ ConvOp conv_bwd_pack(const ConvRaw& w) {
    const Split2 c01 = split2(w.wc[0], w.wc[1]), c23 = split2(w.wc[2], w.wc[3]), d01 = split2(w.wd[0], w.wd[1]), d23 = split2(w.wd[2], w.wd[3]);
    return ConvOp{u32x4{c01.hi, c23.hi, d01.hi, d23.hi}, u32x4{c01.lo, c23.lo, d01.lo, d23.lo}};
}
__device__ __forceinline__ ConvOp conv_bwd_operand(const float* cw, int g, int col) { return conv_bwd_pack(conv_bwd_raw(cw, g, col)); }

struct ThetaOp { u32x4 hi, lo; };
struct ThetaRaw { float w[4]; };
__device__ __forceinline__ ThetaOp theta_pack(const ThetaRaw& t) {
    const Split2 p01 = split2(t.w[0], t.w[1]), p23 = split2(t.w[2], t.w[3]);
    return ThetaOp{u32x4{p01.hi, p23.hi, p01.hi, p23.hi}, u32x4{p01.lo, p23.lo, p01.lo, p23.lo}};
}
// theta^T as B operand of Hp = T x theta^T + b: column j = col, k-slot 4 g + r <-> patch k, k = 15 <-> bias; (1 + a)/2 folded in
__device__ __forceinline__ ThetaRaw theta_t_raw(const float* lp, int N, int g, int col) {
    ThetaRaw t;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int k = 4 * g + r;
        const bool ok = col < N && (k < N || k == 15);
        const int idx = k == 15 ? off_theta_b(N) + col : off_theta_w(N) + col * N + k;
        const float v = lp[ok ? idx : 0];
        t.w[r] = ok ? v * (0.5f * (1.f + LEAKY)) : 0.f;
    }
    return t;
}
__device__ __forceinline__ ThetaOp theta_t_operand(const float* lp, int N, int g, int col) { return theta_pack(theta_t_raw(lp, N, g, col)); }
// theta as B operand of d X = U x theta: column k' = col, k-slot 4 g + r <-> row j of theta
__device__ __forceinline__ ThetaRaw theta_n_raw(const float* lp, int N, int g, int col) {
    ThetaRaw t;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int j = 4 * g + r;
        const bool ok = col < N && j < N;
        const float v = lp[ok ? off_theta_w(N) + j * N + col : 0];
        t.w[r] = ok ? v : 0.f;
    }
    return t;
}
__device__ __forceinline__ ThetaOp theta_n_operand(const float* lp, int N, int g, int col) { return theta_pack(theta_n_raw(lp, N, g, col)); }

// Everything one layer's forward needs as constants: theta^T, the two convolutions, the affine part of its BatchNorms per D register
struct LayerK {
    ThetaOp th;
    ConvOp w[2];
    float gam[2][3], bet[2][3];
};

// `mode[blk]`: 0 = convolution not needed, 1 = raw weights (its BatchNorm statistics are what this phase computes), 2 = x-hat fold
// (weights x istd, shift -mean istd: the product IS x-hat, y = gamma x-hat + beta one fma behind it)
struct LayerRaw {
    ThetaRaw th;
    ConvRaw w[2];
};
// (`theta` false: the phase starts from a saved H and needs no theta^T -- no gathers, a zero operand)
__device__ __forceinline__ void layer_raw(LayerRaw& k, const float* prm, int l, int N, int g, int col, int mode0, int mode1, bool theta = true) {
    const float* lp = prm + l * layer_stride(N);
    if (theta) k.th = theta_t_raw(lp, N, g, col);
    else k.th = ThetaRaw{{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
        if ((blk == 0 ? mode0 : mode1) != 0) k.w[blk] = conv_fwd_raw(lp + off_conv_w(N, blk), g, col);
        else k.w[blk] = ConvRaw{{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    }
}
__device__ __forceinline__ void layer_constants(LayerK& k, const LayerRaw& raw, const float* bnc, int l, int g, int col, int mode0, int mode1) {
    k.th = theta_pack(raw.th);
    const int co = slot_chan(col), coc = co >= 0 ? co : 0;
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
        const int mode = blk == 0 ? mode0 : mode1;
        const float* q = bnc + (2 * l + blk) * MXT_BNC * F;
        const float istd = mode == 2 ? q[1 * F + coc] : 1.f;
        const float shift = mode == 2 ? -q[0 * F + coc] * istd : 0.f;
        if (mode != 0) k.w[blk] = conv_fwd_operand(raw.w[blk], istd, shift, blk == 0 ? 1.f : 0.25f, g, col);
        else k.w[blk] = ConvOp{u32x4{0u, 0u, 0u, 0u}, u32x4{0u, 0u, 0u, 0u}};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int c = slot_chan(4 * g + r);
            k.gam[blk][r] = (mode == 2 && c >= 0) ? q[2 * F + c] : 0.f;
            k.bet[blk][r] = (mode == 2 && c >= 0) ? q[3 * F + c] : 0.f;
        }
    }
}

}  // namespace

struct MxTrainK {
    const float* prm;
    const float* y;
    float* pred;
    double* cells;
    float* gpart;
    float* xrec[MX_MAX_LAYERS];   // X_l tiles: [ntiles][10][4 N]
    float* qrec[MX_MAX_LAYERS];   // l >= 1: x-hat of BatchNorm 2l-1 where the gradient passes (ReLU gate and dropout), else +inf
    float* hrec[MX_MAX_LAYERS];   // H_l = leaky(theta(A X_l)): [ntiles][10][4 N], written by F_1 (l = 0) / F_{2l} (l >= 1); read by F_{2l+1}
                                  // (l >= 1) and G_{2l+1} instead of X_l and the adjacency, by TOP (l = L - 1) instead of the adjacency,
                                  // by F_{2l+2} and G_{2l} beside them (MXT_H_READERS)
    uint32_t* mrec[MX_MAX_LAYERS];   // dropout masks of layer l, one word per lane and tile (bit 3 s + r = keep of sample s, register r):
                                     // hashed once, by the phase that first applies them (F_{2l+2} / TOP), read by G_{2l+1}
    float* arec;                  // adjacency tiles: [ntiles][4][55]
    float* sb;                    // d(x0 + H): [ntiles][10][4 N]
    float* dx;                    // d X_l: [ntiles][10][4 N]
    float* dtop;                  // d X_L: [ntiles][2][4 N] (value | arg-max channel)
    int64_t B, ntiles, global_batch, sample_offset;
    int N, pcount;
    float dropout_p, drop_scale;
    uint32_t drop_thr;
    float gscale, inv_gscale;
    int do_backward;
};

// The kernels' argument block from the chain's; `samples_per_tile`: 4 (narrow chain) or 1 (wide chain)
inline MxTrainK mxt_kernel_args(const MxTrainArgs& m, int samples_per_tile) {
    MxTrainK k;
    k.prm = m.prm; k.y = m.y; k.pred = m.pred; k.cells = m.cells; k.gpart = m.gpart;
    for (int l = 0; l < MX_MAX_LAYERS; ++l) { k.xrec[l] = m.xrec[l]; k.qrec[l] = m.qrec[l]; k.hrec[l] = m.hrec[l]; k.mrec[l] = m.mrec[l]; }
    k.arec = m.arec; k.sb = m.sb; k.dx = m.dx; k.dtop = m.dtop;
    k.B = m.B; k.ntiles = (m.B + samples_per_tile - 1) / samples_per_tile; k.global_batch = m.global_batch; k.sample_offset = m.sample_offset;
    k.N = m.N; k.pcount = m.pcount;
    k.dropout_p = m.dropout_p; k.drop_scale = m.drop_scale; k.drop_thr = m.drop_thr;
    k.gscale = stgcn_train_mx_grad_scale(m.global_batch);
    k.inv_gscale = 1.0f / k.gscale;
    k.do_backward = m.do_backward;
    return k;
}

// Phase (kind, idx) -> template arguments: launch(kind, idx as std::integral_constant) for F_1 .. F_I and G_0 .. G_I
template <int I, typename LAUNCH>
inline int mxt_dispatch_phase(int kind, int idx, LAUNCH launch) {
    if (idx == I) {
        if (kind == PH_F) {
            if constexpr (I >= 1) return launch(std::integral_constant<int, PH_F>{}, std::integral_constant<int, I>{});
            else return RULGNN_EINVAL;
        }
        if (kind == PH_G) return launch(std::integral_constant<int, PH_G>{}, std::integral_constant<int, I>{});
    }
    if constexpr (I > 0) return mxt_dispatch_phase<I - 1>(kind, idx, launch);
    return RULGNN_EINVAL;
}

}  // namespace rulgnn
