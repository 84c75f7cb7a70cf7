// Train-mode ST_GCN forward + backward on the f16 matrix cores of gfx950 for num_patch <= 15 (the C-MAPSS shapes): the phase chain of
// stgcn_train.hip with every contraction on v_mfma_f32_16x16x32_f16 (2-way split operands, fp32 accumulation: stgcn_mx.hpp) and --
// the point of this file -- with RECOMPUTATION instead of saved activations.
//
// Reference path replaced: ST_GCN.update up to optimizer.step() -- algorithms/algorithms.py:481-488 (model(X) under model.train(),
// MSE, loss.backward()); the layer is models/ST_GCN/Model.py:74-90 (MPNN_mk), :134-170 (TemporalConvNet), :187-195 (SG_TCN).
//
// Why.  The row-mapped chain hands eight [10, N] activation tensors per sample from phase to phase (H, z1, o0, z2 of every layer):
// 26.0 KB of HBM traffic per sample against 1.7 KB of input, 4.2 TB/s of real traffic -- the step was bound by its own saved tensors.
// A layer forward on the matrix cores costs ~10 MFMAs per sample, so here every phase re-derives what it needs from the layer INPUT:
//
//     F_0 (stgcn_forward_mx.hip)  windows -> X_0, adjacency (55 floats), sum z1, sum z1^2 of BatchNorm 0
//     F_{2l+1}                    l = 0: X_0, A -> H_0 (written); l >= 1: H_l -> layer l up to conv_block2 -> sums of BatchNorm 2l+1
//     F_{2l}, l >= 1              X_{l-1}, A -> layer l-1 in full -> X_l (written) -> layer l up to conv_block1, H_l (written) -> sums
//                                 of BatchNorm 2l
//     TOP                         X_{L-1}, H_{L-1} -> layer L-1 from H on, head, loss, head backward -> d X_L as (value, arg-max
//                                 channel), sums of BN 2L-1
//     G_{2l+1}                    H_l, d X_{l+1} -> layer l again from H on, BatchNorm 2l+1 / conv_block2 backward -> d(x0 + H) (written)
//     G_{2l}                      X_l, A, d(x0 + H); l >= 1 (N = 14): H_l -> BatchNorm 2l / conv_block1 / theta backward (X_l and A for
//                                 A X and (A d Hp)^T; H_l, read or rebuilt, as the convolution's operand and for the LeakyReLU gate);
//                                 l >= 1: d X_l (written) and the sums of BatchNorm 2l-1 from the gated x-hat F_{2l} left
// H_l = leaky(theta(A X_l)) is written once per layer by the first phase of this file that computes it (F_1 for l = 0, F_{2l} above) and
// read from its record where that pays (rounds 8 and 18; MXT_H_READERS in stgcn_train_mx_ops.hpp: one switch per reader, with what each
// was measured at -- G_0 and the layer l-1 pass of F_{2l} can read it too and are switched off).
//
// Per sample at 14 x 30, L = 2: 13.5 KB instead of 26.0 KB (round 18's H_0 record and G_2's H tile add 0.9 KB: bytes traded for issue
// slots, the phases' limit).  Between phases only layer inputs, the H records and two gradient tensors cross HBM.
//
// Layout.  The "D layout" of stgcn_forward_mx.hip: one 16x16 tile per sample, column = patch t = lane & 15, row = channel slot
// 4 (lane >> 4) + r; a [10, N] tensor is three registers and four samples are in flight per wavefront.  The backward uses the same
// chains with transposed constant operands:
//     d o0 = W2^T-conv(d z2), d H = W1^T-conv(d z1)    A operand [ci][tap, co], data = [d z | d z of column t + d]         3 MFMAs
//     d X  = A . (d Hp . theta) = ((A d Hp)^T)^T-chain: U = d Hp^T x Adj (2 MFMAs), d X = U x theta (2 MFMAs)
//     d theta[j][k] = sum_c d Hp[c][j] (A X)[c][k]      contraction over channel slots = the packed D registers themselves
//     d W[co][ci, tap] = sum_t d z[co][t] h[ci][t - d tap]: contraction over COLUMNS -- both operands, already packed (hi | lo)
//                                                      pairs, transposed through a per-wavefront LDS image and ds_read_b64_tr_b16
// Weight-gradient accumulators live in MFMA accumulator registers across the persistent tile loop; every wavefront writes one row of
// partial gradients, summed in a fixed order by stgcn_train_finalize_kernel (shared with the fp32 chain, as are prepare and the cells).
//
// f16 range.  Gradients are carried multiplied by S = 2^(ceil(log2 global_batch) + 3) (d pred = 2 diff / B would sit in f16's
// subnormals) and unscaled exactly when rows / sums leave the wavefront.  Activations are not rescaled: statistics of inputs scaled to
// O(1) (every dataset the reference wires) stay far inside the f16 range.  A value that leaves it ends as Inf / NaN in a BatchNorm
// sum, the loss or a gradient row; every TOP / G wavefront checks what it writes and raises the step's status word
// (StepScratch::pad[0]), on which finalize leaves parameters and optimizer state untouched and reports a NaN loss -- the caller
// repeats the step on the exact fp32 chain (RULGNN_STEP_CHAIN; stgcn.py does).
//
// Memory.  Inputs arrive by LDS-DMA one tile ahead (each record is requested again as soon as its last LDS read has retired), outputs
// leave one tile late, right behind the s_waitcnt vmcnt(0) that also counts stores (stgcn_forward_mx.hip, round 3).  The records are
// stored write-through (whole 16-byte pieces out of a staging tile), so a phase ends with no dirty lines in L2 for the next launch to
// wait behind, and a record's last reader in the step loads it non-temporally (MXT_RECORD_POLICY, MXT_LAST_READER_NT).
// A full-tile record is written into its staging tile where its values are produced (branch-free: padding lanes write to a dump area)
// and the tile is the pending storage; the next tile issues the 16-byte LDS reads in front of its wait and the stores back to back
// behind it (round 24; MXT_RECORD_STAGING in stgcn_train_mx_ops.hpp: one switch per piece, profiles/r24_record_stores.md).
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "stgcn_host.hpp"
#include "stgcn_mx.hpp"
#include "stgcn_train_layout.hpp"
#include "stgcn_train_mx.hpp"
#include "stgcn_train_mx_ops.hpp"

namespace rulgnn {

// =====================================================================================================================
// the phase kernel (everything but F_0)
// =====================================================================================================================
// The body of a phase.  PERSIST: the phase runs inside the single small-batch launch (stgcn_train_mx_persist_kernel below): the sums its
// BatchNorm constants come from were completed by the other workgroups of the SAME launch -- it waits for their arrivals (`target` on the
// step's counter) right in front of the cell reads, i.e. behind its first tile's requests and the BatchNorm-independent half of the
// prologue, and reads the cells with agent-scope atomic loads.  Everything else a phase reads was written by the wavefront itself (tile
// t belongs to the same wavefront in every phase of a launch) or by an earlier launch.
// (-DMXP_TRACE: workgroup 0, wavefront 0 stamps the marks below -- in the persistent launch and in the phase kernels alike -- and prints
// them when the launch ends: 100 MHz ticks since the previous mark)
#ifdef MXP_TRACE
__device__ unsigned mxp_ts[128];
__device__ int mxp_n;
__device__ unsigned mxp_id[128];
#define MXP_MARKI(ID) do { if (blockIdx.x == 0 && threadIdx.x == 0 && mxp_n < 128) { mxp_id[mxp_n] = ID; mxp_ts[mxp_n++] = (unsigned)wall_clock64(); } } while (0)
#define MXP_MARK() MXP_MARKI(0)
__device__ __forceinline__ void mxp_dump() {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        for (int i = 0; i < mxp_n; ++i) {
            if (mxp_id[i] >= 100) printf("\nphase %u:", mxp_id[i]);
            else printf(" [%u] +%u", mxp_id[i], mxp_ts[i] - mxp_ts[i - 1]);
        }
        printf("\n");
        mxp_n = 0;
    }
}
#else
#define MXP_MARK() do {} while (0)
#define MXP_MARKI(ID) do {} while (0)
#endif
// LDS of a phase (floats), for the body's carve and the launchers alike.  Workgroup: [BatchNorm table | gradient row image | pair
// partials]; then one region per wavefront (the wavefronts only meet in the prologue and the epilogue).
struct MxtLds {
    int bnc, red, pairbuf, waves;                                       // the workgroup's part; `waves`: the wavefronts' regions
    int zero, scr, dump, sh, wg, X, A, SB, DX, XP, HS, H, wave_floats;  // within a region
    int total;
};
__host__ __device__ constexpr MxtLds mxt_lds(int L, int kind, int idx, int nfix, int N) {
    const MxtTraits t = mxt_traits(L, kind, idx, nfix);
    const int XF = 40 * N;                                   // one [10][4 N] tile
    MxtLds l{};
    l.bnc = 0;                                               // [2L][BN_TABLE_ROWS][F], the rows this phase uses
    l.red = l.bnc + ((2 * L * MXT_BNC * F + 3) & ~3);        // [MXT_RED_FLOATS]
    l.pairbuf = l.red + MXT_RED_FLOATS;                      // [MXT_WAVES][2 F + 1] doubles
    l.waves = l.pairbuf + 2 * MXT_WAVES * (2 * F + 2);
    l.zero = 0;
    l.scr = l.zero + MXT_ZERO_FLOATS;
    l.dump = l.scr;                                          // [MXT_DUMP_FLOATS]: where the padding lanes' staging writes go (TILE_OUT; TOP has none)
    l.sh = l.scr + MXT_SCRATCH_FLOATS;
    l.wg = l.sh + MXT_SHIFT_FLOATS;                          // G: the transposing image of the weight gradient's operands
    l.X = l.wg + (kind == PH_G ? MXT_WG_FLOATS : 0);         // X_LIN, or H_LY (H_IN)
    l.A = l.X + XF;                                          // the adjacency tile, or H_LY (H_TOP)
    l.SB = l.A + (t.H_TOP ? XF : t.AF);                      // G_{2l}
    l.DX = l.SB + (t.NEED_SB ? XF : 0);                      // gradient in (full tile or TOP's two rows)
    l.XP = l.DX + (t.GRAD_IN ? XF : 0);                      // G_{2l}, l >= 1: the gated x-hat of BatchNorm 2l-1
    l.HS = l.XP + (t.BWD_PREV ? XF : 0);                     // the staging tiles (TILE_OUT): one, or one per record (MxtTraits::NSTG)
    l.H = l.HS + t.NSTG * XF;                                // H_TILE: H_{l-1} (F_{2l}) / H_l (G_{2l})
    l.wave_floats = l.H + (t.H_TILE ? XF : 0);
    l.total = l.waves + MXT_WAVES * l.wave_floats;
    return l;
}

template <int L, int KIND, int IDX, int NFIX, bool PERSIST>
__device__ __forceinline__ void mxt_phase_body(const MxTrainK& a, float* smem_all, unsigned target) {
    MXP_MARKI(100 + KIND * 10 + IDX);                                              // phase entry
    const int N = NFIX ? NFIX : a.N;
    const int LS = layer_stride(N);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, col = lane & 15;
    constexpr int NBN = 2 * L;
    constexpr int CS = cell_stride(L);
    constexpr MxtTraits T = mxt_traits(L, KIND, IDX, NFIX);
    constexpr int LY = T.LY, BLK = T.BLK, LIN = T.LIN, AF = T.AF;
    constexpr bool WITH_PREV = T.WITH_PREV, BWD_PREV = T.BWD_PREV, GRAD_IN = T.GRAD_IN, GRAD_TOP = T.GRAD_TOP, NEED_SB = T.NEED_SB;
    constexpr bool H_OUT = T.H_OUT, H_IN = T.H_IN, H_TOP = T.H_TOP, H_PREV = T.H_PREV, H_GE = T.H_GE;
    static_assert(!(KIND == PH_F && IDX == 0), "F_0 is stgcn_train_f0_mx_kernel");

    // ---- LDS carve (mxt_lds) -----------------------------------------------------------------------------------------------
    const int XF = 40 * N;                                   // one [10][4 N] tile
    constexpr MxtLds LC = mxt_lds(L, KIND, IDX, NFIX, NFIX);      // the workgroup's part and the offsets up to X do not depend on N
    const MxtLds ld = mxt_lds(L, KIND, IDX, NFIX, N);
    float* const bnc = smem_all + LC.bnc;
    float* const red = smem_all + LC.red;
    double* const pairbuf = reinterpret_cast<double*>(smem_all + LC.pairbuf);
    const int off_zero = LC.zero, off_scr = LC.scr, off_sh = LC.sh, off_wg = LC.wg, off_X = LC.X;
    const int off_A = ld.A, off_SB = ld.SB, off_DX = ld.DX, off_XP = ld.XP, off_HS = ld.HS, off_H = ld.H;
    float* const smem = smem_all + LC.waves + wave * ld.wave_floats;
    u32x2* const sh_tile = reinterpret_cast<u32x2*>(smem + off_sh);
    u32x2* const wg_img = reinterpret_cast<u32x2*>(smem + off_wg);

    int64_t tile = (int64_t)blockIdx.x * MXT_WAVES + wave;
    const int64_t tstride = (int64_t)gridDim.x * MXT_WAVES;

    // ---- requests --------------------------------------------------------------------------------------------------------
    // (`LAST_`: this phase is the record's last reader in the step -- MXT_LAST_READER_NT)
    auto dma = [&](const float* src, int off, int bytes, auto LAST_) {
        constexpr bool NT = decltype(LAST_)::value && MXT_LAST_READER_NT;
        if constexpr (NFIX != 0) {
            if (bytes == 160 * NFIX) { dma_tile_fixed<160 * NFIX, NT>(src, smem + off, lane); return; }
            if (bytes == 32 * NFIX) { dma_tile_fixed<32 * NFIX, NT>(src, smem + off, lane); return; }
        }
        if constexpr (AF != 0) {
            if (bytes == 4 * AF) { dma_tile_fixed<4 * AF, NT>(src, smem + off, lane); return; }
        }
        dma_tile<NT>(src, smem + off, bytes, lane);
    };
    constexpr std::true_type LAST{};
    // H_l dies with G_{2l} where that phase reads it, else with G_{2l+1}; X_l dies with G_{2l}, the adjacency with G_0; the gradient
    // tensors and Q_l have one reader each
    constexpr std::bool_constant<KIND == PH_G && (BLK == 0 || !mxt_g_even_reads_h(LY, NFIX))> LAST_H{};
    constexpr std::bool_constant<KIND == PH_G && BLK == 0> LAST_X{};
    constexpr std::bool_constant<KIND == PH_G && IDX == 0> LAST_A{};
    auto req_XA = [&](int64_t t) {
        if constexpr (H_IN) {
            dma(a.hrec[LY] + t * XF, off_X, 4 * XF, LAST_H);
        } else if constexpr (H_TOP) {
            dma(a.xrec[LIN] + t * XF, off_X, 4 * XF, std::false_type{});
            dma(a.hrec[LY] + t * XF, off_A, 4 * XF, std::false_type{});
        } else {
            dma(a.xrec[LIN] + t * XF, off_X, 4 * XF, LAST_X);
            dma(a.arec + t * AF, off_A, 4 * AF, LAST_A);
            if constexpr (H_PREV) dma(a.hrec[LIN] + t * XF, off_H, 4 * XF, std::false_type{});
        }
    };
    // G_{2l}: each half tile reads its two samples of H_l from the tile when it starts, and the tile is requested again behind the
    // second half's read -- half a tile later than the other inputs.  (All four samples in registers from the top of the tile, the
    // request with X_l's: G_2 spills 28 bytes instead of 16 and the step is SLOWER than with the rebuild -- profiles/r18_h_records.md)
    auto req_H = [&](int64_t t) { if constexpr (H_GE) dma(a.hrec[LY] + t * XF, off_H, 4 * XF, LAST_H); };
    auto req_SB = [&](int64_t t) { if constexpr (NEED_SB) dma(a.sb + t * XF, off_SB, 4 * XF, LAST); };
    auto req_DX = [&](int64_t t) {
        if constexpr (GRAD_TOP) dma(a.dtop + t * (8 * N), off_DX, 32 * N, LAST);
        else if constexpr (GRAD_IN) dma(a.dx + t * XF, off_DX, 4 * XF, LAST);
    };
    auto req_XP = [&](int64_t t) { if constexpr (BWD_PREV) dma(a.qrec[LY] + t * XF, off_XP, 4 * XF, LAST); };

    // ---- prologue.  The loads go out in three bursts, in the order their consumers need them -- the vector memory counter retires in
    // issue order, so a wait for one burst is a wait for every burst in front of it: (1) the reduction cells, the BatchNorm count and
    // gamma / beta of this wavefront's pair (one pair per wavefront, stgcn_train_layout.hpp); (2) the parameter gathers of the operands
    // (theta, the convolutions, the transposed forms, TOP's head) and the dropout keys; (3) the first tile.  The BatchNorm table then waits
    // for burst 1 alone; the operands that fold a BatchNorm in are built behind it --------------------------------------------------------
    // the reduction pairs this phase's BatchNorm constants come from, one per wavefront: the forward pairs of the layers it runs
    // (F_{2l+1}: 2l; F_{2l}, l >= 1: 2l-2, 2l-1; TOP, G_{2l+1}: 2l, 2l+1; G_{2l}: 2l) and the backward pair of BatchNorm IDX (G)
    constexpr int FW0 = WITH_PREV ? 2 * LY - 2 : 2 * LY;                           // first forward pair
    constexpr int NFW = (KIND == PH_F && BLK == 1) || (KIND == PH_G && BLK == 0) ? 1 : 2;
    static_assert(NFW + (KIND == PH_G ? 1 : 0) <= MXT_WAVES, "one reduction pair per wavefront");
    const bool bn_fwd = wave < NFW, bn_mine = bn_fwd || (KIND == PH_G && wave == NFW);
    const int bn_b = bn_fwd ? FW0 + wave : IDX;
    BnPairRaw bnraw;
    // (PERSIST: the cells are complete only once the step's counter says so -- loaded behind the wait below)
    if (!PERSIST && bn_mine) bn_pair_load<false>(bnraw, a.cells, a.prm, L, N, bn_fwd, bn_b, lane);
    __builtin_amdgcn_sched_barrier(0);
    for (int i = lane; i < MXT_ZERO_FLOATS; i += 64) smem[off_zero + i] = 0.f;
    if (lane < 2) sh_tile[64 + 65 * lane] = u32x2{0u, 0u};
    if constexpr (KIND == PH_G) {
        if (lane < 2) wg_img[WG_H_HI + WG_ZERO + (WG_H_LO - WG_H_HI) * lane] = u32x2{0u, 0u};      // the causal zeros of the shifted read
    }
    // which convolutions of the main layer / the previous layer this phase runs, and how
    constexpr int M0_LY = (KIND == PH_F && BLK == 0) ? 1 : 2;                          // conv_block1 of layer LY
    constexpr int M1_LY = (KIND == PH_F && BLK == 0) ? 0 : ((KIND == PH_F) ? 1 : ((KIND == PH_G && BLK == 0) ? 0 : 2));   // conv_block2
    MXP_MARKI(1);
    LayerRaw rc, rp;
    layer_raw(rc, a.prm, LY, N, g, col, M0_LY, M1_LY, !(H_IN || H_TOP || H_GE));
    if constexpr (WITH_PREV) layer_raw(rp, a.prm, LY - 1, N, g, col, 2, 2, !H_PREV);
    ConvOp wT = ConvOp{u32x4{0u, 0u, 0u, 0u}, u32x4{0u, 0u, 0u, 0u}};
    ThetaOp thN = ThetaOp{u32x4{0u, 0u, 0u, 0u}, u32x4{0u, 0u, 0u, 0u}};
    ConvRaw wT_raw = ConvRaw{{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};          // (converted behind the BatchNorm cells' loads: one round trip)
    ThetaRaw thN_raw = ThetaRaw{{0.f, 0.f, 0.f, 0.f}};
    if constexpr (KIND == PH_G) {
        wT_raw = conv_bwd_raw(a.prm + LY * LS + off_conv_w(N, BLK), g, col);
        if constexpr (BLK == 0 && LY >= 1) thN_raw = theta_n_raw(a.prm + LY * LS, N, g, col);
    }
    // head (TOP), row mapping: lane (sample row, t) holds row t and column t of fc1
    float fc1w[16], fc1wT[16];
    float fc1b = 0.f, fc2w = 0.f, fc2b = 0.f;
    if constexpr (KIND == PH_TOP) {
        const int colc = col < N ? col : 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int kc2 = k < N ? k : 0;
            const float v = a.prm[off_fc1_w(N, L) + colc * N + kc2], vt = a.prm[off_fc1_w(N, L) + kc2 * N + colc];
            fc1w[k] = (col < N && k < N) ? v : 0.f;
            fc1wT[k] = (col < N && k < N) ? vt : 0.f;
        }
        const float b1 = a.prm[off_fc1_b(N, L) + colc], w2 = a.prm[off_fc2_w(N, L) + colc];
        fc1b = col < N ? b1 : 0.f;
        fc2w = col < N ? w2 : 0.f;
        fc2b = a.prm[off_fc2_b(N, L)];
    }
    uint32_t dkey[L];
#pragma unroll
    for (int l = 0; l < L; ++l) dkey[l] = step_scratch(a.cells, L)->drop_key[l];
    const bool use_drop = a.dropout_p > 0.f;
    uint32_t mask_next = 0u;                    // G_{2l+1}: the dropout mask of the tile in hand, read one tile ahead
    constexpr bool MASK_IN = KIND == PH_G && BLK == 1;
    if constexpr (MASK_IN) {
        if (use_drop && tile < a.ntiles) mask_next = a.mrec[LY][tile * 64 + lane];
    }
    __builtin_amdgcn_sched_barrier(0);
    if (tile < a.ntiles) { req_XA(tile); req_H(tile); req_SB(tile); req_DX(tile); req_XP(tile); }
    {
        MXP_MARKI(2);                                                              // independent prologue done
        if constexpr (PERSIST) {
            if (threadIdx.x == 0) {
                unsigned* const ctr = step_barrier(a.cells, L);
                // (a workgroup that never arrives -- a grid that is not co-resident -- must not hang the GPU: after ~2^22 polls, seconds,
                // the step is rejected like a guard trip)
                unsigned spins = 0;
                while (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
                    __builtin_amdgcn_s_sleep(1);
                    if (++spins > (1u << 22)) { atomicOr(&step_scratch(a.cells, L)->pad[0], 4u); break; }
                }
            }
            __syncthreads();
        }
        constexpr bool COH = PERSIST;
        MXP_MARKI(3);                                                              // barrier passed
        if (bn_mine) {
            if constexpr (PERSIST) bn_pair_load<COH>(bnraw, a.cells, a.prm, L, N, bn_fwd, bn_b, lane);
            bn_pair_finish(bnraw, bnc, bn_fwd, bn_b, lane);
        }
        if constexpr (KIND == PH_G) {
            wT = conv_bwd_pack(wT_raw);
            if constexpr (BLK == 0 && LY >= 1) thN = theta_pack(thN_raw);
        }
        __syncthreads();
    }
    MXP_MARKI(4);                                                                  // BatchNorm table in LDS
    LayerK kc;                                   // layer LY
    layer_constants(kc, rc, bnc, LY, g, col, M0_LY, M1_LY);
    LayerK kp;                                   // layer LY - 1 (F_{2l}, l >= 1)
    if constexpr (WITH_PREV) layer_constants(kp, rp, bnc, LY - 1, g, col, 2, 2);
    float bA[3] = {0.f, 0.f, 0.f}, bk1[3] = {0.f, 0.f, 0.f}, bk2[3] = {0.f, 0.f, 0.f};     // BatchNorm IDX backward: gamma istd, S mean(dy), S mean(dy xhat)
    if constexpr (KIND == PH_G) {
        const float* q = bnc + IDX * MXT_BNC * F;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int c = slot_chan(4 * g + r);
            bA[r] = c >= 0 ? q[4 * F + c] : 0.f;
            bk1[r] = c >= 0 ? q[5 * F + c] * a.gscale : 0.f;      // carried x S like the gradients
            bk2[r] = c >= 0 ? q[6 * F + c] * a.gscale : 0.f;
        }
    }

    // ---- per-lane addressing ---------------------------------------------------------------------------------------------------
    const bool col_ok = col < N;
    const float colm = col_ok ? 1.f : 0.f;
    const int pitch = 4 * N;
    int xoff[3], aoff[3], chan[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int c = slot_chan(4 * g + r);
        chan[r] = c;
        xoff[r] = (c >= 0 && col_ok) ? c * pitch + col : -1;      // inside a [10][4 N] tile; -1: padding -> the zero words
    }
    {
        const int cc = slot_chan(col);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int c = slot_chan(4 * g + r);
            aoff[r] = (c >= 0 && cc >= 0) ? sym(c, cc) : -1;
        }
    }
    auto ld_tile = [&](int base, float (&v)[4][3]) {
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int r = 0; r < 3; ++r) v[s][r] = smem[(xoff[r] >= 0 ? base + xoff[r] : off_zero) + s * N];
    };
    // A full-tile record leaves through LDS: the tile is assembled in the wavefront's staging words and stored as 16-byte pieces of the
    // contiguous [10][4 N] record -- three dwordx4 stores of whole cache lines instead of twelve dword stores of 4 N-byte row pieces.
    // All four samples go out: beyond the batch a record is never used (every reader overwrites the samples >= ns of what it loads).
    // The three pieces of that path have a switch each (MXT_RECORD_STAGING, stgcn_train_mx_ops.hpp).
    // Staging writes.  `swr[r]`: where register row r of sample 0 goes in staging tile 0 -- the lane's word of the tile, or (branch-free
    // form) for a padding lane its word of the dump area; sample s is s N words on (an immediate offset at fixed N), staging tile k
    // another k XF for the lanes inside the tile (the dump area lies in front of the tiles).
    static_assert(!T.TILE_OUT || (KIND != PH_TOP && LC.dump >= LC.scr && LC.dump + MXT_DUMP_FLOATS <= LC.sh),
                  "the dump area lies inside the wavefront's region, in words no tile-writing phase uses");
    int swr[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) swr[r] = xoff[r] >= 0 ? off_HS + xoff[r] : LC.dump + lane;
    auto stg_put = [&](int k, int s, int r, float v) {
        if constexpr (MXT_STAGE_BRANCHFREE) {
            const int w = k == 0 ? swr[r] : (swr[r] >= off_HS ? swr[r] + k * XF : swr[r]);
            smem[w + s * N] = v;
        } else {
            if (xoff[r] >= 0) smem[off_HS + k * XF + xoff[r] + s * N] = v;
        }
    };
    auto stg_put_tile = [&](int k, const float (&v)[4][3]) {
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int r = 0; r < 3; ++r) stg_put(k, s, r, v[s][r]);
    };
    // Staging tile k -> its record, 16-byte pieces.  Rolled: one LDS round trip per piece (the store's asm is a memory barrier for the
    // compiler).  Read-ahead form: stg_read issues every read (MXT_MAX_PIECES per lane; at fixed N the count is known: three at N = 14, the
    // last on twelve lanes), stg_store the stores back to back; the caller puts the tile's wait between them.
    struct StgPieces { float4 q[MXT_MAX_PIECES]; };
    const int nq = XF / 4;
    auto stg_read = [&](int k, StgPieces& p) {
        const float4* const stg = reinterpret_cast<const float4*>(smem + off_HS + k * XF);
#pragma unroll
        for (int j = 0; j < MXT_MAX_PIECES; ++j) {
            const int i = lane + 64 * j;
            p.q[j] = stg[i < nq ? i : 0];
        }
    };
    auto stg_store = [&](float* dst, const StgPieces& p) {
#pragma unroll
        for (int j = 0; j < MXT_MAX_PIECES; ++j) {
            const int i = lane + 64 * j;
            if (i < nq) st_rec16<MXT_RECORD_POLICY>(dst + 4 * i, p.q[j]);
        }
    };
    auto stg_drain_rolled = [&](int k, float* dst) {
        const float* const stg = smem + off_HS + k * XF;
        for (int i = lane; i < nq; i += 64) st_rec16<MXT_RECORD_POLICY>(dst + 4 * i, reinterpret_cast<const float4*>(stg)[i]);
    };
    // (not staged where produced: registers -> the one staging tile -> record, at the top of the next tile)
    auto st_tile = [&](float* dst, const float (&v)[4][3]) {
        stg_put_tile(0, v);
        __builtin_amdgcn_wave_barrier();
        stg_drain_rolled(0, dst);
        __builtin_amdgcn_wave_barrier();
    };
    const int sh_rd1 = col >= 1 ? lane - 1 : 64, sh_rd2 = col >= 2 ? lane - 2 : 64;     // forward taps: column t - d
    int sh_rd1_lo = sh_rd1 + 65, sh_rd2_lo = sh_rd2 + 65;
    const int sh_bk = col + (BLK == 0 ? 1 : 2) < 16 ? lane + (BLK == 0 ? 1 : 2) : 64;   // transposed convolution of this phase: column t + d
    int sh_bk_lo = sh_bk + 65;
    asm volatile("" : "+v"(sh_rd1_lo), "+v"(sh_rd2_lo), "+v"(sh_bk_lo));
    // weight-gradient image (wg_chunk): this lane writes the pairs of its column t = col, slots 4 g .. 4 g + 3; the transposed read hands
    // lane (g', slot) the columns 4 g' .. 4 g' + 3, for which lane 4 q + p of the group addresses row 4 g' + q, slots 4 p .. 4 p + 3; the
    // tap at t - d reads d rows higher, rows above the first from the zero chunk
    const int wg_wr = wg_chunk(col, g);
    const int wg_row = 4 * g + (col >> 2), wg_rows = wg_row - (BLK == 0 ? 1 : 2);
    const int wg_rd = wg_chunk(wg_row, col & 3);
    const int wg_rds = wg_rows >= 0 ? wg_chunk(wg_rows, col & 3) : WG_ZERO;
    const unsigned t_bias = g == 3 ? 0x3C00u << 16 : 0u;
    uint32_t dro[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) dro[r] = (uint32_t)((chan[r] >= 0 ? chan[r] : 0) * N + col);

    // ---- persistent accumulators ---------------------------------------------------------------------------------------------------
    float s_a[3] = {0.f, 0.f, 0.f}, s_b[3] = {0.f, 0.f, 0.f};      // BatchNorm reduction pair of this lane's channels
    f32x4 acc_w0 = {0.f, 0.f, 0.f, 0.f}, acc_w1 = {0.f, 0.f, 0.f, 0.f};      // conv weight gradient: tap at t / tap at t - d
    f32x4 acc_th = {0.f, 0.f, 0.f, 0.f};                                   // theta / fc1 weight gradient
    float acc_b = 0.f, acc_w2 = 0.f, acc_b2 = 0.f, acc_loss = 0.f;
    const float inv_gb = 1.0f / (float)a.global_batch;

    // ---- building blocks of a tile ------------------------------------------------------------------------------------------------------
    // T = (A X)^T, Hp' = (1 + a)/2 (theta (A X) + b), H = leaky(Hp)
    // (generic in the number of samples in flight: four in the forward phases, two per half tile in the backward phases, whose working set
    // does not fit 256 registers at four)
    auto stage_T = [&](const auto& X, const auto& adjB, auto& T, auto& xo) {
        constexpr int NS = std::extent_v<std::remove_reference_t<decltype(T)>>;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const Split2 p01 = split2(X[s][0], X[s][1]), p2 = split2(X[s][2], 0.f);
            const Op2 o = {u32x4{p01.hi, p2.hi, p01.hi, p2.hi}, u32x4{p01.lo, p2.lo, p01.lo, p2.lo}};
            xo[s] = o;
            T[s] = mfma16z(o.h, adjB[s]);
            T[s] = mfma16(o.l, adjB[s], T[s]);
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    auto stage_Hp = [&](const auto& T, const ThetaOp& th, auto& Hp) {
        constexpr int NS = std::extent_v<std::remove_reference_t<decltype(Hp)>>;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const Split2 p01 = split2(T[s][0], T[s][1]), p23 = split2(T[s][2], T[s][3]);
            const u32x4 ta = {p01.hi, p23.hi | t_bias, p01.lo, p23.lo};
            Hp[s] = mfma16z(ta, th.hi);
            Hp[s] = mfma16(ta, th.lo, Hp[s]);
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    // z = W x [D ; D of column t - d] (+ shift x partner); keeps the packed operand halves of D and of the shifted column
    auto stage_conv = [&](const auto& D, float partner, const ConvOp& w, int rd, int rd_lo, auto& z, auto& keep, auto& keep_sh) {
        constexpr int NS = std::extent_v<std::remove_reference_t<decltype(z)>>;
        u32x4 bh[NS], bl[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const Pk p = pack3(D[s][0], D[s][1], D[s][2], partner);
            const Shifted prev = shift_read(sh_tile, rd, rd_lo, lane, p);
            bh[s] = cat(p.hi, prev.hi);
            bl[s] = cat(p.lo, prev.lo);
            keep[s] = p;
            keep_sh[s] = prev;
            __builtin_amdgcn_sched_barrier(0);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            z[s] = mfma16z(w.hi, bh[s]);
            z[s] = mfma16(w.hi, bl[s], z[s]);
            z[s] = mfma16(w.lo, bh[s], z[s]);
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    auto leaky_of = [&](const auto& Hp, auto& H) {
        constexpr int NS = std::extent_v<std::remove_reference_t<decltype(H)>>;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            keep_until_here(Hp[s][3]);
#pragma unroll
            for (int r = 0; r < 3; ++r) H[s][r] = fmaf((1.f - LEAKY) / (1.f + LEAKY), __builtin_fabsf(Hp[s][r]), Hp[s][r]);
        }
    };
    // One layer in full (both BatchNorms known): X <- dropout(relu(BN(z2)) + o0) + X.  `sbase[s]`: dropout counter of (sample s, channel 0, patch 0).
    // (`h_in`: H of the layer from its record -- no T, Hp)
    auto layer_full = [&](float (&X)[4][3], const u32x4 (&adjB)[4], const LayerK& k, uint32_t key, const uint32_t (&sbase)[4],
                          float (*xh1_out)[4][3], float (*y2_out)[4][3], float (*q_out)[4][3], uint32_t* mbits_out,
                          const float (*h_in)[4][3] = nullptr) {
        f32x4 z[4];
        float H[4][3], V[4][3];
        Pk pk[4];
        Shifted ps[4];
        if (h_in) {
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int r = 0; r < 3; ++r) H[s][r] = (*h_in)[s][r];
        } else {
            f32x4 T[4], Hp[4];
            Op2 xo[4];
            stage_T(X, adjB, T, xo);
            stage_Hp(T, k.th, Hp);
            leaky_of(Hp, H);
        }
        stage_conv(H, 1.0f, k.w[0], sh_rd1, sh_rd1_lo, z, pk, ps);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            keep_until_here(z[s][3]);
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const float y1 = fmaf(k.gam[0][r], z[s][r], k.bet[0][r]);
                V[s][r] = relu2(fmaf(2.f, H[s][r], relu2(y1)));                  // 4 o0
            }
        }
        stage_conv(V, 1.0f, k.w[1], sh_rd2, sh_rd2_lo, z, pk, ps);
        uint32_t mbits = 0u;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            keep_until_here(z[s][3]);
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const float xh = z[s][r];
                const float y2 = fmaf(k.gam[1][r], xh, k.bet[1][r]);
                if (xh1_out) (*xh1_out)[s][r] = xh;
                if (y2_out) (*y2_out)[s][r] = y2;
                float o1 = fmaf(0.5f, relu2(y2), 0.25f * V[s][r]);               // relu(BN(z2)) + o0, both >= 0
                bool keep = true;
                if (use_drop) {
                    const uint32_t h = lowbias32((sbase[s] + dro[r]) ^ key);
                    keep = h >= a.drop_thr;
                    o1 = keep ? o1 * a.drop_scale : 0.f;
                    mbits |= keep ? 1u << (3 * s + r) : 0u;
                }
                // what the backward sums of this BatchNorm need: x-hat where the gradient passes the ReLU and the dropout, else +inf
                if (q_out) (*q_out)[s][r] = (keep && y2 > 0.f) ? xh : INFINITY;
                X[s][r] = fmaf(colm, o1, X[s][r]);
            }
        }
        *mbits_out = mbits;
    };

    bool pend = false;
    int64_t pend_tile = 0;
    int pend_ns = 0;
    float pend_v[4][3], pend_q[4][3], pend_h[4][3];     // (staged where produced: unused, the staging tiles hold the records)
    float pend_top0 = 0.f, pend_top1 = 0.f, pend_pred = 0.f;
    uint32_t pend_m = 0u;                       // dropout mask bits of the tile (F_{2l}, TOP: written)
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int r = 0; r < 3; ++r) pend_v[s][r] = pend_q[s][r] = pend_h[s][r] = 0.f;
    // The full-tile records of this phase, in the order they leave; REC k lives in pend_v / pend_q / pend_h or in staging tile k.
    // (F_{2l}: X_l, Q_l, H_l; F_1: H_0; G_{2l+1}: d(x0 + H); G_{2l}: d X_l)
    constexpr int NREC = WITH_PREV ? 3 : (T.TILE_OUT ? 1 : 0);
    constexpr int REC_H = WITH_PREV ? 2 : 0;    // H_OUT: which record H_l is
    auto rec_dst = [&](int k) -> float* {
        if constexpr (WITH_PREV) return (k == 0 ? a.xrec[LY] : k == 1 ? a.qrec[LY] : a.hrec[LY]) + pend_tile * XF;
        else if constexpr (H_OUT) return a.hrec[LY] + pend_tile * XF;
        else if constexpr (KIND == PH_G && BLK == 1) return a.sb + pend_tile * XF;
        else return a.dx + pend_tile * XF;
    };
    // a value of record k as it is produced (k: 0 -> pend_v, 1 -> pend_q, 2 -> pend_h where the registers are the pending storage)
    auto rec_put = [&](int k, int s, int r, float v) {
        if constexpr (MXT_STAGE_EARLY) stg_put(k, s, r, v);
        else (k == 0 ? pend_v : k == 1 ? pend_q : pend_h)[s][r] = v;
    };
    // the pending records' way out.  Staged where produced: `rec_read` in front of the tile's wait (read-ahead) or nothing, `rec_store`
    // behind it; the epilogue runs both.
    // (`pieces`: a local of the tile body -- declared outside the loop the twelve registers per record are carried around the back edge)
    // (G_{2l}, l >= 1, sits at 256 registers: with the pieces held across the wait it spills more than its parent, so it keeps the
    // rolled drain behind the wait; so does the generic-N single launch, one register allocation for eight bodies)
    constexpr bool READ_AHEAD = MXT_STAGE_READ_AHEAD && !BWD_PREV && !(PERSIST && NFIX == 0);
    using RecPieces = StgPieces[NREC > 0 ? NREC : 1];
    auto rec_read = [&](RecPieces& pieces) {
        if constexpr (READ_AHEAD) {
            asm volatile("" ::: "memory");
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int k = 0; k < NREC; ++k) stg_read(k, pieces[k]);
        }
    };
    auto rec_store = [&](const RecPieces& pieces) {
        if constexpr (READ_AHEAD) {
#pragma unroll
            for (int k = 0; k < NREC; ++k) stg_store(rec_dst(k), pieces[k]);
        } else if constexpr (MXT_STAGE_EARLY) {
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int k = 0; k < NREC; ++k) stg_drain_rolled(k, rec_dst(k));
            __builtin_amdgcn_wave_barrier();
        } else {
            if constexpr (WITH_PREV) {
                st_tile(rec_dst(0), pend_v);
                st_tile(rec_dst(1), pend_q);
                st_tile(rec_dst(2), pend_h);
            } else if constexpr (NREC == 1) {
                st_tile(rec_dst(0), pend_v);
            }
        }
    };

    MXP_MARKI(5);                                                                  // constants ready
    for (; tile < a.ntiles; tile += tstride) {
        const int64_t s0 = tile * 4;
        const int ns_tile = (int)((a.B - s0) < 4 ? (a.B - s0) : 4);
        // Two instantiations of the tile body: every tile but (at most) the last one is FULL -- there `ns` is the constant 4 and the
        // per-sample guards of the partial tile (selects on every gradient element, scalar branches around the sums) compile away.
        auto tile_body = [&](auto FULL_) {
        constexpr bool FULL = decltype(FULL_)::value;
        const int ns = FULL ? 4 : ns_tile;
        const int64_t nt = tile + tstride;
        // (read-ahead: the pending records' LDS reads go first -- their latency sits under the wait the tile pays anyway)
        RecPieces pieces;
        if constexpr (NREC > 0) { if (pend) rec_read(pieces); }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
        if (!pend) MXP_MARKI(13);                                                  // the first tile in hand
        // ---- what the previous tile leaves: stored HERE, behind the wait that also counts stores ------------------------------------
        if (pend) {
            if constexpr (NREC > 0) rec_store(pieces);
            if constexpr (WITH_PREV) {
                if (use_drop) st_rec4<MXT_RECORD_POLICY>(a.mrec[LY - 1] + pend_tile * 64 + lane, pend_m);
            }
            if constexpr (KIND == PH_TOP) {
                if (g < pend_ns && col_ok && a.do_backward) {
                    float* p = a.dtop + pend_tile * (8 * N) + g * N + col;
                    st_rec4<MXT_RECORD_POLICY>(p, pend_top0);
                    st_rec4<MXT_RECORD_POLICY>(p + pitch, pend_top1);
                }
                if (g < pend_ns && col == 0) st_rec4<MXT_RECORD_POLICY>(a.pred + pend_tile * 4 + g, pend_pred);
                if (use_drop && a.do_backward) st_rec4<MXT_RECORD_POLICY>(a.mrec[LY] + pend_tile * 64 + lane, pend_m);
            }
        }
        // ---- inputs ------------------------------------------------------------------------------------------------------------------
        float X[4][3];                          // X_LIN; H_IN: H_LY
        float HT[4][3];                         // H_TOP: H_LY; H_PREV: H_LIN
        u32x4 adjB[4];
        ld_tile(off_X, X);
        if constexpr (H_TOP) ld_tile(off_A, HT);
        if constexpr (H_PREV) {
            ld_tile(off_H, HT);
            if (ns < 4) {                       // beyond the batch the record holds whatever an earlier step left
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    if (s >= ns) HT[s][0] = HT[s][1] = HT[s][2] = 0.f;
            }
        }
        if constexpr (H_IN || H_TOP) {
            if (ns < 4) {                       // the record holds whatever an earlier step left beyond the batch
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    if (s >= ns) {
                        X[s][0] = X[s][1] = X[s][2] = 0.f;
                        if constexpr (H_TOP) HT[s][0] = HT[s][1] = HT[s][2] = 0.f;
                    }
            }
        } else {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                // F_0 left every entry as its (hi | lo << 16) f16 pair: the operand is four byte permutes, no split (slot 3 of every
                // lane group is padding: always zero)
                unsigned q[3];
#pragma unroll
                for (int r = 0; r < 3; ++r) q[r] = __builtin_bit_cast(unsigned, smem[(aoff[r] >= 0 ? off_A + aoff[r] : off_zero) + s * 55]);
                adjB[s] = u32x4{__builtin_amdgcn_perm(q[1], q[0], 0x05040100u), q[2] & 0xFFFFu, __builtin_amdgcn_perm(q[1], q[0], 0x07060302u), q[2] >> 16};
            }
            if (ns < 4) {                       // samples beyond the batch (last tile): whatever the workspace holds there must not reach an accumulator
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    if (s >= ns) { adjB[s] = u32x4{0u, 0u, 0u, 0u}; X[s][0] = X[s][1] = X[s][2] = 0.f; }
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
        if (nt < a.ntiles) req_XA(nt);
        uint32_t sbase[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) sbase[s] = (uint32_t)((a.sample_offset + s0 + s) * F) * (uint32_t)N;
        const bool any_row = true;
        (void)any_row;

        if constexpr (KIND == PH_F) {
            // ===== forward statistics phases ==============================================================================================
            if constexpr (WITH_PREV) {
                float Qn[4][3];
                if constexpr (H_PREV) layer_full(X, adjB, kp, dkey[LY - 1], sbase, nullptr, nullptr, &Qn, &pend_m, &HT);
                else layer_full(X, adjB, kp, dkey[LY - 1], sbase, nullptr, nullptr, &Qn, &pend_m);
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int r = 0; r < 3; ++r) { rec_put(0, s, r, X[s][r]); rec_put(1, s, r, Qn[s][r]); }
            }
            f32x4 z[4];
            float H[4][3];
            Pk pk[4];
            Shifted ps[4];
            if constexpr (H_IN) {
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int r = 0; r < 3; ++r) H[s][r] = X[s][r];
            } else {
                f32x4 T[4], Hp[4];
                Op2 xo[4];
                stage_T(X, adjB, T, xo);
                stage_Hp(T, kc.th, Hp);
                leaky_of(Hp, H);
            }
            if constexpr (H_OUT) {
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int r = 0; r < 3; ++r) rec_put(REC_H, s, r, H[s][r]);
            }
            if constexpr (BLK == 0) {
                stage_conv(H, 0.f, kc.w[0], sh_rd1, sh_rd1_lo, z, pk, ps);          // raw z1
            } else {
                stage_conv(H, 1.0f, kc.w[0], sh_rd1, sh_rd1_lo, z, pk, ps);         // x-hat of BatchNorm 2l
                float V[4][3];
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    keep_until_here(z[s][3]);
#pragma unroll
                    for (int r = 0; r < 3; ++r) V[s][r] = relu2(fmaf(2.f, H[s][r], relu2(fmaf(kc.gam[0][r], z[s][r], kc.bet[0][r]))));
                }
                stage_conv(V, 0.f, kc.w[1], sh_rd2, sh_rd2_lo, z, pk, ps);          // raw z2
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                keep_until_here(z[s][3]);
                if (s < ns) {
#pragma unroll
                    for (int r = 0; r < 3; ++r) {
                        const float zv = z[s][r] * colm;
                        s_a[r] += zv;
                        s_b[r] = fmaf(zv, zv, s_b[r]);
                    }
                }
            }
            if constexpr (H_OUT) { pend = true; pend_tile = tile; pend_ns = ns; }
            return;
        }

        if constexpr (KIND == PH_TOP) {
            // ===== last layer, head, loss, head backward ===================================================================================
            float xh1[4][3], y2[4][3];
            // (this row's label, requested before the last layer's forward: read where it is used -- `if (rowok) ... a.y[s0 + g]`, a load
            // under a condition -- it was a memory round trip per tile in the middle of the kernel)
            const float ylab = a.y[s0 + (g < ns ? g : ns - 1)];
            if constexpr (H_TOP) layer_full(X, adjB, kc, dkey[LY], sbase, &xh1, &y2, nullptr, &pend_m, &HT);
            else layer_full(X, adjB, kc, dkey[LY], sbase, &xh1, &y2, nullptr, &pend_m);
            // max over the ten channels with its arg-max: per lane over its (up to three) channels, then across the four lane groups
            float pm[4], pa[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const float v0 = X[s][0], v1 = g == 3 ? X[s][0] : X[s][1], v2 = g == 3 ? X[s][0] : X[s][2];
                float m = v0;
                int ar = 0;
                if (v1 > m) { m = v1; ar = 1; }
                if (v2 > m) { m = v2; ar = 2; }
                pm[s] = fmaf(v0 + v1 + v2, 0.f, m);                      // NaN / Inf stay
                pa[s] = __builtin_bit_cast(float, 3 * g + ar);            // channel of slot 4 g + ar
            }
            transpose_rows4(pm[0], pm[1], pm[2], pm[3]);                  // out: register = lane group, row = sample
            transpose_rows4(pa[0], pa[1], pa[2], pa[3]);
            float pooled = pm[0];
            int arg = __builtin_bit_cast(int, pa[0]);
#pragma unroll
            for (int q = 1; q < 4; ++q) {
                const bool take = pm[q] > pooled;
                pooled = take ? pm[q] : pooled;
                arg = take ? __builtin_bit_cast(int, pa[q]) : arg;
            }
            pooled = fmaf((pm[0] + pm[1]) + (pm[2] + pm[3]), 0.f, pooled);
            const bool rowok = g < ns, valid = rowok && col_ok;
            pooled = valid ? pooled : 0.f;
            float y1 = fc1b;
            fmac1_rowbcast<0>(y1, pooled, fc1w[0]);   fmac1_rowbcast<1>(y1, pooled, fc1w[1]);   fmac1_rowbcast<2>(y1, pooled, fc1w[2]);
            fmac1_rowbcast<3>(y1, pooled, fc1w[3]);   fmac1_rowbcast<4>(y1, pooled, fc1w[4]);   fmac1_rowbcast<5>(y1, pooled, fc1w[5]);
            fmac1_rowbcast<6>(y1, pooled, fc1w[6]);   fmac1_rowbcast<7>(y1, pooled, fc1w[7]);   fmac1_rowbcast<8>(y1, pooled, fc1w[8]);
            fmac1_rowbcast<9>(y1, pooled, fc1w[9]);   fmac1_rowbcast<10>(y1, pooled, fc1w[10]); fmac1_rowbcast<11>(y1, pooled, fc1w[11]);
            fmac1_rowbcast<12>(y1, pooled, fc1w[12]); fmac1_rowbcast<13>(y1, pooled, fc1w[13]); fmac1_rowbcast<14>(y1, pooled, fc1w[14]);
            fmac1_rowbcast<15>(y1, pooled, fc1w[15]);
            y1 = relu(y1);
            const float pred = Row<16>::allsum(y1 * fc2w) + fc2b;
            float dpred = 0.f;                                             // x S
            if (rowok) {
                const float diff = pred - ylab;
                dpred = 2.f * diff * inv_gb * a.gscale;
                if (col == 0) acc_loss = fmaf(diff, diff, acc_loss);
            }
            pend = true; pend_tile = tile; pend_ns = ns; pend_pred = pred;
            if (!a.do_backward) return;
            const float dy1 = (y1 > 0.f) ? dpred * fc2w : 0.f;            // d(fc1 pre-activation), lane j
            float dpool = 0.f;
            fmac1_rowbcast<0>(dpool, dy1, fc1wT[0]);   fmac1_rowbcast<1>(dpool, dy1, fc1wT[1]);   fmac1_rowbcast<2>(dpool, dy1, fc1wT[2]);
            fmac1_rowbcast<3>(dpool, dy1, fc1wT[3]);   fmac1_rowbcast<4>(dpool, dy1, fc1wT[4]);   fmac1_rowbcast<5>(dpool, dy1, fc1wT[5]);
            fmac1_rowbcast<6>(dpool, dy1, fc1wT[6]);   fmac1_rowbcast<7>(dpool, dy1, fc1wT[7]);   fmac1_rowbcast<8>(dpool, dy1, fc1wT[8]);
            fmac1_rowbcast<9>(dpool, dy1, fc1wT[9]);   fmac1_rowbcast<10>(dpool, dy1, fc1wT[10]); fmac1_rowbcast<11>(dpool, dy1, fc1wT[11]);
            fmac1_rowbcast<12>(dpool, dy1, fc1wT[12]); fmac1_rowbcast<13>(dpool, dy1, fc1wT[13]); fmac1_rowbcast<14>(dpool, dy1, fc1wT[14]);
            fmac1_rowbcast<15>(dpool, dy1, fc1wT[15]);
            dpool = valid ? dpool : 0.f;
            acc_w2 = fmaf(dpred, y1, acc_w2);
            acc_b2 += (col == 0) ? dpred : 0.f;
            acc_b += dy1;
            acc_th = __builtin_amdgcn_mfma_f32_16x16x4f32(dy1, pooled, acc_th, 0, 0, 0);      // d fc1.w[j][t]: k = the four samples
            pend_top0 = dpool;
            pend_top1 = __builtin_bit_cast(float, arg);
            // the sums of the last BatchNorm want d X_L in the D layout: through the scratch words
            float* scr = smem + off_scr;
            scr[lane] = dpool;
            scr[64 + lane] = __builtin_bit_cast(float, arg);
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const float dv = scr[16 * s + col];
                const int da = __builtin_bit_cast(int, scr[64 + 16 * s + col]);
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    float gq = (chan[r] == da) ? dv : 0.f;
                    if (use_drop) gq = (pend_m >> (3 * s + r)) & 1u ? gq * a.drop_scale : 0.f;       // the mask layer_full hashed
                    const float dy = y2[s][r] > 0.f ? gq : 0.f;
                    s_a[r] += dy;
                    s_b[r] = fmaf(dy, xh1[s][r], s_b[r]);
                }
            }
            __builtin_amdgcn_wave_barrier();
            return;
        }

        if constexpr (KIND == PH_G) {
            // ===== backward phases =========================================================================================================
            // the gradient entering the layer: d X_{l+1}, D layout, x S
            float gin[4][3];
            if constexpr (GRAD_TOP) {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const float dv = smem[(col_ok ? off_DX + col : off_zero) + s * N];
                    const int da = __builtin_bit_cast(int, smem[(col_ok ? off_DX + pitch + col : off_zero) + s * N]);
#pragma unroll
                    for (int r = 0; r < 3; ++r) gin[s][r] = (chan[r] == da && s < ns) ? dv : 0.f;
                }
            } else if constexpr (GRAD_IN) {
                ld_tile(off_DX, gin);
                if (ns < 4) {
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        if (s >= ns) gin[s][0] = gin[s][1] = gin[s][2] = 0.f;
                }
            }
            float SB[4][3];
            if constexpr (NEED_SB) {
                ld_tile(off_SB, SB);
                if (ns < 4) {
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        if (s >= ns) SB[s][0] = SB[s][1] = SB[s][2] = 0.f;
                }
            }
            float Q[4][3];
            if constexpr (BWD_PREV) {
                ld_tile(off_XP, Q);
                if (ns < 4) {
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        if (s >= ns) Q[s][0] = Q[s][1] = Q[s][2] = INFINITY;
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
            if (nt < a.ntiles) { req_SB(nt); req_DX(nt); req_XP(nt); }

            uint32_t mask_cur = 0u;
            if constexpr (MASK_IN) {
                mask_cur = mask_next;
                if (use_drop && nt < a.ntiles) mask_next = a.mrec[LY][nt * 64 + lane];
            }
            // ---- two samples at a time (the working set of four does not fit the register file) ------------------------------------------------
            auto g_half = [&](auto HS_) {
                constexpr int HS = decltype(HS_)::value;
                constexpr int NS = 2;
                float Xh[NS][3];
                u32x4 ad[NS];
#pragma unroll
                for (int e = 0; e < NS; ++e) {
                    if constexpr (!H_IN) ad[e] = adjB[HS + e];
#pragma unroll
                    for (int r = 0; r < 3; ++r) Xh[e][r] = X[HS + e][r];
                }
                // layer LY forward again, as far as this phase needs it (H_IN: from H on)
                f32x4 Hp[NS], z[NS], AXd[NS];
                float H[NS][3];
                if constexpr (H_IN) {
#pragma unroll
                    for (int e = 0; e < NS; ++e)
#pragma unroll
                        for (int r = 0; r < 3; ++r) H[e][r] = Xh[e][r];
                } else if constexpr (H_GE) {
                    // H from its record: no T, Hp, LeakyReLU; X_l is split for (A X) alone
#pragma unroll
                    for (int e = 0; e < NS; ++e) {
                        const Split2 p01 = split2(Xh[e][0], Xh[e][1]), p2 = split2(Xh[e][2], 0.f);
                        AXd[e] = mfma16z(ad[e], u32x4{p01.hi, p2.hi, p01.hi, p2.hi});              // (A X) in the D layout: rows c, columns k
                        AXd[e] = mfma16(ad[e], u32x4{p01.lo, p2.lo, p01.lo, p2.lo}, AXd[e]);
#pragma unroll
                        for (int r = 0; r < 3; ++r) {
                            const float hv = smem[(xoff[r] >= 0 ? off_H + xoff[r] : off_zero) + (HS + e) * N];
                            H[e][r] = (HS + e < ns) ? hv : 0.f;          // beyond the batch: whatever an earlier step left
                        }
                    }
                    if constexpr (HS == 2) {
                        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                        __builtin_amdgcn_wave_barrier();
                        if (nt < a.ntiles) req_H(nt);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                } else {
                    f32x4 T[NS];
                    Op2 xo[NS];
                    stage_T(Xh, ad, T, xo);
                    if constexpr (BLK == 0) {
#pragma unroll
                        for (int e = 0; e < NS; ++e) {
                            AXd[e] = mfma16z(ad[e], xo[e].h);                                // (A X) in the D layout: rows c, columns k
                            AXd[e] = mfma16(ad[e], xo[e].l, AXd[e]);
                        }
                    }
                    stage_Hp(T, kc.th, Hp);
                    leaky_of(Hp, H);
                }
                Pk hk[NS];
                Shifted hks[NS];
                stage_conv(H, 1.0f, kc.w[0], sh_rd1, sh_rd1_lo, z, hk, hks);                  // x-hat of BatchNorm 2l
                float xh0[NS][3], y1[NS][3];
#pragma unroll
                for (int e = 0; e < NS; ++e) {
                    keep_until_here(z[e][3]);
#pragma unroll
                    for (int r = 0; r < 3; ++r) {
                        xh0[e][r] = z[e][r];
                        y1[e][r] = fmaf(kc.gam[0][r], z[e][r], kc.bet[0][r]);
                    }
                }
                // the operand the weight gradient transposes: conv_block1: H; conv_block2: V = 4 o0
                Pk dk[NS];                              // packed d z (BLK 1) -- later the packed d Hp (BLK 0)
                float dz[NS][3], gsum[NS][3], V[NS][3];
                if constexpr (BLK == 1) {
                    // ---- G_{2l+1}: conv_block2 again (BatchNorm 2l+1 backward, conv_block2 gradient, d(x0 + H)) ------------------------------
#pragma unroll
                    for (int e = 0; e < NS; ++e)
#pragma unroll
                        for (int r = 0; r < 3; ++r) V[e][r] = relu2(fmaf(2.f, H[e][r], relu2(y1[e][r])));
                    stage_conv(V, 1.0f, kc.w[1], sh_rd2, sh_rd2_lo, z, hk, hks);              // x-hat of BatchNorm 2l+1; hk, hks <- V
                }
                // BatchNorm IDX backward of one sample: d z (and, G_{2l+1}, the gradient that bypasses the convolution)
                auto bn_backward = [&](int e) {
                    if constexpr (BLK == 1) {
                        keep_until_here(z[e][3]);
#pragma unroll
                        for (int r = 0; r < 3; ++r) {
                            const float xh = z[e][r];
                            const float y2 = fmaf(kc.gam[1][r], xh, kc.bet[1][r]);
                            float gq = gin[HS + e][r];
                            if (use_drop) gq = (mask_cur >> (3 * (HS + e) + r)) & 1u ? gq * a.drop_scale : 0.f;   // hashed by F_{2l+2} / TOP
                            const bool x1pos = y2 > 0.f;
                            gsum[e][r] = (x1pos || V[e][r] > 0.f) ? gq : 0.f;                // d(x1 + o0): o1 = relu(x1 + o0) > 0
                            const float dy = x1pos ? gq : 0.f;
                            const float v = bA[r] * (fmaf(-xh, bk2[r], dy) - bk1[r]);
                            dz[e][r] = (HS + e < ns) ? v * colm : 0.f;
                        }
                    } else {
#pragma unroll
                        for (int r = 0; r < 3; ++r) {
                            const float dy = y1[e][r] > 0.f ? SB[HS + e][r] : 0.f;
                            const float v = bA[r] * (fmaf(-xh0[e][r], bk2[r], dy) - bk1[r]);
                            dz[e][r] = (HS + e < ns) ? v * colm : 0.f;
                        }
                    }
                };
                // d(input of the convolution) = W^T-conv(d z); weight gradient from the transposed tiles: acc += dzT x [hT | hsT]
                // (contraction over the columns t = 4 g + r of the transposed tiles).  The transposition is an LDS round trip: both tiles
                // are already packed (hi | lo) pairs, written as they are and read back with the transposing read, the tap at t - d as the
                // same image read d rows higher -- no matrix instruction, no split.  One image serves the samples back to back (LDS
                // operations of a wavefront execute in order).  Nothing waits for LDS with nothing to do: a sample's H / V tile makes its
                // round trip under the sample's own BatchNorm backward, its d z tile (shift tile and image) under the next sample's
                // BatchNorm backward or the d I products.
                f32x4 dI[NS];
                {
                    u32x4 bh[NS], bl[NS];
                    Pk q[NS], u[NS], us[NS];            // d z, the operand and the operand of the tap at t - d, transposed
#pragma unroll
                    for (int e = 0; e < NS; ++e) {
                        wg_img[WG_H_HI + wg_wr] = hk[e].hi;
                        wg_img[WG_H_LO + wg_wr] = hk[e].lo;
                        u[e] = Pk{lds_read_tr16(wg_img + WG_H_HI + wg_rd), lds_read_tr16(wg_img + WG_H_LO + wg_rd)};
                        us[e] = Pk{lds_read_tr16(wg_img + WG_H_HI + wg_rds), lds_read_tr16(wg_img + WG_H_LO + wg_rds)};
                        bn_backward(e);
                        const Pk p = pack3(dz[e][0], dz[e][1], dz[e][2], 0.f);
                        wg_img[WG_DZ_HI + wg_wr] = p.hi;
                        wg_img[WG_DZ_LO + wg_wr] = p.lo;
                        const Shifted nx = shift_read(sh_tile, sh_bk, sh_bk_lo, lane, p);
                        bh[e] = cat(p.hi, nx.hi);
                        bl[e] = cat(p.lo, nx.lo);
                        q[e] = Pk{lds_read_tr16(wg_img + WG_DZ_HI + wg_rd), lds_read_tr16(wg_img + WG_DZ_LO + wg_rd)};
                        __builtin_amdgcn_sched_barrier(0);
                    }
#pragma unroll
                    for (int e = 0; e < NS; ++e) {
                        dI[e] = mfma16z(wT.hi, bh[e]);
                        dI[e] = mfma16(wT.hi, bl[e], dI[e]);
                        dI[e] = mfma16(wT.lo, bh[e], dI[e]);
                        acc_w0 = mfma16(cat(q[e].hi, q[e].lo), cat(u[e].hi, u[e].hi), acc_w0);
                        acc_w1 = mfma16(cat(q[e].hi, q[e].lo), cat(us[e].hi, us[e].hi), acc_w1);
                    }
                    acc_w0 = mfma16(cat(q[0].hi, q[1].hi), cat(u[0].lo, u[1].lo), acc_w0);
                    acc_w1 = mfma16(cat(q[0].hi, q[1].hi), cat(us[0].lo, us[1].lo), acc_w1);
                    __builtin_amdgcn_sched_barrier(0);
                }
                if constexpr (BLK == 1) {
                    // d(x0 + H) and the sums of BatchNorm 2l
#pragma unroll
                    for (int e = 0; e < NS; ++e) {
                        keep_until_here(dI[e][3]);
#pragma unroll
                        for (int r = 0; r < 3; ++r) {
                            float gq = dI[e][r] + gsum[e][r];
                            gq = (V[e][r] > 0.f && HS + e < ns) ? gq * colm : 0.f;
                            rec_put(0, HS + e, r, gq);
                            const float dy = y1[e][r] > 0.f ? gq : 0.f;
                            s_a[r] += dy;
                            s_b[r] = fmaf(dy, xh0[e][r], s_b[r]);
                        }
                    }
                } else {
                    // d Hp = leaky'(Hp) (d H + d(x0 + H)); theta gradient: contraction over the channel slots
#pragma unroll
                    for (int e = 0; e < NS; ++e) {
                        keep_until_here(dI[e][3]);
                        float dHp[3];
#pragma unroll
                        for (int r = 0; r < 3; ++r) {
                            const float gq = dI[e][r] + SB[HS + e][r];
                            // H_GE: the gate from H instead of Hp -- the same branch for every input: H = Hp + c |Hp| with
                            // c = (1 - a)/(1 + a) in (0, 1) has the sign of Hp, +-0 gives 0 on both sides (not > 0), and a NaN
                            // compares false on both
                            const bool hp_pos = H_GE ? H[e][r] > 0.f : Hp[e][r] > 0.f;
                            const float v = hp_pos ? gq : gq * LEAKY;
                            dHp[r] = (HS + e < ns) ? v * colm : 0.f;
                            acc_b += dHp[r];
                        }
                        dk[e] = pack3(dHp[0], dHp[1], dHp[2], 0.f);
                    }
                    {
                        Pk ax[NS];
#pragma unroll
                        for (int e = 0; e < NS; ++e) {
                            keep_until_here(AXd[e][3]);
                            ax[e] = pack3(AXd[e][0], AXd[e][1], AXd[e][2], 0.f);
                            acc_th = mfma16(cat(dk[e].hi, dk[e].lo), cat(ax[e].hi, ax[e].hi), acc_th);
                        }
                        acc_th = mfma16(cat(dk[0].hi, dk[1].hi), cat(ax[0].lo, ax[1].lo), acc_th);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    if constexpr (LY >= 1) {
                        // d X_l = A (d Hp theta) + d X_{l+1}: U = (A d Hp)^T, then U x theta
                        f32x4 U[NS], dXl[NS];
#pragma unroll
                        for (int e = 0; e < NS; ++e) {
                            U[e] = mfma16z(cat(dk[e].hi, dk[e].hi), ad[e]);
                            U[e] = mfma16(cat(dk[e].lo, dk[e].lo), ad[e], U[e]);
                        }
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int e = 0; e < NS; ++e) {
                            const Split2 p01 = split2(U[e][0], U[e][1]), p23 = split2(U[e][2], U[e][3]);
                            const u32x4 ua = {p01.hi, p23.hi, p01.lo, p23.lo};
                            dXl[e] = mfma16z(ua, thN.hi);
                            dXl[e] = mfma16(ua, thN.lo, dXl[e]);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                        // the sums of BatchNorm 2l-1: F_{2l} left its x-hat where the gradient passes (ReLU gate, dropout), +inf elsewhere
#pragma unroll
                        for (int e = 0; e < NS; ++e) {
                            keep_until_here(dXl[e][3]);
#pragma unroll
                            for (int r = 0; r < 3; ++r) {
                                const float dX = (HS + e < ns) ? (dXl[e][r] + gin[HS + e][r]) * colm : 0.f;
                                rec_put(0, HS + e, r, dX);
                                const bool open = Q[HS + e][r] < INFINITY;
                                const float dy = open ? dX * a.drop_scale : 0.f;
                                s_a[r] += dy;
                                s_b[r] = fmaf(dy, open ? Q[HS + e][r] : 0.f, s_b[r]);
                            }
                        }
                    }
                }
            };
            g_half(std::integral_constant<int, 0>{});
            __builtin_amdgcn_sched_barrier(0);
            g_half(std::integral_constant<int, 2>{});
            if constexpr (BLK == 1 || LY >= 1) { pend = true; pend_tile = tile; pend_ns = ns; }
        }
        };
        if (ns_tile == 4) tile_body(std::true_type{});
        else tile_body(std::false_type{});
    }

    MXP_MARKI(6);                                                                  // tile loop done
    // ---- the last tile's outputs ---------------------------------------------------------------------------------------------------------
    if (pend) {
        if constexpr (NREC > 0) { RecPieces pieces; rec_read(pieces); rec_store(pieces); }
        if constexpr (WITH_PREV) {
            if (use_drop) st_rec4<MXT_RECORD_POLICY>(a.mrec[LY - 1] + pend_tile * 64 + lane, pend_m);
        }
        if constexpr (KIND == PH_TOP) {
            if (g < pend_ns && col_ok && a.do_backward) {
                float* p = a.dtop + pend_tile * (8 * N) + g * N + col;
                st_rec4<MXT_RECORD_POLICY>(p, pend_top0);
                st_rec4<MXT_RECORD_POLICY>(p + pitch, pend_top1);
            }
            if (g < pend_ns && col == 0) st_rec4<MXT_RECORD_POLICY>(a.pred + pend_tile * 4 + g, pend_pred);
            if (use_drop && a.do_backward) st_rec4<MXT_RECORD_POLICY>(a.mrec[LY] + pend_tile * 64 + lane, pend_m);
        }
    }

    MXP_MARKI(7);                                                                  // last tile's stores issued
    // ---- epilogue: the four wavefronts meet here.  BatchNorm pair: fp64 from the 16-lane reduction on, the wavefronts' sums combined in
    // a fixed order, one atomic per channel and workgroup ---------------------------------------------------------------------------------
    StepScratch* const sc = step_scratch(a.cells, L);
    bool bad = false;
    const bool has_pair = (KIND == PH_F) || (KIND == PH_TOP && a.do_backward) || (KIND == PH_G && IDX > 0);
    constexpr int PBW = 2 * F + 2;                       // doubles per wavefront in pairbuf: the pair, the loss
    if (has_pair) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            double da = (double)s_a[r], db = (double)s_b[r];
#pragma unroll
            for (int off = 8; off >= 1; off >>= 1) {
                da += __shfl_xor(da, off, 16);
                db += __shfl_xor(db, off, 16);
            }
            if (col == 0 && chan[r] >= 0) {
                pairbuf[wave * PBW + chan[r]] = da;
                pairbuf[wave * PBW + F + chan[r]] = db;
            }
        }
    }
    if constexpr (KIND == PH_TOP) {
        float vl = acc_loss;
        vl += __shfl_xor(vl, 16, 64);
        vl += __shfl_xor(vl, 32, 64);
        if (lane == 0) pairbuf[wave * PBW + 2 * F] = (double)vl;
    }
    __syncthreads();
    MXP_MARKI(8);                                                                  // pair sums in LDS
    if (has_pair && threadIdx.x < 2 * F) {
        double* cell = a.cells + (int64_t)(blockIdx.x % CELL_REPLICAS) * CS;
        if (KIND == PH_F) cell += cell_fwd(L) + IDX * 2 * F;
        else if (KIND == PH_TOP) cell += cell_bwd(L) + (NBN - 1) * 2 * F;
        else cell += cell_bwd(L) + (IDX - 1) * 2 * F;
        double v = 0.0;
#pragma unroll
        for (int w = 0; w < MXT_WAVES; ++w) v += pairbuf[w * PBW + threadIdx.x];
        atomicAdd(cell + threadIdx.x, KIND == PH_F ? v : v * (double)a.inv_gscale);
    }
    if (KIND == PH_TOP && threadIdx.x == 2 * F) {
        double v = 0.0;
#pragma unroll
        for (int w = 0; w < MXT_WAVES; ++w) v += pairbuf[w * PBW + 2 * F];
        atomicAdd(a.cells + (int64_t)(blockIdx.x % CELL_REPLICAS) * CS + cell_loss(L), v);
        bad |= !(v <= 1.0e300 && v >= 0.0);
    }
    if constexpr (KIND == PH_F) return;
    if (KIND == PH_TOP && !a.do_backward) {
        if (__any(bad) && lane == 0) atomicOr(&sc->pad[0], 1u);
        return;
    }

    MXP_MARKI(9);                                                                  // atomics issued
    // ---- the workgroup's row of partial gradients: every wavefront writes its accumulators into its own LDS image of the phase's contiguous
    // parameter range (one round, one barrier), then the row store adds the four images in a fixed order, (w0 + w2) + (w1 + w3) -- the rows,
    // and with them finalize, stay deterministic -- and the row leaves in coalesced stores ---------------------------------------------------
    const float us = a.inv_gscale;
    const int NN = N * N;
    int rbase = 0, rlen = 0;
    // (image 0 in the workgroup's region, images 1 .. 3 over the wavefronts' regions -- dead by now, 4 x wave_floats >= 3 x MXT_RED_FLOATS)
    float* const red2 = smem_all + LC.waves;
    {
        float* const img = wave == 0 ? red : red2 + (wave - 1) * MXT_RED_FLOATS;
        auto put = [&](int idx, float v) { img[idx] = v; };
        if constexpr (KIND == PH_TOP) {
            // [fc1.w | fc1.b | fc2.w | fc2.b]; fc1.w in the fp32 MFMA's D layout: row j = 4 g + r, column k = col
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = 4 * g + r;
                if (j < N && col_ok) put(j * N + col, acc_th[r]);
            }
            float vb = acc_b, vw = acc_w2, v2 = acc_b2;
            vb += __shfl_xor(vb, 16, 64); vb += __shfl_xor(vb, 32, 64);
            vw += __shfl_xor(vw, 16, 64); vw += __shfl_xor(vw, 32, 64);
            v2 += __shfl_xor(v2, 16, 64); v2 += __shfl_xor(v2, 32, 64);
            if (g == 0 && col_ok) { put(NN + col, vb); put(NN + N + col, vw); }
            if (lane == 0) put(NN + 2 * N, v2);
        }
        if constexpr (KIND == PH_G) {
            const int ci = slot_chan(col);
            const int cbase = BLK == 0 ? NN + N : 0;                  // G_{2l}: [theta.w | theta.b | conv_block1.w]; G_{2l+1}: [conv_block2.w]
            const float ws = BLK == 1 ? 0.25f : 1.f;                  // conv_block2's data operand was V = 4 o0
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const int co = chan[r];
                if (co >= 0 && ci >= 0) {
                    put(cbase + (co * F + ci) * 2 + 1, acc_w0[r] * ws);
                    put(cbase + (co * F + ci) * 2 + 0, acc_w1[r] * ws);
                }
            }
            if constexpr (BLK == 0) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = 4 * g + r;
                    if (j < N && col_ok) put(j * N + col, acc_th[r]);
                }
                float vb = acc_b;
                vb += __shfl_xor(vb, 16, 64); vb += __shfl_xor(vb, 32, 64);
                if (g == 0 && col_ok) put(NN + col, vb);
            }
        }
    }
    __syncthreads();
    MXP_MARKI(10);                                                                 // gradient image complete
    if constexpr (KIND == PH_TOP) { rbase = off_fc1_w(N, L); rlen = NN + 2 * N + 1; }
    else if constexpr (BLK == 0) { rbase = LY * LS + off_theta_w(N); rlen = NN + N + CONVW; }
    else { rbase = LY * LS + off_conv_w(N, 1); rlen = CONVW; }
    float* row = a.gpart + (size_t)blockIdx.x * a.pcount + rbase;
    for (int i = threadIdx.x; i < rlen; i += 64 * MXT_WAVES) {
        const float v = ((red[i] + red2[MXT_RED_FLOATS + i]) + (red2[i] + red2[2 * MXT_RED_FLOATS + i])) * us;
        st_rec4<MXT_RECORD_POLICY>(row + i, v);
        bad |= !finite_f(v);
    }
    if (__any(bad) && lane == 0) atomicOr(&sc->pad[0], 1u);
}

template <int L, int KIND, int IDX, int NFIX>
__global__ __launch_bounds__(64 * MXT_WAVES, MX_WAVES_PER_SIMD) void stgcn_train_mx_kernel(MxTrainK a) {
    extern __shared__ __attribute__((aligned(16))) float smem_all[];
    mxt_phase_body<L, KIND, IDX, NFIX, false>(a, smem_all, 0u);
#ifdef MXP_TRACE
    mxp_dump();
#endif
}

// =====================================================================================================================
// Small batches: F_1 .. G_0 as ONE launch (RULGNN_STEP_MX_PERSIST; an experiment kept as an explicit, tested option -- it does NOT pay:
// 85 us per step at batch 100 against 77 us for the ten launches, profiles/r06_notes.md section 4).  At the reference protocol's batch
// (100: configs/hparams.py:16-27) a phase is one tile per wavefront on seven workgroups and the ten-launch chain is ten dispatches + ten
// prologues at their latency floor.  Here every workgroup walks the phases itself; between two phases stands an arrival counter instead
// of a kernel boundary:
//   * arrive: the workgroup's cell atomics (agent scope) and its own record stores are drained (s_waitcnt vmcnt(0)), the wavefronts meet,
//     one agent-scope atomic add;
//   * wait: in the NEXT phase's prologue, right in front of the cell reads (mxt_phase_body<PERSIST>): the first tile's LDS-DMA requests
//     and the parameter loads / operand conversions that need no BatchNorm are in flight by then.
// No fence on either side: the only data that crosses a workgroup inside the launch are the fp64 cells -- atomics on the producing and
// the consuming side (MI355X_MICROARCH.md, inter-workgroup visibility: "8-B agent atomics both sides"); tiles stay on the wavefront that
// owns them (same grid, same tile -> wavefront map in every phase), the gradient rows and the status word are read by the finalize
// LAUNCH.  F_0 stays its own launch (other translation unit; it also carries the head-of-step scalars).
// The grid must be co-resident: the host launches it only when every workgroup has a CU of its own.
// =====================================================================================================================
// (inlined: as calls -- 80 callee-saved registers through scratch per phase -- the step measured 94 us instead of 85)
template <int L, int KIND, int IDX, int NFIX>
__device__ __forceinline__ void mxt_persist_phase(const MxTrainK& a, float* smem_all, unsigned& arrived_phases) {
    mxt_phase_body<L, KIND, IDX, NFIX, true>(a, smem_all, arrived_phases * gridDim.x);
    constexpr bool PERSIST = true;
    MXP_MARKI(11);                                                                 // body returned
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    MXP_MARKI(12);                                                                 // drained
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_fetch_add(step_barrier(a.cells, L), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    ++arrived_phases;
}
template <int L, int NFIX, int I>
struct MxtPersistChain {
    static __device__ __forceinline__ void forward(const MxTrainK& a, float* smem_all, unsigned& n) {
        if constexpr (I > 1) MxtPersistChain<L, NFIX, I - 1>::forward(a, smem_all, n);
        mxt_persist_phase<L, PH_F, I, NFIX>(a, smem_all, n);
    }
    static __device__ __forceinline__ void backward(const MxTrainK& a, float* smem_all, unsigned& n) {
        mxt_persist_phase<L, PH_G, I, NFIX>(a, smem_all, n);
        if constexpr (I > 0) MxtPersistChain<L, NFIX, I - 1>::backward(a, smem_all, n);
    }
};
template <int L, int NFIX>
__global__ __launch_bounds__(64 * MXT_WAVES, MX_WAVES_PER_SIMD) void stgcn_train_mx_persist_kernel(MxTrainK a) {
    extern __shared__ __attribute__((aligned(16))) float smem_all[];
    unsigned n = 0;                                   // phases this workgroup has arrived at; F_1 reads what F_0's LAUNCH left: target 0
    MxtPersistChain<L, NFIX, 2 * L - 1>::forward(a, smem_all, n);
    mxt_persist_phase<L, PH_TOP, 0, NFIX>(a, smem_all, n);
    MxtPersistChain<L, NFIX, 2 * L - 1>::backward(a, smem_all, n);
#ifdef MXP_TRACE
    mxp_dump();
#endif
}

// =====================================================================================================================
// host side
// =====================================================================================================================
constexpr int mxt_nfix(int N) { return N == 14 ? 14 : 0; }      // the NFIX mxt_launch_n instantiates
// stgcn_train_mx_shape_ok admits num_patch <= 15 and at most MX_MAX_LAYERS layers: the largest request (G_{2l}, l >= 1: five tiles and the
// transposing image per wavefront; six tiles where it reads H_l, which mxt_g_even_reads_h allows at N = 14 only) stays inside what a
// launch may ask for -- 80 KB, two workgroups per CU -- so a shape the gate accepts cannot fail a launcher's check.
constexpr size_t MXT_MAX_LDS_BYTES = 80 * 1024;
constexpr size_t mxt_lds_bytes_max(int L, int N) {
    int m = 0;
    mxt_each_phase(L, [&](int kind, int idx) { m = std::max(m, mxt_lds(L, kind, idx, mxt_nfix(N), N).total); });
    return sizeof(float) * (size_t)m;
}
static_assert(mxt_lds_bytes_max(MX_MAX_LAYERS, 15) <= MXT_MAX_LDS_BYTES && mxt_lds_bytes_max(MX_MAX_LAYERS, 14) <= MXT_MAX_LDS_BYTES &&
                  mxt_lds_bytes_max(1, 15) <= MXT_MAX_LDS_BYTES,
              "every matrix-core phase must fit its LDS limit");
// Pinned (the launches' requests must not move with an edit of mxt_lds): the bytes of every phase (G_2 at three layers and N = 15: the generic
// body, without the H tile)
constexpr bool mxt_bytes_are(int L, int N, std::initializer_list<int> want) {
    const int* w = want.begin();
    bool ok = (int)want.size() == 4 * L;
    mxt_each_phase(L, [&](int kind, int idx) { ok = ok && 4 * mxt_lds(L, kind, idx, mxt_nfix(N), N).total == *w++; });
    return ok;
}
// (F_{2l}, l >= 1, staged where produced: two more staging tiles per wavefront, 2 x 4 x 160 N bytes)
constexpr int mxt_f_even_extra(int N) { return MXT_STAGE_EARLY ? 2 * MXT_WAVES * 160 * N : 0; }
static_assert(mxt_f_even_extra(14) == 17920 || !MXT_STAGE_EARLY);
static_assert(mxt_bytes_are(1, 14, {30320, 33840, 42096, 47536}));
static_assert(mxt_bytes_are(2, 14, {30880, 34400, 34400 + mxt_f_even_extra(14), 21920, 42656, 48096, 78496, 48096}));
static_assert(mxt_bytes_are(3, 14, {31440, 34960, 34960 + mxt_f_even_extra(14), 22480, 34960 + mxt_f_even_extra(14), 22480, 43216, 48656, 79056, 48656, 79056, 48656}));
static_assert(mxt_bytes_are(2, 15, {32160, 35680, 35680 + mxt_f_even_extra(15), 22560, 43936, 50016, 72736, 50016}));
static_assert(mxt_bytes_are(3, 15, {32720, 36240, 36240 + mxt_f_even_extra(15), 23120, 36240 + mxt_f_even_extra(15), 23120, 44496, 50576, 73296, 50576, 73296, 50576}));
static_assert(mxt_bytes_are(2, 2, {15520, 19040, 19040 + mxt_f_even_extra(2), 14240, 27296, 25056, 31136, 25056}));

template <int L, int KIND, int IDX, int NFIX>
static int mxt_launch(const MxTrainK& k, hipStream_t stream, int max_grid, int* grid_out) {
    auto kern = &stgcn_train_mx_kernel<L, KIND, IDX, NFIX>;
    const size_t lds = sizeof(float) * (size_t)mxt_lds(L, KIND, IDX, NFIX, k.N).total;
    if (const int rc = allow_dynamic_lds(kern, lds, MXT_MAX_LDS_BYTES); rc != RULGNN_OK) return rc;
    auto [cus, per_cu] = residency(kern, 64 * MXT_WAVES, lds);
    if (per_cu > MX_WAVES_PER_SIMD) per_cu = MX_WAVES_PER_SIMD;           // a workgroup is one wavefront per SIMD
    if (const char* e = getenv("RULGNN_MXT_BLOCKS_PER_CU")) { const int v = atoi(e); if (v > 0) per_cu = v; }   // tuning aid
    int64_t grid = (int64_t)cus * per_cu;
    const int64_t want = (k.ntiles + MXT_WAVES - 1) / MXT_WAVES;
    if (grid > want) grid = want;
    if (grid > max_grid) grid = max_grid;
    if (grid_out) *grid_out = (int)grid;
    return launch_checked(kern, dim3((unsigned)grid), dim3(64 * MXT_WAVES), lds, stream, k);
}

template <int L, int KIND, int IDX>
static int mxt_launch_n(const MxTrainK& k, hipStream_t stream, int max_grid, int* grid_out) {
    if (mxt_nfix(k.N) == 14) return mxt_launch<L, KIND, IDX, 14>(k, stream, max_grid, grid_out);
    return mxt_launch<L, KIND, IDX, 0>(k, stream, max_grid, grid_out);
}

template <int L>
static int mxt_phase(int kind, int idx, const MxTrainK& k, hipStream_t st, int mg, int* go) {
    if (kind == PH_TOP) return mxt_launch_n<L, PH_TOP, 0>(k, st, mg, go);
    return mxt_dispatch_phase<2 * L - 1>(kind, idx, [&](auto K, auto I) { return mxt_launch_n<L, decltype(K)::value, decltype(I)::value>(k, st, mg, go); });
}

bool stgcn_train_mx_shape_ok(const rulgnn_stgcn_shape* s, const float* x) {
    const int N = s->num_patch, P = s->patch_size, L = s->num_layers;
    if (N < 2 || N > 15 || L < 1 || L > MX_MAX_LAYERS || s->mpnn_k != 1) return false;
    if (((int64_t)N * P) % 4 != 0 || (reinterpret_cast<uintptr_t>(x) & 15) != 0) return false;     // F_0's 16-byte DMA pieces
    return true;
}

float stgcn_train_mx_grad_scale(int64_t global_batch) {
    int e = 0;
    while (((int64_t)1 << e) < global_batch && e < 40) ++e;
    return ldexpf(1.0f, e + 3);
}

// F_1 .. G_0 of a whole step as one launch (stgcn_train_mx_persist_kernel): two layers, a batch small enough that every workgroup of
// the phases' common grid (one tile per wavefront) has a CU of its own -- RULGNN_EUNSUPPORTED otherwise, and the caller runs the phases
// as launches.  *grid_out = the grid: every phase's partial gradient rows (finalize).
template <int NFIX>
static int mxt_persist_launch(const MxTrainK& k, hipStream_t stream, int64_t grid) {
    constexpr int L = 2;
    auto kern = &stgcn_train_mx_persist_kernel<L, NFIX>;
    const size_t lds = mxt_lds_bytes_max(L, k.N);
    if (const int rc = allow_dynamic_lds(kern, lds, MXT_MAX_LDS_BYTES); rc != RULGNN_OK) return rc;
    return launch_checked(kern, dim3((unsigned)grid), dim3(64 * MXT_WAVES), lds, stream, k);
}
int stgcn_train_mx_persistent_grid(int64_t batch, int num_layers, int max_grid) {
    if (num_layers != 2 || batch <= 0) return 0;
    const int cus = device_cu_count();
    const int64_t grid = ((batch + 3) / 4 + MXT_WAVES - 1) / MXT_WAVES;
    // one workgroup per CU: co-resident whatever else runs.  (Measured with a 512-workgroup grid at the headline batch: 0.44 ms against
    // 0.345 for the launches, 0.23 against 0.14 at 16 384 -- one register allocation for eight bodies spills in the tile loops.)
    return grid <= cus && grid <= max_grid ? (int)grid : 0;
}
int stgcn_train_mx_persistent(const MxTrainArgs& m, hipStream_t stream, int max_grid, int* grid_out) {
    const int grid = m.do_backward ? stgcn_train_mx_persistent_grid(m.B, m.L, max_grid) : 0;
    if (grid == 0) return RULGNN_EUNSUPPORTED;
    const MxTrainK k = mxt_kernel_args(m, 4);
    if (grid_out) *grid_out = grid;
    return mxt_nfix(k.N) == 14 ? mxt_persist_launch<14>(k, stream, grid) : mxt_persist_launch<0>(k, stream, grid);
}

int stgcn_train_mx_phase(const MxTrainArgs& m, int kind, int idx, hipStream_t stream, int max_grid, int* grid_out) {
    const MxTrainK k = mxt_kernel_args(m, 4);
    if (m.B == 0) { if (grid_out) *grid_out = 0; return RULGNN_OK; }
    switch (m.L) {
        case 1: return mxt_phase<1>(kind, idx, k, stream, max_grid, grid_out);
        case 2: return mxt_phase<2>(kind, idx, k, stream, max_grid, grid_out);
        case 3: return mxt_phase<3>(kind, idx, k, stream, max_grid, grid_out);
        default: return RULGNN_EUNSUPPORTED;
    }
}

}  // namespace rulgnn
