// AGCN_TF on gfx950.
// Reference path replaced: AGCN_TF_model.forward -- models/AGCN_TF/Model.py:137-189 (features :7-72, MPNN_mk :75-101, SelfAttention
// :104-122, MultiHeadSelfAttention :125-134) -- and AGCN_TF.update, algorithms/algorithms.py:574-599 (plain MSE + Adam).
//
//   x [bs, P * n] -> X [P, 40]: SAGCN's 40 statistics per patch, cumulative columns, unit Frobenius norm (sagcn_features: csrc/sagcn.hip)
//   temporal branch, nodes = patches:  U_t = tanh(X W1t^T + b1t) [P, Ha], A_t = U_t W2t^T + b2t [P, P], H_t = lrelu((A_t X) Tt^T + bt)
//   spatial branch, nodes = features:  the same on X^T [40, P] with W1s [Ha, P], W2s [40, Ha], Ts [Hg, P]
//   H = [H_s ; H_t] [N = 40 + P, Hg] -> per head softmax((H Wq^T + bq)(H Wk^T + bk)^T / sqrt(Hg)) (H Wv^T + bv) -> heads side by side
//   -> Linear(N * heads * Hg -> 1).
//
// Two facts carry the kernels.  The adjacency is linear in its MLP's output, so
//   A_t X = U_t G_t + 1 c_t^T,  G_t = W2t^T X [Ha, 40],  c_t = X^T b2t [40]      (spatial: G_s = W2s^T X^T [Ha, P], c_s = X b2s [P])
// and neither A nor dA exists anywhere: dU = dM G^T, dG = U^T dM, dW2 = sum_b X_b dG_b^T, db2 = sum_b X_b colsum(dM_b).  And the head is
// linear in the attention output, so d loss / d O_b = dpred_b W_fc: the attention backward reads W_fc and one scalar per sample, and
// delta_i = sum_c dO_ic O_ic = dpred_b (the row's share of the fc dot product), which the forward stores next to the log-sum-exp.
//
// Every product inside the kernels is a workgroup-level loop over 16 x 16 tiles of v_mfma_f32_16x16x4_f32 (at_mm): the operands are
// read through small accessors (LDS blocks, parameters or activations in HBM / L2), out-of-range rows, columns and k are fed as zeros,
// so Ha, Hg, P and N are padded to the tile in registers only.  The Q / K / V projections and dH = sum dQ Wq + dK Wk + dV Wv are
// calls into the shared sgemm over the B * N rows (the biases are added where the attention kernels load the rows); every parameter
// gradient but fc's is a split-K product over all samples in a fixed order (sgemm_splitk_batch), fc's a fixed-order sum over the batch.
// No floating-point atomics anywhere: two runs give the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sgemm_mfma.hpp"
#include "families_host.hpp"

namespace rulgnn {

namespace {

constexpr int AT_GB = 256, AT_WAVES = AT_GB / 64;
constexpr int AT_F = 40, AT_LD = AT_F + 1, AT_RAW = 20;
constexpr int AT_RT = 64;                    // U rows (temporal) / G_s columns (spatial) per tile of the graph stage
constexpr int AT_QT = 64;                    // query rows per workgroup of the attention forward
constexpr int AT_BT = 32;                    // own rows per workgroup of the attention backward (two score blocks in LDS)
constexpr int AT_KC = 64;                    // rows of the other side staged per chunk
constexpr int AT_MAXP = 256, AT_MAXN = 2048, AT_MAXH = 128, AT_MAXHEADS = 4;
constexpr float AT_SLOPE = 0.01f;            // F.leaky_relu's default

struct AtGeom {
    int64_t B;
    int P, n, Ha, Hg, heads, N, HD, nqt, nbt;             // N = 40 + P nodes, HD = heads * Hg, query tiles (forward) / row tiles (backward)
    float scale;
    int o_w1s, o_b1s, o_w2s, o_b2s, o_w1t, o_b1t, o_w2t, o_b2t, o_ths, o_bs, o_tht, o_bt, o_head, head_stride, o_wfc, o_bfc, pcount;
    // workspace, float offsets
    int64_t w_raw, w_feat, w_H, w_Q, w_K, w_V, w_O, w_lse, w_rowdot, w_part, w_dpred, w_sq, w_one;
    int64_t w_dQ, w_dK, w_dV, w_dH, w_dZt, w_dZs, w_Mt, w_Ms, w_dpUt, w_dpUs, w_dGt, w_dct, w_dGs, w_dcs, w_XT, w_split;
    size_t split_floats, total_bytes;
    size_t lds_graph_fwd, lds_graph_bwd, lds_attn_fwd, lds_attn_bwd;
};

// LDS of the graph stage, float offsets.  X [P][41] | c_t [40] | dc_t [40] | c_s [P] | then the temporal blocks and the spatial blocks
// over the same floats (the branches run one after the other)
struct AtGraphLds {
    int X, ct, dct, cs, U, G, M, dM, dG, Us, Gs, Ms, dUs, total;
};
__host__ __device__ inline AtGraphLds at_graph_lds(int P, int Ha, bool bwd) {
    AtGraphLds l;
    l.X = 0;
    l.ct = P * AT_LD;
    l.dct = l.ct + AT_F;
    l.cs = l.dct + AT_F;
    const int base = (l.cs + P + 1) & ~1;
    l.U = base;                                // [AT_RT][Ha + 1]
    l.G = l.U + AT_RT * (Ha + 1);              // [Ha][41]
    l.M = l.G + Ha * AT_LD;                    // [AT_RT][41]
    l.dM = l.M + AT_RT * AT_LD;                // [AT_RT][41]      (backward)
    l.dG = l.dM + AT_RT * AT_LD;               // [Ha][41]         (backward)
    const int end_t = bwd ? l.dG + Ha * AT_LD : l.dM;
    l.Us = base;                               // [40][Ha + 1]
    l.Gs = l.Us + AT_F * (Ha + 1);             // [Ha][AT_RT + 1]
    l.Ms = l.Gs + Ha * (AT_RT + 1);            // [40][P + 1]      (backward: dM_s)
    l.dUs = l.Ms + AT_F * (P + 1);             // [40][Ha + 1]     (backward)
    const int end_s = bwd ? l.dUs + AT_F * (Ha + 1) : l.dUs;
    l.total = end_t > end_s ? end_t : end_s;
    return l;
}
__host__ __device__ inline int at_score_ld(int N) { return N + 1 + (N & 1); }      // odd: rows land on different banks

int at_geometry(const rulgnn_agcntf_shape* s, AtGeom* g) {
    if (!s) return RULGNN_EINVAL;
    if (s->batch < 0 || s->num_patch < 1 || s->patch_size < 2 || s->hidden_adj_dim < 1 || s->hidden_gnn_dim < 1 || s->num_heads < 1) return RULGNN_EINVAL;
    if (s->num_patch > AT_MAXP || s->patch_size > AT_MAXN || s->hidden_adj_dim > AT_MAXH || s->hidden_gnn_dim > AT_MAXH || s->num_heads > AT_MAXHEADS)
        return RULGNN_EUNSUPPORTED;
    g->B = s->batch; g->P = s->num_patch; g->n = s->patch_size; g->Ha = s->hidden_adj_dim; g->Hg = s->hidden_gnn_dim; g->heads = s->num_heads;
    g->N = AT_F + g->P; g->HD = g->heads * g->Hg;
    g->nqt = (g->N + AT_QT - 1) / AT_QT; g->nbt = (g->N + AT_BT - 1) / AT_BT;
    g->scale = 1.0f / sqrtf((float)g->Hg);
    const int P = g->P, Ha = g->Ha, Hg = g->Hg, N = g->N, HD = g->HD;
    {   // int row counts of the GEMMs, 32-bit workgroup counts
        const int widest = HD > Ha ? (HD > AT_F ? HD : AT_F) : (Ha > AT_F ? Ha : AT_F);
        if (g->B * (int64_t)N * widest >= (int64_t)1 << 31 || g->B * (int64_t)P * (g->n > AT_F ? g->n : AT_F) >= (int64_t)1 << 31) return RULGNN_EUNSUPPORTED;
    }
    int o = 0;
    g->o_w1s = o; o += Ha * P;    g->o_b1s = o; o += Ha;
    g->o_w2s = o; o += AT_F * Ha; g->o_b2s = o; o += AT_F;
    g->o_w1t = o; o += Ha * AT_F; g->o_b1t = o; o += Ha;
    g->o_w2t = o; o += P * Ha;    g->o_b2t = o; o += P;
    g->o_ths = o; o += Hg * P;    g->o_bs = o; o += Hg;
    g->o_tht = o; o += Hg * AT_F; g->o_bt = o; o += Hg;
    g->o_head = o; g->head_stride = 3 * (Hg * Hg + Hg); o += g->heads * g->head_stride;
    g->o_wfc = o; o += N * HD;
    g->o_bfc = o; o += 1;
    g->pcount = o;
    // LDS of every kernel, decided here: a shape whose kernels would not fit is unsupported before anything is launched
    g->lds_graph_fwd = sizeof(float) * (size_t)at_graph_lds(P, Ha, false).total;
    g->lds_graph_bwd = sizeof(float) * (size_t)at_graph_lds(P, Ha, true).total;
    g->lds_attn_fwd = sizeof(float) * ((size_t)(AT_QT + AT_KC) * (Hg + 1) + (size_t)AT_QT * at_score_ld(N) + AT_QT);
    g->lds_attn_bwd = sizeof(float) * ((size_t)(2 * AT_BT + AT_KC) * (Hg + 1) + (size_t)2 * AT_BT * at_score_ld(N) + 2 * N);
    const size_t need[] = {g->lds_graph_fwd, g->lds_graph_bwd, g->lds_attn_fwd, g->lds_attn_bwd, sizeof(float) * ((size_t)P * AT_LD + AT_GB),
                           sizeof(float) * ((size_t)3 * g->n + g->n / 2 + 1 + 7 * AT_GB)};
    for (size_t v : need)
        if (v > MAX_LDS_BYTES) return RULGNN_EUNSUPPORTED;
    WsCarver c;
    auto take = [&c](int64_t nfl) { return (int64_t)(c.take<float>((size_t)(nfl > 0 ? nfl : 1)) / sizeof(float)); };
    const int64_t B = g->B, BN = B * N, BP = B * P;
    g->w_raw = take(BP * AT_RAW);
    g->w_feat = take(BP * AT_F);
    g->w_H = take(BN * Hg);
    g->w_Q = take(BN * HD); g->w_K = take(BN * HD); g->w_V = take(BN * HD); g->w_O = take(BN * HD);
    g->w_lse = take(B * g->heads * N);
    g->w_rowdot = take(B * g->heads * N);
    g->w_part = take(B * g->heads * g->nqt);
    g->w_dpred = take(B); g->w_sq = take(B); g->w_one = take(64);
    g->w_dQ = take(BN * HD); g->w_dK = take(BN * HD); g->w_dV = take(BN * HD);
    g->w_dH = take(BN * Hg);
    g->w_dZt = take(BP * Hg); g->w_dZs = take(B * AT_F * Hg);
    g->w_Mt = take(BP * AT_F); g->w_Ms = take(B * AT_F * P);
    g->w_dpUt = take(BP * Ha); g->w_dpUs = take(B * AT_F * Ha);
    g->w_dGt = take((int64_t)Ha * B * AT_F); g->w_dct = take(B * AT_F);
    g->w_dGs = take(BP * Ha); g->w_dcs = take(BP);
    g->w_XT = take((int64_t)P * B * AT_F);
    g->split_floats = 1024;
    if (B > 0) {
        // the parameter-gradient products go ten at a time (at_pgrad_jobs): the scratch holds the largest group
        SplitKJob jobs[12 + 6 * AT_MAXHEADS];
        int nj = 0;
        const int kbp = (int)BP, kbf = (int)(B * AT_F), kbn = (int)BN;
        const int dims[][3] = {{Hg, AT_F, kbp}, {1, Hg, kbp}, {Ha, AT_F, kbp}, {1, Ha, kbp}, {P, Ha, kbf}, {P, 1, kbf},
                               {Hg, P, kbf},    {1, Hg, kbf}, {Ha, P, kbf},    {1, Ha, kbf}, {AT_F, Ha, kbp}, {AT_F, 1, kbp}};
        for (const auto& d : dims) { jobs[nj] = SplitKJob{}; jobs[nj].M = d[0]; jobs[nj].N = d[1]; jobs[nj].K = d[2]; ++nj; }
        for (int h = 0; h < 3 * g->heads; ++h) {
            jobs[nj] = SplitKJob{}; jobs[nj].M = Hg; jobs[nj].N = Hg; jobs[nj].K = kbn; ++nj;
            jobs[nj] = SplitKJob{}; jobs[nj].M = 1; jobs[nj].N = Hg; jobs[nj].K = kbn; ++nj;
        }
        for (int j0 = 0; j0 < nj; j0 += 10) {
            const size_t v = sgemm_splitk_batch_floats(jobs + j0, nj - j0 < 10 ? nj - j0 : 10);
            g->split_floats = v > g->split_floats ? v : g->split_floats;
        }
    }
    g->w_split = take((int64_t)g->split_floats);
    g->total_bytes = c.total();
    return RULGNN_OK;
}

__device__ __forceinline__ f32x4t at_mfma(float a, float b, f32x4t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ float at_lrelu(float v) { return v > 0.f ? v : AT_SLOPE * v; }

// C[M][N] = sum_k a(m, k) b(k, n) by the whole workgroup: wavefront w takes the (16-row, NB x 16-column) tasks w, w + 4, ...;
// lane (kq, li) = (lane / 16, lane % 16) feeds A[m = li][k = 4 s + kq] and B[k = 4 s + kq][n = li] and receives C[m = 4 kq + r][n = li].
// a, b are called for in-range (m, k) / (k, n) only (the rest is fed as zeros), c(m, n, value) once for every in-range output; M, N, K >= 1.
// No barrier inside: the caller separates the producers of a / b and the consumers of c.
template <int NB, class FA, class FB, class FC>
__device__ __forceinline__ void at_mm(int M, int N, int K, FA a, FB b, FC c) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, kq = lane >> 4;
    const int mt = (M + 15) >> 4, ng = (N + 16 * NB - 1) / (16 * NB);
    for (int t = wave; t < mt * ng; t += AT_WAVES) {
        const int i = t / ng, j0 = (t - i * ng) * NB;
        f32x4t acc[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) acc[j] = (f32x4t){0.f, 0.f, 0.f, 0.f};
        // out-of-range rows / columns read a clamped (valid) element and feed a zero: the loads carry no condition, so the unrolled loop
        // has the operands of four k steps in flight; the last, partial k step is taken apart
        const int m = 16 * i + li, mc = m < M ? m : M - 1;
        const bool m_in = m < M;
        int nc[NB];
        bool nin[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int nn = 16 * (j0 + j) + li;
            nin[j] = nn < N;
            nc[j] = nin[j] ? nn : N - 1;
        }
        const int Kmain = K & ~3;
#pragma unroll 4
        for (int k0 = 0; k0 < Kmain; k0 += 4) {
            const int k = k0 + kq;
            const float a0 = a(mc, k), av = m_in ? a0 : 0.f;
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const float b0 = b(k, nc[j]);
                acc[j] = at_mfma(av, nin[j] ? b0 : 0.f, acc[j]);
            }
        }
        if (Kmain < K) {
            const int k = Kmain + kq, kc = k < K ? k : K - 1;
            const bool kin = k < K;
            const float a0 = a(mc, kc), av = (m_in && kin) ? a0 : 0.f;
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const float b0 = b(kc, nc[j]);
                acc[j] = at_mfma(av, (nin[j] && kin) ? b0 : 0.f, acc[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int nn = 16 * (j0 + j) + li;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int mm = 16 * i + 4 * kq + r;
                if (mm < M && nn < N) c(mm, nn, acc[j][r]);
            }
        }
    }
}

// ---- graph stage: one workgroup per sample, both branches from the feature block in LDS ------------------------------------------------
// Forward (BWD = false) writes H [B][N][Hg] (spatial rows first).  Backward recomputes U, G, c and M of both branches from the features
// -- the forward keeps nothing but H, whose sign is the leaky ReLU's -- and writes, per sample, the factors of the parameter-gradient
// products: dZ_t [B][P][Hg], M_t [B][P][40], dU_t(1 - U_t^2) [B][P][Ha], dG_t [Ha][B][40], colsum(dM_t) [B][40], X again as [P][B][40];
// dZ_s [B][40][Hg], M_s [B][40][P], dU_s(1 - U_s^2) [B][40][Ha], dG_s^T [B][P][Ha], colsum(dM_s) [B][P].
struct AtGraphBufs {
    const float* feat;
    float* H;                 // forward: written; backward: read
    const float* dH;
    float *dZt, *dZs, *Mt, *Ms, *dpUt, *dpUs, *dGt, *dct, *dGs, *dcs, *XT;
};

template <bool BWD>
__global__ __launch_bounds__(AT_GB) void at_graph_kernel(AtGeom g, const float* __restrict__ prm, AtGraphBufs q) {
    extern __shared__ float lds[];
    const int P = g.P, Ha = g.Ha, Hg = g.Hg, N = g.N, tid = threadIdx.x;
    const AtGraphLds l = at_graph_lds(P, Ha, BWD);
    const int UL = Ha + 1, GL = AT_RT + 1, ML = P + 1;
    float* X = lds + l.X;
    float* ct = lds + l.ct;
    float* dct = lds + l.dct;
    float* cs = lds + l.cs;
    float* U = lds + l.U;
    float* G = lds + l.G;
    float* M = lds + l.M;
    float* dM = lds + l.dM;
    float* dG = lds + l.dG;
    float* Us = lds + l.Us;
    float* Gs = lds + l.Gs;
    float* Ms = lds + l.Ms;
    float* dUs = lds + l.dUs;
    const float* W1s = prm + g.o_w1s; const float* b1s = prm + g.o_b1s; const float* W2s = prm + g.o_w2s; const float* b2s = prm + g.o_b2s;
    const float* W1t = prm + g.o_w1t; const float* b1t = prm + g.o_b1t; const float* W2t = prm + g.o_w2t; const float* b2t = prm + g.o_b2t;
    const float* Ths = prm + g.o_ths; const float* bs = prm + g.o_bs; const float* Tht = prm + g.o_tht; const float* bt = prm + g.o_bt;
    for (int64_t b = blockIdx.x; b < g.B; b += gridDim.x) {
        __syncthreads();
        const float* fb = q.feat + b * P * AT_F;
        for (int i = tid; i < P * AT_F; i += AT_GB) X[(i / AT_F) * AT_LD + i % AT_F] = fb[i];
        __syncthreads();
        // ---- temporal branch ----
        if (tid < AT_F) {
            float a = 0.f;
            for (int p = 0; p < P; ++p) a = fmaf(b2t[p], X[p * AT_LD + tid], a);
            ct[tid] = a;
            dct[tid] = 0.f;
        }
        for (int p = tid; p < P; p += AT_GB) {
            float a = 0.f;
            for (int j = 0; j < AT_F; ++j) a = fmaf(b2s[j], X[p * AT_LD + j], a);
            cs[p] = a;
        }
        at_mm<3>(Ha, AT_F, P, [&](int m, int k) { return W2t[k * Ha + m]; }, [&](int k, int n) { return X[k * AT_LD + n]; },
                 [&](int m, int n, float v) { G[m * AT_LD + n] = v; });
        if (BWD) {
            float* xt = q.XT + b * AT_F;
            for (int i = tid; i < P * AT_F; i += AT_GB) xt[(int64_t)(i / AT_F) * g.B * AT_F + i % AT_F] = X[(i / AT_F) * AT_LD + i % AT_F];
        }
        __syncthreads();
        for (int r0 = 0; r0 < P; r0 += AT_RT) {
            const int rv = P - r0 < AT_RT ? P - r0 : AT_RT;
            at_mm<4>(rv, Ha, AT_F, [&](int m, int k) { return X[(r0 + m) * AT_LD + k]; }, [&](int k, int n) { return W1t[n * AT_F + k]; },
                     [&](int m, int n, float v) { U[m * UL + n] = tanhf(v + b1t[n]); });
            __syncthreads();
            at_mm<3>(rv, AT_F, Ha, [&](int m, int k) { return U[m * UL + k]; }, [&](int k, int n) { return G[k * AT_LD + n]; },
                     [&](int m, int n, float v) { M[m * AT_LD + n] = v + ct[n]; });
            __syncthreads();
            if (!BWD) {
                float* hb = q.H + (b * N + AT_F + r0) * Hg;
                at_mm<4>(rv, Hg, AT_F, [&](int m, int k) { return M[m * AT_LD + k]; }, [&](int k, int n) { return Tht[n * AT_F + k]; },
                         [&](int m, int n, float v) { hb[m * Hg + n] = at_lrelu(v + bt[n]); });
            } else {
                const float* hb = q.H + (b * N + AT_F + r0) * Hg;
                const float* dh = q.dH + (b * N + AT_F + r0) * Hg;
                float* dz = q.dZt + (b * P + r0) * Hg;
                for (int i = tid; i < rv * Hg; i += AT_GB) dz[i] = hb[i] > 0.f ? dh[i] : AT_SLOPE * dh[i];
                float* mg = q.Mt + (b * P + r0) * AT_F;
                for (int i = tid; i < rv * AT_F; i += AT_GB) mg[i] = M[(i / AT_F) * AT_LD + i % AT_F];
                __syncthreads();                  // dZ_t of this tile is read back below (same workgroup, same L1)
                at_mm<3>(rv, AT_F, Hg, [&](int m, int k) { return dz[m * Hg + k]; }, [&](int k, int n) { return Tht[k * AT_F + n]; },
                         [&](int m, int n, float v) { dM[m * AT_LD + n] = v; });
                __syncthreads();
                if (tid < AT_F) {
                    float a = dct[tid];
                    for (int m = 0; m < rv; ++m) a += dM[m * AT_LD + tid];
                    dct[tid] = a;
                }
                float* du = q.dpUt + (b * P + r0) * Ha;
                at_mm<4>(rv, Ha, AT_F, [&](int m, int k) { return dM[m * AT_LD + k]; }, [&](int k, int n) { return G[n * AT_LD + k]; },
                         [&](int m, int n, float v) { const float u = U[m * UL + n]; du[m * Ha + n] = v * (1.f - u * u); });
                at_mm<3>(Ha, AT_F, rv, [&](int m, int k) { return U[k * UL + m]; }, [&](int k, int n) { return dM[k * AT_LD + n]; },
                         [&](int m, int n, float v) { dG[m * AT_LD + n] = r0 == 0 ? v : dG[m * AT_LD + n] + v; });
            }
            __syncthreads();
        }
        if (BWD) {
            for (int i = tid; i < Ha * AT_F; i += AT_GB)
                q.dGt[((int64_t)(i / AT_F) * g.B + b) * AT_F + i % AT_F] = dG[(i / AT_F) * AT_LD + i % AT_F];
            if (tid < AT_F) q.dct[b * AT_F + tid] = dct[tid];
            __syncthreads();
        }
        // ---- spatial branch ----
        at_mm<4>(AT_F, Ha, P, [&](int m, int k) { return X[k * AT_LD + m]; }, [&](int k, int n) { return W1s[n * P + k]; },
                 [&](int m, int n, float v) { Us[m * UL + n] = tanhf(v + b1s[n]); });
        const float* dzs = q.dZs + b * AT_F * Hg;
        if (BWD) {
            const float* hb = q.H + b * N * Hg;
            const float* dh = q.dH + b * N * Hg;
            float* dz = q.dZs + b * AT_F * Hg;
            for (int i = tid; i < AT_F * Hg; i += AT_GB) dz[i] = hb[i] > 0.f ? dh[i] : AT_SLOPE * dh[i];
            for (int i = tid; i < AT_F * UL; i += AT_GB) dUs[i] = 0.f;
            __syncthreads();
            // dM_s [40][P] over the floats that hold M_s in the forward (M_s goes straight to HBM here)
            at_mm<4>(AT_F, P, Hg, [&](int m, int k) { return dzs[m * Hg + k]; }, [&](int k, int n) { return Ths[k * P + n]; },
                     [&](int m, int n, float v) { Ms[m * ML + n] = v; });
            __syncthreads();
            for (int p = tid; p < P; p += AT_GB) {
                float a = 0.f;
                for (int j = 0; j < AT_F; ++j) a += Ms[j * ML + p];
                q.dcs[b * P + p] = a;
            }
        }
        __syncthreads();
        for (int p0 = 0; p0 < P; p0 += AT_RT) {
            const int cv = P - p0 < AT_RT ? P - p0 : AT_RT;
            at_mm<4>(Ha, cv, AT_F, [&](int m, int k) { return W2s[k * Ha + m]; }, [&](int k, int n) { return X[(p0 + n) * AT_LD + k]; },
                     [&](int m, int n, float v) { Gs[m * GL + n] = v; });
            __syncthreads();
            if (!BWD) {
                at_mm<4>(AT_F, cv, Ha, [&](int m, int k) { return Us[m * UL + k]; }, [&](int k, int n) { return Gs[k * GL + n]; },
                         [&](int m, int n, float v) { Ms[m * ML + p0 + n] = v + cs[p0 + n]; });
            } else {
                float* mg = q.Ms + b * AT_F * P + p0;
                at_mm<4>(AT_F, cv, Ha, [&](int m, int k) { return Us[m * UL + k]; }, [&](int k, int n) { return Gs[k * GL + n]; },
                         [&](int m, int n, float v) { mg[m * P + n] = v + cs[p0 + n]; });
                at_mm<4>(AT_F, Ha, cv, [&](int m, int k) { return Ms[m * ML + p0 + k]; }, [&](int k, int n) { return Gs[n * GL + k]; },
                         [&](int m, int n, float v) { dUs[m * UL + n] += v; });
                float* dg = q.dGs + (b * P + p0) * Ha;
                at_mm<4>(cv, Ha, AT_F, [&](int m, int k) { return Ms[k * ML + p0 + m]; }, [&](int k, int n) { return Us[k * UL + n]; },
                         [&](int m, int n, float v) { dg[m * Ha + n] = v; });
            }
            __syncthreads();
        }
        if (!BWD) {
            float* hb = q.H + b * N * Hg;
            at_mm<4>(AT_F, Hg, P, [&](int m, int k) { return Ms[m * ML + k]; }, [&](int k, int n) { return Ths[n * P + k]; },
                     [&](int m, int n, float v) { hb[m * Hg + n] = at_lrelu(v + bs[n]); });
        } else {
            float* du = q.dpUs + b * AT_F * Ha;
            for (int i = tid; i < AT_F * Ha; i += AT_GB) {
                const int j = i / Ha, h = i - j * Ha;
                const float u = Us[j * UL + h];
                du[i] = dUs[j * UL + h] * (1.f - u * u);
            }
        }
    }
}

// ---- attention --------------------------------------------------------------------------------------------------------------------------
// rows [r0, r0 + nr) of one sample and head into an LDS block [.][D + 1]: kind 0 / 1 / 2 = the projected Q / K / V (+ its bias, which the
// projection GEMM leaves out), 3 = dO = dpred * W_fc
struct AtAttnBufs {
    const float *Q, *K, *V;
    float* O;
    float *lse, *rowdot, *part;
    const float* dpred;
    float *dQ, *dK, *dV;
};
__device__ __forceinline__ void at_load_rows(const AtGeom& g, const float* __restrict__ prm, const AtAttnBufs& q, int kind, int64_t b, int head,
                                             int r0, int nr, float* dst) {
    const int D = g.Hg, DL = D + 1, HD = g.HD;
    if (kind == 3) {
        const float dp = q.dpred[b];
        const float* w = prm + g.o_wfc + (int64_t)r0 * HD + head * D;
        for (int i = threadIdx.x; i < nr * D; i += AT_GB) { const int r = i / D, c = i - r * D; dst[r * DL + c] = dp * w[r * HD + c]; }
    } else {
        const float* src = (kind == 0 ? q.Q : (kind == 1 ? q.K : q.V)) + (b * g.N + r0) * HD + head * D;
        const float* bias = prm + g.o_head + head * g.head_stride + kind * (D * D + D) + D * D;
        for (int i = threadIdx.x; i < nr * D; i += AT_GB) { const int r = i / D, c = i - r * D; dst[r * DL + c] = src[(int64_t)r * HD + c] + bias[c]; }
    }
}

// Forward: one workgroup per (sample, head, tile of AT_QT query rows).  The tile's whole score block [AT_QT][N] stays in LDS: scores from
// K in chunks of AT_KC rows, an exact two-pass softmax over the N real columns (the padding never enters: neither the maximum nor the sum
// nor the products), then P V from V in chunks.  Writes O, the rows' log-sum-exp, every row's share of the fc dot product (the backward's
// delta up to dpred) and the tile's share of the prediction.  LDS: Qt / O tile [AT_QT][D + 1] | chunk [AT_KC][D + 1] | S [AT_QT][ld] | rowv [AT_QT]
__global__ __launch_bounds__(AT_GB) void at_attn_fwd_kernel(AtGeom g, const float* __restrict__ prm, AtAttnBufs q) {
    extern __shared__ float lds[];
    const int D = g.Hg, DL = D + 1, N = g.N, HD = g.HD, SL = at_score_ld(N), tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* Qt = lds;
    float* Ch = Qt + AT_QT * DL;
    float* S = Ch + AT_KC * DL;
    float* rowv = S + AT_QT * SL;
    const int64_t items = g.B * g.heads * g.nqt;
    for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
        const int qt = (int)(it % g.nqt), head = (int)((it / g.nqt) % g.heads);
        const int64_t b = it / ((int64_t)g.nqt * g.heads);
        const int q0 = qt * AT_QT, qn = N - q0 < AT_QT ? N - q0 : AT_QT;
        __syncthreads();
        at_load_rows(g, prm, q, 0, b, head, q0, qn, Qt);
        for (int k0 = 0; k0 < N; k0 += AT_KC) {
            const int kn = N - k0 < AT_KC ? N - k0 : AT_KC;
            at_load_rows(g, prm, q, 1, b, head, k0, kn, Ch);
            __syncthreads();
            at_mm<4>(qn, kn, D, [&](int m, int k) { return Qt[m * DL + k]; }, [&](int k, int n) { return Ch[n * DL + k]; },
                     [&](int m, int n, float v) { S[m * SL + k0 + n] = v * g.scale; });
            __syncthreads();
        }
        for (int r = wave; r < qn; r += AT_WAVES) {
            float* s = S + r * SL;
            float mx = -INFINITY;
            for (int j = lane; j < N; j += 64) mx = fmaxf(mx, s[j]);
#pragma unroll
            for (int m = 32; m > 0; m >>= 1) mx = fmaxf(mx, __shfl_xor(mx, m, 64));
            float sum = 0.f;
            for (int j = lane; j < N; j += 64) { const float e = expf(s[j] - mx); s[j] = e; sum += e; }
#pragma unroll
            for (int m = 32; m > 0; m >>= 1) sum += __shfl_xor(sum, m, 64);
            const float inv = 1.0f / sum;
            for (int j = lane; j < N; j += 64) s[j] *= inv;
            if (lane == 0) q.lse[(b * g.heads + head) * N + q0 + r] = mx + logf(sum);
        }
        for (int k0 = 0; k0 < N; k0 += AT_KC) {
            const int kn = N - k0 < AT_KC ? N - k0 : AT_KC;
            __syncthreads();
            at_load_rows(g, prm, q, 2, b, head, k0, kn, Ch);
            __syncthreads();
            at_mm<4>(qn, D, kn, [&](int m, int k) { return S[m * SL + k0 + k]; }, [&](int k, int n) { return Ch[k * DL + n]; },
                     [&](int m, int n, float v) { Qt[m * DL + n] = k0 == 0 ? v : Qt[m * DL + n] + v; });
        }
        __syncthreads();
        for (int r = wave; r < qn; r += AT_WAVES) {
            float* o = q.O + (b * N + q0 + r) * HD + head * D;
            const float* w = prm + g.o_wfc + (int64_t)(q0 + r) * HD + head * D;
            float a = 0.f;
            for (int c = lane; c < D; c += 64) { const float v = Qt[r * DL + c]; o[c] = v; a = fmaf(v, w[c], a); }
#pragma unroll
            for (int m = 32; m > 0; m >>= 1) a += __shfl_xor(a, m, 64);
            if (lane == 0) { rowv[r] = a; q.rowdot[(b * g.heads + head) * N + q0 + r] = a; }
        }
        __syncthreads();
        if (tid == 0) {
            float a = 0.f;
            for (int r = 0; r < qn; ++r) a += rowv[r];
            q.part[it] = a;
        }
    }
}

// pred = b_fc + the tiles' shares in a fixed order; MSE share and dpred against y
__global__ void at_head_finish_kernel(AtGeom g, const float* __restrict__ part, const float* __restrict__ prm, const float* __restrict__ y,
                                      float* __restrict__ pred, float* __restrict__ sq, float* __restrict__ dpred, float inv_gb) {
    const int per = g.heads * g.nqt;
    for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < g.B; b += (int64_t)gridDim.x * blockDim.x) {
        float a = prm[g.o_bfc];
        for (int k = 0; k < per; ++k) a += part[b * per + k];
        pred[b] = a;
        if (y) {
            const float d = a - y[b];
            sq[b] = d * d * inv_gb;
            dpred[b] = 2.f * d * inv_gb;
        }
    }
}

// g fc.weight[i] = sum_b dpred[b] O[b][i], g fc.bias = sum_b dpred[b]: one thread per element, the samples in order
__global__ void at_fc_grad_kernel(AtGeom g, const float* __restrict__ O, const float* __restrict__ dpred, float* __restrict__ gw, float* __restrict__ gb) {
    const int64_t tot = (int64_t)g.N * g.HD;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= tot; i += (int64_t)gridDim.x * blockDim.x) {
        float a = 0.f;
        if (i < tot) {
            for (int64_t b = 0; b < g.B; ++b) a = fmaf(dpred[b], O[b * tot + i], a);
            gw[i] = a;
        } else {
            for (int64_t b = 0; b < g.B; ++b) a += dpred[b];
            gb[0] = a;
        }
    }
}

// Backward, one workgroup per (sample, head, tile of AT_BT own rows), the other side's N rows in chunks; no atomics: the query-side pass
// owns rows of dQ, the key-side pass rows of dK and dV.  Scores are recomputed from Q, K and the saved log-sum-exp:
//   P_ij = exp(s_ij - lse_i),  dP_ij = dO_i . V_j,  dS_ij = P_ij (dP_ij - delta_i) / sqrt(Hg),  delta_i = dpred * rowdot_i
//   query side: own = (Q_i, dO_i) -> dQ = dS K          key side: own = (K_j, V_j) -> dK = dS^T Q, dV = P^T dO   (blocks held transposed)
// LDS: A1, A2 [AT_BT][D + 1] (own rows; then the outputs) | chunk [AT_KC][D + 1] | S1, S2 [AT_BT][ld] | lse [N] | delta [N]
template <bool KEYSIDE>
__global__ __launch_bounds__(AT_GB) void at_attn_bwd_kernel(AtGeom g, const float* __restrict__ prm, AtAttnBufs q) {
    extern __shared__ float lds[];
    const int D = g.Hg, DL = D + 1, N = g.N, HD = g.HD, SL = at_score_ld(N), tid = threadIdx.x;
    float* A1 = lds;
    float* A2 = A1 + AT_BT * DL;
    float* Ch = A2 + AT_BT * DL;
    float* S1 = Ch + AT_KC * DL;
    float* S2 = S1 + AT_BT * SL;
    float* lse = S2 + AT_BT * SL;
    float* delta = lse + N;
    const int64_t items = g.B * g.heads * g.nbt;
    for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
        const int bt = (int)(it % g.nbt), head = (int)((it / g.nbt) % g.heads);
        const int64_t b = it / ((int64_t)g.nbt * g.heads);
        const int r0 = bt * AT_BT, rn = N - r0 < AT_BT ? N - r0 : AT_BT;
        __syncthreads();
        at_load_rows(g, prm, q, KEYSIDE ? 1 : 0, b, head, r0, rn, A1);
        at_load_rows(g, prm, q, KEYSIDE ? 2 : 3, b, head, r0, rn, A2);
        {
            const float dp = q.dpred[b];
            const int64_t at = (b * g.heads + head) * N;
            for (int i = tid; i < N; i += AT_GB) { lse[i] = q.lse[at + i]; delta[i] = dp * q.rowdot[at + i]; }
        }
        // S1 = own (Q or K) . other (K or Q)^T / sqrt(Hg);  S2 = own (dO or V) . other (V or dO)^T
        for (int pass = 0; pass < 2; ++pass) {
            float* A = pass == 0 ? A1 : A2;
            float* S = pass == 0 ? S1 : S2;
            const float sc = pass == 0 ? g.scale : 1.f;
            const int kind = pass == 0 ? (KEYSIDE ? 0 : 1) : (KEYSIDE ? 3 : 2);
            for (int k0 = 0; k0 < N; k0 += AT_KC) {
                const int kn = N - k0 < AT_KC ? N - k0 : AT_KC;
                __syncthreads();
                at_load_rows(g, prm, q, kind, b, head, k0, kn, Ch);
                __syncthreads();
                // (two column tiles per task: 2 x 2 tasks for the four wavefronts; four per task left two of them idle)
                at_mm<2>(rn, kn, D, [&](int m, int k) { return A[m * DL + k]; }, [&](int k, int n) { return Ch[n * DL + k]; },
                         [&](int m, int n, float v) { S[m * SL + k0 + n] = v * sc; });
            }
        }
        __syncthreads();
        for (int i = tid; i < rn * N; i += AT_GB) {
            const int r = i / N, c = i - r * N;
            const int qi = KEYSIDE ? c : r0 + r;                  // the query index of this entry
            const float p = expf(S1[r * SL + c] - lse[qi]);
            S1[r * SL + c] = p;
            S2[r * SL + c] = p * (S2[r * SL + c] - delta[qi]) * g.scale;
        }
        // out1 = dS . other (K or Q) -> A1;  key side: out2 = P^T . dO -> A2
        for (int pass = 0; pass < (KEYSIDE ? 2 : 1); ++pass) {
            float* A = pass == 0 ? A1 : A2;
            float* S = pass == 0 ? S2 : S1;
            const int kind = pass == 0 ? (KEYSIDE ? 0 : 1) : 3;
            for (int k0 = 0; k0 < N; k0 += AT_KC) {
                const int kn = N - k0 < AT_KC ? N - k0 : AT_KC;
                __syncthreads();
                at_load_rows(g, prm, q, kind, b, head, k0, kn, Ch);
                __syncthreads();
                at_mm<4>(rn, D, kn, [&](int m, int k) { return S[m * SL + k0 + k]; }, [&](int k, int n) { return Ch[k * DL + n]; },
                         [&](int m, int n, float v) { A[m * DL + n] = k0 == 0 ? v : A[m * DL + n] + v; });
            }
        }
        __syncthreads();
        float* o1 = (KEYSIDE ? q.dK : q.dQ) + (b * N + r0) * HD + head * D;
        for (int i = tid; i < rn * D; i += AT_GB) { const int r = i / D, c = i - r * D; o1[(int64_t)r * HD + c] = A1[r * DL + c]; }
        if (KEYSIDE) {
            float* o2 = q.dV + (b * N + r0) * HD + head * D;
            for (int i = tid; i < rn * D; i += AT_GB) { const int r = i / D, c = i - r * D; o2[(int64_t)r * HD + c] = A2[r * DL + c]; }
        }
    }
}

inline unsigned at_grid(int64_t n, int64_t cap) {
    return (unsigned)(n < 1 ? 1 : (n > cap ? cap : n));
}

// the parameter-gradient products of one step, each one strided product over all samples (K = B * P, B * 40 or B * N rows)
int at_pgrad_jobs(const AtGeom& g, float* ws, float* gr, SplitKJob* jobs) {
    const int P = g.P, Ha = g.Ha, Hg = g.Hg, HD = g.HD;
    const int kbp = (int)(g.B * P), kbf = (int)(g.B * AT_F), kbn = (int)(g.B * g.N);
    const int64_t bf = g.B * AT_F;
    const float* one = ws + g.w_one;
    const float* feat = ws + g.w_feat;
    const float* XT = ws + g.w_XT;
    int nj = 0;
    auto add = [&](const float* A, int64_t sAm, int64_t sAk, const float* Bm, int64_t sBn, int64_t sBk, float* C, int64_t ldc, int M, int N, int K) {
        jobs[nj++] = SplitKJob{A, sAm, sAk, Bm, sBn, sBk, C, ldc, M, N, K};
    };
    auto bias = [&](const float* Bm, int64_t sBk, float* C, int N, int K) { add(one, 0, 0, Bm, 1, sBk, C, N, 1, N, K); };
    add(ws + g.w_dZt, 1, Hg, ws + g.w_Mt, 1, AT_F, gr + g.o_tht, AT_F, Hg, AT_F, kbp);          // theta_t = dZ_t^T M_t
    bias(ws + g.w_dZt, Hg, gr + g.o_bt, Hg, kbp);
    add(ws + g.w_dpUt, 1, Ha, feat, 1, AT_F, gr + g.o_w1t, AT_F, Ha, AT_F, kbp);                // W1t = dpreU_t^T X
    bias(ws + g.w_dpUt, Ha, gr + g.o_b1t, Ha, kbp);
    add(XT, bf, 1, ws + g.w_dGt, bf, 1, gr + g.o_w2t, Ha, P, Ha, kbf);                           // W2t = sum_b X dG_t^T
    add(XT, bf, 1, ws + g.w_dct, 0, 1, gr + g.o_b2t, 1, P, 1, kbf);                              // b2t = sum_b X colsum(dM_t)
    add(ws + g.w_dZs, 1, Hg, ws + g.w_Ms, 1, P, gr + g.o_ths, P, Hg, P, kbf);                    // theta_s = dZ_s^T M_s
    bias(ws + g.w_dZs, Hg, gr + g.o_bs, Hg, kbf);
    add(ws + g.w_dpUs, 1, Ha, XT, bf, 1, gr + g.o_w1s, P, Ha, P, kbf);                           // W1s = dpreU_s^T X^T
    bias(ws + g.w_dpUs, Ha, gr + g.o_b1s, Ha, kbf);
    add(feat, 1, AT_F, ws + g.w_dGs, 1, Ha, gr + g.o_w2s, Ha, AT_F, Ha, kbp);                    // W2s = sum_b X^T dG_s^T
    add(feat, 1, AT_F, ws + g.w_dcs, 0, 1, gr + g.o_b2s, 1, AT_F, 1, kbp);                       // b2s = sum_b X^T colsum(dM_s)
    const int64_t dq[3] = {g.w_dQ, g.w_dK, g.w_dV};
    for (int h = 0; h < g.heads; ++h)
        for (int t = 0; t < 3; ++t) {
            const float* d = ws + dq[t] + h * Hg;
            float* gw = gr + g.o_head + h * g.head_stride + t * (Hg * Hg + Hg);
            add(d, 1, HD, ws + g.w_H, 1, Hg, gw, Hg, Hg, Hg, kbn);                               // W = d(QKV)^T H
            bias(d, HD, gw + Hg * Hg, Hg, kbn);
        }
    return nj;
}

}  // namespace

// RULGNN_OK, or the code every entry returns for a refused shape: unsupported for anything at_geometry refuses, a negative batch included.
int Agcntf::shape_status(const Shape* s) {
    AtGeom g;
    return at_geometry(s, &g) == RULGNN_OK ? RULGNN_OK : RULGNN_EUNSUPPORTED;
}

int64_t Agcntf::param_count(const Shape* s) {
    AtGeom g;
    return at_geometry(s, &g) == RULGNN_OK ? g.pcount : -1;
}

size_t Agcntf::workspace_bytes(const Shape* s) {
    AtGeom g;
    return at_geometry(s, &g) == RULGNN_OK ? g.total_bytes : 0;
}

int64_t Agcntf::tap_offset(const Shape* s, int which) {
    AtGeom g;
    if (at_geometry(s, &g) != RULGNN_OK) return -1;
    switch (which) {
        case 0: return g.w_feat;
        case 1: return g.w_H;
        case 2: return g.w_O;
        default: return -1;
    }
}

// mode bit 0: forward, bit 1: backward (after a forward with the same args / workspace)
int Agcntf::run(const Shape* s, const Args* a, int mode, hipStream_t st) {
    AtGeom g;
    RULGNN_TRY(at_geometry(s, &g));
    if (a->workspace_bytes < g.total_bytes) return RULGNN_EWORKSPACE;
    if (g.B == 0) return RULGNN_OK;
    float* ws = static_cast<float*>(a->workspace);
    const float* prm = a->params;
    const int64_t gb = a->global_batch > 0 ? a->global_batch : g.B;
    const int Hg = g.Hg, HD = g.HD, BN = (int)(g.B * g.N);
    const int64_t qkv[3] = {g.w_Q, g.w_K, g.w_V};
    AtGraphBufs gq{ws + g.w_feat, ws + g.w_H, ws + g.w_dH, ws + g.w_dZt, ws + g.w_dZs, ws + g.w_Mt, ws + g.w_Ms, ws + g.w_dpUt,
                   ws + g.w_dpUs, ws + g.w_dGt, ws + g.w_dct, ws + g.w_dGs, ws + g.w_dcs, ws + g.w_XT};
    AtAttnBufs aq{ws + g.w_Q, ws + g.w_K, ws + g.w_V, ws + g.w_O, ws + g.w_lse, ws + g.w_rowdot, ws + g.w_part,
                  a->dpred ? a->dpred : ws + g.w_dpred, ws + g.w_dQ, ws + g.w_dK, ws + g.w_dV};
    if (mode & 1) {
        RULGNN_TRY(sagcn_features(g.B, g.P, g.n, a->x, ws + g.w_raw, ws + g.w_feat, st));
        RULGNN_TRY(allow_dynamic_lds(at_graph_kernel<false>, g.lds_graph_fwd));
        RULGNN_TRY(launch_checked(at_graph_kernel<false>, dim3(at_grid(g.B, 8192)), dim3(AT_GB), g.lds_graph_fwd, st, g, prm, gq));
        for (int h = 0; h < g.heads; ++h)
            for (int t = 0; t < 3; ++t)
                RULGNN_TRY(sgemm(ws + g.w_H, Hg, 1, prm + g.o_head + h * g.head_stride + t * (Hg * Hg + Hg), Hg, 1, ws + qkv[t] + h * Hg, HD, BN, Hg,
                                 Hg, false, st));
        RULGNN_TRY(allow_dynamic_lds(at_attn_fwd_kernel, g.lds_attn_fwd));
        RULGNN_TRY(launch_checked(at_attn_fwd_kernel, dim3(at_grid(g.B * g.heads * g.nqt, 1 << 16)), dim3(AT_GB), g.lds_attn_fwd, st, g, prm, aq));
        RULGNN_TRY(launch_checked(at_head_finish_kernel, dim3(at_grid((g.B + AT_GB - 1) / AT_GB, 4096)), dim3(AT_GB), 0, st, g, (const float*)(ws + g.w_part),
                                  prm, a->y, a->pred, ws + g.w_sq, ws + g.w_dpred, 1.0f / (float)gb));
        if (a->y && a->loss) RULGNN_TRY(block_sum((const float*)(ws + g.w_sq), g.B, a->loss, st));
    }
    if (mode & 2) {
        if (!a->grads) return RULGNN_EINVAL;
        float* gr = a->grads;
        RULGNN_TRY(fill_f32(ws + g.w_one, 1, 1.0f, st));
        RULGNN_TRY(launch_checked(at_fc_grad_kernel, dim3(at_grid(((int64_t)g.N * HD + AT_GB) / AT_GB, 8192)), dim3(AT_GB), 0, st, g, (const float*)(ws + g.w_O),
                                  aq.dpred, gr + g.o_wfc, gr + g.o_bfc));
        RULGNN_TRY(allow_dynamic_lds(at_attn_bwd_kernel<false>, g.lds_attn_bwd));
        RULGNN_TRY(allow_dynamic_lds(at_attn_bwd_kernel<true>, g.lds_attn_bwd));
        const unsigned grid = at_grid(g.B * g.heads * g.nbt, 1 << 16);
        RULGNN_TRY(launch_checked(at_attn_bwd_kernel<false>, dim3(grid), dim3(AT_GB), g.lds_attn_bwd, st, g, prm, aq));
        RULGNN_TRY(launch_checked(at_attn_bwd_kernel<true>, dim3(grid), dim3(AT_GB), g.lds_attn_bwd, st, g, prm, aq));
        // dH [B N, Hg] = sum over heads of dQ Wq + dK Wk + dV Wv
        const int64_t dq[3] = {g.w_dQ, g.w_dK, g.w_dV};
        for (int h = 0; h < g.heads; ++h)
            for (int t = 0; t < 3; ++t)
                RULGNN_TRY(sgemm(ws + dq[t] + h * Hg, HD, 1, prm + g.o_head + h * g.head_stride + t * (Hg * Hg + Hg), 1, Hg, ws + g.w_dH, Hg, BN, Hg,
                                 Hg, h + t > 0, st));
        RULGNN_TRY(allow_dynamic_lds(at_graph_kernel<true>, g.lds_graph_bwd));
        RULGNN_TRY(launch_checked(at_graph_kernel<true>, dim3(at_grid(g.B, 8192)), dim3(AT_GB), g.lds_graph_bwd, st, g, prm, gq));
        SplitKJob jobs[12 + 6 * AT_MAXHEADS];
        const int nj = at_pgrad_jobs(g, ws, gr, jobs);
        for (int j0 = 0; j0 < nj; j0 += 10)
            RULGNN_TRY(sgemm_splitk_batch(jobs + j0, nj - j0 < 10 ? nj - j0 : 10, ws + g.w_split, g.split_floats, st));
    }
    return RULGNN_OK;
}

}  // namespace rulgnn
