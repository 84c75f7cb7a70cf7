// LOGO on gfx950.
// Reference path replaced: LOGO_model.forward -- models/LOGO/Model.py:198-262 (Pearson graph :17-35, local graph :39-54, gated fusion
// :163-196, MPNN_mk :130-160, Bi_LSTM_Standard :75-126, graph-learning loss :56-71) -- and LOGO.update, algorithms/algorithms.py:107-136
// (MSE + theta * L_GL, Adam, no scheduler step).
//
//   x [B, N, T p] -> per graph g = (b, t): Xg = x[b, :, t p : (t + 1) p] [N, p], E = Xg Wn^T + bn [N, 2p],
//   A_T = softmax_row(leaky(E E^T - 1e8 I)) + I; per sample A_G = Pearson(x[b]) [N, N];
//   z = sigmoid(W_Z_T A_T + W_Z_G A_G), r = sigmoid(W_R_T A_T + W_R_G A_G), A^ = tanh(W_h_T A_G + W_h r)   (Linear on the last axis)
//   C = softmax_row((1 - z) A_T + z A^ - 1e8 I) + I, Hg = leaky((C E) Theta^T + b) [N, 3p]
//   -> three Bi-LSTM layers with summed halves over sequences q = t N + n whose STEPS are the samples b (3p -> 3h -> 6h -> 3h; dropout
//   behind layers 2 and 3, closing leaky) -> per sample flat [T N 3h] -> fc1 (16) ReLU fc2 (8) ReLU cls (1).
//   L_GL = mean(D . C) + gamma sqrt(mean(C^2)), D[i][j] = |Xg_i - Xg_j|^2; loss = MSE + theta L_GL.
//
// Graph stage: lg_graph_fwd / lg_graph_bwd, one workgroup per sample.  The window x[b], the Pearson graph and the
// three A_G products are built once per sample; the workgroup then walks the sample's T patches with every N x N and N x 2p intermediate in
// LDS.  HBM sees x once in and Hg once out, written in the LSTM's [q][b][3p] layout.  The backward rebuilds E, A_T, z, r, A^, C from x and
// the parameters, keeps the parameter-gradient accumulators of its samples in LDS and writes one partial row per workgroup; the rows and
// the per-sample loss sums are added in a fixed order.  No floating-point atomics anywhere: two runs give the same bits.
// The products are N <= 32 by N <= 32 by at most 32 (14 x 14 x 20 at FD001) and the stage is bounded by its ~12 workgroup barriers per
// patch, not by arithmetic, so they are plain LDS FMA loops with one output element per thread.
//
// Temporal stack: three bilstm_forward / bilstm_backward calls (csrc/bilstm.hip, ndir = 2).  Dropout behind layer 2 is one in-place pass;
// dropout behind layer 3, the closing leaky ReLU and the transposition to the head's [b][q][3h] layout are ONE pass (fc1's k index (q, j)
// is not a two-stride view of [q][b][3h], so the pass that exists anyway writes the layout fc1 reads: no separate pack pass).
// Dropout: counter hash of the other families, key = dropout_layer_key(seed, step, site), site 0 behind bi_lstm2 and 1 behind bi_lstm3,
// element counter ((q B + b) W + j) mod 2^32 over [q][b][j] with W the layer's width.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sgemm_mfma.hpp"
#include "families_host.hpp"       // (stgcn_host.hpp: dropout_layer_key; stgcn_device.hpp: lowbias32)
#include "stft_device.hpp"        // the per-patch STFT magnitude (LOGO_bearing's front end)

namespace rulgnn {

namespace {

constexpr int LG_GB = 256;
constexpr int LG_MAXN = RULGNN_LOGO_MAX_NODES, LG_MAXP = RULGNN_LOGO_MAX_PATCH_SIZE, LG_MAXW = RULGNN_LOGO_MAX_LSTM_WIDTH,
              LG_MAXQ = RULGNN_LOGO_MAX_SEQUENCES;
constexpr int LG_ROWS = 256;                  // most workgroups of the backward = partial-gradient rows (fixed: it fixes the summation order)
constexpr int LG_F1 = 16, LG_F2 = 8;          // fc1 / fc2 widths (Model.py:214-216)
constexpr int LG_HEADROW = LG_F1 + LG_F2 * LG_F1 + LG_F2 + LG_F2 + 1;      // [g fc1.bias | g fc2.weight | g fc2.bias | g cls.weight | g cls.bias]
constexpr float LG_SLOPE = 0.01f;             // F.leaky_relu's default
constexpr float LG_DIAG = 1e8f;
// LOGO_bearing (ns = nperseg > 0): the nodes are the STFT's N = ns / 2 + 1 frequency bins, a patch's features its p = f = 1 + P / ns
// frames.  Its backward keeps the gradients of Theta [3f][2f] and W_n [2f][f] in registers of fixed owning threads (element i belongs to
// thread i mod 256, slot i / 256) across patches and samples: at f = 33 the two blocks are 8 712 of the partial row's 10 713 floats, and
// with them in LDS the XJTU_SY geometry (N 17, T 32) would need 163 968 B of the 163 840.
constexpr int LGB_MAXN = RULGNN_LOGOB_MAX_NODES, LGB_MAXF = RULGNN_LOGOB_MAX_INPUT_DIM;
constexpr int LGB_RTH = (6 * LGB_MAXF * LGB_MAXF + LG_GB - 1) / LG_GB, LGB_RWN = (2 * LGB_MAXF * LGB_MAXF + LG_GB - 1) / LG_GB;      // 26, 9
static_assert(SB == LG_GB, "stft_device.hpp strides its loops by SB");

struct LgLstm {
    int I, H;
    int o_wih[2], o_whh[2], o_bih[2], o_bhh[2];
    int64_t w_ws;
    size_t ws_bytes;
};

struct LgGeom {
    int64_t B;
    int p, T, N, h, L, Q, p2, p3, H1, H2, K1;                 // L = T p, Q = T N, K1 = Q 3h (fc1's k)
    int ns, P;                                                 // LOGO_bearing: nperseg and the raw patch size (p = its frames); LOGO: 0
    int o_wn, o_bn, o_th, o_thb, o_fu, o_f1w, o_f1b, o_f2w, o_f2b, o_cw, o_cb, pcount;
    LgLstm lstm[3];
    int nA, nB, CW, rows;                                      // partial row [Wn | bn | Theta | b | twelve fusion tensors]; backward grid
    int64_t w_hg, w_o1, w_o2, w_o3, w_td, w_pre1, w_a2, w_sq, w_dpred, w_glpart, w_gl, w_prod, w_dpre1, w_dtd, w_do3, w_do2, w_do1, w_dhg,
        w_part, w_split;
    size_t split_floats, total_bytes, lds_fwd, lds_bwd;
};

// LDS of the graph stage, float offsets, stated once for the kernels and the launcher.  Per sample: X [N][L + 1] | mu, nr [N] | A_G, PZ,
// PR, PH [N][N + 1] (the three A_G products with their biases); per patch: E, CE [N][2p + 1] | A_T, Z, R, A^, C [N][N + 1] | red [2][256];
// the backward adds G, dC, dAT, dZ, dR, dHh, SZ, SR, SH [N][N + 1], dH [N][3p + 1], dCE, dE [N][2p + 1] and the accumulators acc [CW].
// LOGO_bearing (ns > 0): acc is [bn | b | the twelve fusion tensors] only (W_n and Theta: registers, see LGB_RTH), and the STFT's staging
// area (stft_device.hpp: padded patch [P + ns], cos, sin, window [ns]) follows.
struct LgLds {
    int X, mu, nr, AG, PZ, PR, PH, E, CE, AT, Z, R, AH, C, red, G, dC, dAT, dZ, dR, dHh, SZ, SR, SH, dH, dCE, dE, acc, stft, total;
};
__host__ __device__ inline LgLds lg_lds(int N, int L, int p, int CW, bool bwd, int ns = 0, int P = 0) {
    LgLds l;
    const int NN = N * (N + 1), NE = N * (2 * p + 1);
    int o = 0;
    l.X = o; o += N * (L + 1);
    l.mu = o; o += N;
    l.nr = o; o += N;
    l.AG = o; o += NN;
    l.PZ = o; o += NN;
    l.PR = o; o += NN;
    l.PH = o; o += NN;
    l.E = o; o += NE;
    l.CE = o; o += NE;
    l.AT = o; o += NN;
    l.Z = o; o += NN;
    l.R = o; o += NN;
    l.AH = o; o += NN;
    l.C = o; o += NN;
    l.red = o; o += 2 * LG_GB;
    l.G = l.dC = l.dAT = l.dZ = l.dR = l.dHh = l.SZ = l.SR = l.SH = l.dH = l.dCE = l.dE = l.acc = o;
    if (bwd) {
        l.G = o; o += NN;
        l.dC = o; o += NN;
        l.dAT = o; o += NN;
        l.dZ = o; o += NN;
        l.dR = o; o += NN;
        l.dHh = o; o += NN;
        l.SZ = o; o += NN;
        l.SR = o; o += NN;
        l.SH = o; o += NN;
        l.dH = o; o += N * (3 * p + 1);
        l.dCE = o; o += NE;
        l.dE = o; o += NE;
        l.acc = o; o += ns > 0 ? CW - 8 * p * p : CW;
    }
    l.stft = o; o += ns > 0 ? (int)stft_lds_floats(P, ns) : 0;
    l.total = o;
    return l;
}

// The geometry behind both families' gates: p features per node and patch, T patches, N nodes; (ns, P) = (0, 0) for LOGO.
int lg_geometry_of(int64_t batch, int p_, int T_, int N_, int h_, int ns, int P, LgGeom* g) {
    g->B = batch; g->p = p_; g->T = T_; g->N = N_; g->h = h_; g->ns = ns; g->P = P;
    const int N = g->N, p = g->p, h = g->h;
    const int64_t B = g->B;
    g->L = g->T * p; g->Q = g->T * N; g->p2 = 2 * p; g->p3 = 3 * p; g->H1 = 3 * h; g->H2 = 6 * h;
    const int64_t k1 = (int64_t)g->Q * g->H1;
    if (k1 * (B > 0 ? B : 1) >= (int64_t)1 << 31 || (int64_t)g->Q * (B > 0 ? B : 1) * g->H2 >= (int64_t)1 << 31) return RULGNN_EUNSUPPORTED;
    g->K1 = (int)k1;
    int o = 0;
    g->o_wn = o; o += g->p2 * p;
    g->o_bn = o; o += g->p2;
    g->o_th = o; o += g->p3 * g->p2;
    g->o_thb = o; o += g->p3;
    g->nA = o;
    const int widths[3][2] = {{g->p3, g->H1}, {g->H1, g->H2}, {g->H2, g->H1}};
    for (int l = 0; l < 3; ++l) {
        LgLstm& k = g->lstm[l];
        k.I = widths[l][0]; k.H = widths[l][1];
        for (int d = 0; d < 2; ++d) {
            k.o_wih[d] = o; o += 4 * k.H * k.I;
            k.o_whh[d] = o; o += 4 * k.H * k.H;
            k.o_bih[d] = o; o += 4 * k.H;
            k.o_bhh[d] = o; o += 4 * k.H;
        }
    }
    g->o_fu = o; o += 6 * (N * N + N);
    g->nB = 6 * (N * N + N);
    g->o_f1w = o; o += LG_F1 * g->K1;
    g->o_f1b = o; o += LG_F1;
    g->o_f2w = o; o += LG_F2 * LG_F1;
    g->o_f2b = o; o += LG_F2;
    g->o_cw = o; o += LG_F2;
    g->o_cb = o; o += 1;
    g->pcount = o;
    g->CW = g->nA + g->nB;
    g->rows = (int)(B < 1 ? 1 : (B > LG_ROWS ? LG_ROWS : B));
    g->lds_fwd = sizeof(float) * (size_t)lg_lds(N, g->L, p, g->CW, false, ns, P).total;
    g->lds_bwd = sizeof(float) * (size_t)lg_lds(N, g->L, p, g->CW, true, ns, P).total;
    if (g->lds_fwd > MAX_LDS_BYTES || g->lds_bwd > MAX_LDS_BYTES) return RULGNN_EUNSUPPORTED;
    WsCarver c;
    auto take = [&c](int64_t nfl) { return (int64_t)(c.take<float>((size_t)(nfl > 0 ? nfl : 1)) / sizeof(float)); };
    const int64_t QB = (int64_t)g->Q * B;
    for (int l = 0; l < 3; ++l) {
        LgLstm& k = g->lstm[l];
        k.ws_bytes = 0; k.w_ws = 0;
        if (B > 0) {
            const rulgnn_bilstm_shape ls{B, g->Q, k.I, k.H};
            k.ws_bytes = bilstm_workspace_bytes(&ls);
            if (k.ws_bytes == 0) return RULGNN_EUNSUPPORTED;
            k.w_ws = take((int64_t)(k.ws_bytes / sizeof(float)));
        }
    }
    g->w_hg = take(QB * g->p3);
    g->w_o1 = take(QB * g->H1);
    g->w_o2 = take(QB * g->H2);
    g->w_o3 = take(QB * g->H1);
    g->w_td = take(B * g->K1);
    g->w_pre1 = take(B * LG_F1);
    g->w_a2 = take(B * LG_F2);
    g->w_sq = take(B); g->w_dpred = take(B);
    g->w_glpart = take(2 * B);
    g->w_gl = take(4);
    g->w_prod = take(B * LG_HEADROW);
    g->w_dpre1 = take(B * LG_F1);
    g->w_dtd = take(B * g->K1);
    g->w_do3 = take(QB * g->H1);
    g->w_do2 = take(QB * g->H2);
    g->w_do1 = take(QB * g->H1);
    g->w_dhg = take(QB * g->p3);
    g->w_part = take((int64_t)g->rows * g->CW);
    g->split_floats = 1024;
    if (B > 0) {
        const size_t need = sgemm_splitk_need_floats((int)B, LG_F1, g->K1);
        g->split_floats = need > g->split_floats ? need : g->split_floats;
    }
    g->w_split = take((int64_t)g->split_floats);
    g->total_bytes = c.total();
    return RULGNN_OK;
}

int lg_geometry(const rulgnn_logo_shape* s, LgGeom* g) {
    if (!s) return RULGNN_EINVAL;
    if (s->batch < 0 || s->patch_size < 0 || s->num_patch < 0 || s->num_nodes < 0 || s->hidden_dim < 0) return RULGNN_EINVAL;
    if (s->num_nodes < 2 || s->num_nodes > LG_MAXN || s->patch_size < 1 || s->patch_size > LG_MAXP || s->num_patch < 1 || s->hidden_dim < 1 ||
        (int64_t)s->num_nodes * s->num_patch > LG_MAXQ || (int64_t)6 * s->hidden_dim > LG_MAXW)
        return RULGNN_EUNSUPPORTED;
    return lg_geometry_of(s->batch, s->patch_size, s->num_patch, s->num_nodes, s->hidden_dim, 0, 0, g);
}

// LOGO_bearing's gate: the STFT's shape (even nperseg, more than nperseg / 2 points to reflect), kwargs that describe it, then LOGO's
// geometry on N = nperseg / 2 + 1 nodes of f = 1 + patch_size / nperseg features.
int lgb_geometry(const rulgnn_logob_shape* s, LgGeom* g) {
    if (!s) return RULGNN_EINVAL;
    if (s->batch < 0 || s->patch_size < 0 || s->num_patch < 0 || s->input_dim < 0 || s->num_nodes < 0 || s->nperseg < 0 || s->hidden_dim < 0)
        return RULGNN_EINVAL;
    if (s->nperseg < 2 || (s->nperseg & 1) || s->patch_size <= s->nperseg / 2 || s->num_patch < 1 || s->hidden_dim < 1) return RULGNN_EUNSUPPORTED;
    const int N = s->nperseg / 2 + 1, f = 1 + s->patch_size / s->nperseg;
    if (s->num_nodes != N || s->input_dim != f) return RULGNN_EINVAL;              // the reference's shape error at its first forward
    if (N > LGB_MAXN || f > LGB_MAXF || (int64_t)N * s->num_patch > RULGNN_LOGOB_MAX_SEQUENCES || (int64_t)6 * s->hidden_dim > RULGNN_LOGOB_MAX_LSTM_WIDTH)
        return RULGNN_EUNSUPPORTED;
    return lg_geometry_of(s->batch, f, s->num_patch, N, s->hidden_dim, s->nperseg, s->patch_size, g);
}

__device__ __forceinline__ float lg_lrelu(float v) { return v > 0.f ? v : LG_SLOPE * v; }
__device__ __forceinline__ float lg_dlrelu(float v) { return v > 0.f ? 1.f : LG_SLOPE; }
__device__ __forceinline__ float lg_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }
__device__ __forceinline__ float lg_relu(float v) { return v < 0.f ? 0.f : v; }          // (a NaN stays a NaN, as torch's; fmaxf would drop it)

inline unsigned lg_blocks(int64_t elems, int64_t cap = 1 << 16) {
    const int64_t n = (elems + LG_GB - 1) / LG_GB;
    return (unsigned)(n < 1 ? 1 : (n > cap ? cap : n));
}

// rows of [N][N + 1]: v -> softmax(v) + I, one thread per row
__device__ __forceinline__ void lg_softmax_rows(float* M, int N) {
    const int tid = threadIdx.x, NL = N + 1;
    if (tid < N) {
        float* row = M + tid * NL;
        float mx = -INFINITY;
        for (int j = 0; j < N; ++j) mx = fmaxf(mx, row[j]);
        float sum = 0.f;
        for (int j = 0; j < N; ++j) { const float ex = expf(row[j] - mx); row[j] = ex; sum += ex; }
        const float inv = 1.0f / sum;
        for (int j = 0; j < N; ++j) row[j] = row[j] * inv + (j == tid ? 1.0f : 0.f);
    }
}

// rows of [N][N + 1]: d (softmax + I) -> d (softmax argument), in place; Pm holds softmax + I
__device__ __forceinline__ void lg_softmax_rows_bwd(float* dM, const float* Pm, int N) {
    const int tid = threadIdx.x, NL = N + 1;
    if (tid < N) {
        float* row = dM + tid * NL;
        const float* pr = Pm + tid * NL;
        float s = 0.f;
        for (int j = 0; j < N; ++j) s = fmaf(pr[j] - (j == tid ? 1.0f : 0.f), row[j], s);
        for (int j = 0; j < N; ++j) row[j] = (pr[j] - (j == tid ? 1.0f : 0.f)) * (row[j] - s);
    }
}

// What a sample's patches share: the window in LDS, the Pearson graph A_G and PZ, PR, PH = A_G W^T + b of W_Z_G, W_R_G, W_h_T.
// ST (LOGO_bearing): xb is the raw window [T][P]; patch t goes through the STFT staging area once and its magnitude [N][f] lands in
// X[n][t f + j] -- the spectrogram exists in LDS only (the tables are built once per workgroup, before the first sample).
template <bool ST>
__device__ __forceinline__ void lg_sample_setup(const LgGeom& g, const LgLds& l, float* lds, const float* __restrict__ prm, const float* __restrict__ xb) {
    const int N = g.N, L = g.L, XL = L + 1, NL = N + 1, tid = threadIdx.x, fs = N * N + N;
    float* X = lds + l.X; float* mu = lds + l.mu; float* nr = lds + l.nr; float* AG = lds + l.AG;
    const float* wzg = prm + g.o_fu + 1 * fs; const float* wrg = prm + g.o_fu + 3 * fs; const float* wht = prm + g.o_fu + 4 * fs;
    if (ST) {
        const StftLds sl = stft_carve(lds + l.stft, g.P, g.ns);
        const int f = g.p;
        for (int t = 0; t < g.T; ++t) {
            stft_load_patch(sl, xb + (int64_t)t * g.P, g.P, g.ns, tid);
            __syncthreads();
            for (int i = tid; i < N * f; i += LG_GB) {
                const int n = i / f, j = i - n * f;
                X[n * XL + t * f + j] = stft_magnitude(sl, g.ns, n, j);
            }
            __syncthreads();
        }
    } else {
        for (int i = tid; i < N * L; i += LG_GB) X[(i / L) * XL + i % L] = xb[i];
        __syncthreads();
    }
    if (tid < N) {
        float s = 0.f;
        for (int j = 0; j < L; ++j) s += X[tid * XL + j];
        const float m = s / (float)L;
        float q = 0.f;
        for (int j = 0; j < L; ++j) { const float d = X[tid * XL + j] - m; q = fmaf(d, d, q); }
        mu[tid] = m;
        nr[tid] = sqrtf(q);
    }
    __syncthreads();
    for (int i = tid; i < N * N; i += LG_GB) {
        const int a = i / N, c = i - a * N;
        const float ma = mu[a], mc = mu[c];
        float dot = 0.f;
        for (int j = 0; j < L; ++j) dot = fmaf(X[a * XL + j] - ma, X[c * XL + j] - mc, dot);
        AG[a * NL + c] = dot / (nr[a] * nr[c]);              // a constant sensor: 0 / 0 = NaN, as the reference
    }
    __syncthreads();
    for (int i = tid; i < N * N; i += LG_GB) {
        const int r = i / N, j = i - r * N;
        float pz = wzg[N * N + j], pr = wrg[N * N + j], ph = wht[N * N + j];
#pragma unroll 4
        for (int k = 0; k < N; ++k) {
            const float ag = AG[r * NL + k];
            pz = fmaf(ag, wzg[j * N + k], pz);
            pr = fmaf(ag, wrg[j * N + k], pr);
            ph = fmaf(ag, wht[j * N + k], ph);
        }
        lds[l.PZ + r * NL + j] = pz; lds[l.PR + r * NL + j] = pr; lds[l.PH + r * NL + j] = ph;
    }
    __syncthreads();
}

// Patch t of the sample in LDS: E, (G), A_T, z, r, A^, C, CE; adds the patch's share of sum(D . C) and sum(C^2) to s1, s2.  Ends behind a
// barrier with CE complete.
template <bool BWD>
__device__ __forceinline__ void lg_patch(const LgGeom& g, const LgLds& l, float* lds, const float* __restrict__ prm, int t, float& s1, float& s2) {
    const int N = g.N, p = g.p, p2 = g.p2, XL = g.L + 1, NL = N + 1, EL = p2 + 1, tid = threadIdx.x, fs = N * N + N;
    const float* X = lds + l.X + t * p;
    float* E = lds + l.E; float* CE = lds + l.CE; float* AT = lds + l.AT; float* Z = lds + l.Z; float* R = lds + l.R; float* AH = lds + l.AH;
    float* Cm = lds + l.C; float* G = lds + l.G;
    const float* wn = prm + g.o_wn; const float* bn = prm + g.o_bn;
    const float* wzt = prm + g.o_fu; const float* wrt = prm + g.o_fu + 2 * fs; const float* wh = prm + g.o_fu + 5 * fs;
    for (int i = tid; i < N * p2; i += LG_GB) {
        const int n = i / p2, c = i - n * p2;
        float a = bn[c];
#pragma unroll 4
        for (int j = 0; j < p; ++j) a = fmaf(X[n * XL + j], wn[c * p + j], a);
        E[n * EL + c] = a;
    }
    __syncthreads();
    for (int i = tid; i < N * N; i += LG_GB) {
        const int a = i / N, c = i - a * N;
        float dot = 0.f;
        for (int k = 0; k < p2; ++k) dot = fmaf(E[a * EL + k], E[c * EL + k], dot);
        const float v = a == c ? dot - LG_DIAG : dot;
        if (BWD) G[a * NL + c] = v;
        AT[a * NL + c] = lg_lrelu(v);
    }
    __syncthreads();
    lg_softmax_rows(AT, N);
    __syncthreads();
    for (int i = tid; i < N * N; i += LG_GB) {
        const int r = i / N, j = i - r * N;
        float az = wzt[N * N + j] + lds[l.PZ + r * NL + j], ar = wrt[N * N + j] + lds[l.PR + r * NL + j];
#pragma unroll 4
        for (int k = 0; k < N; ++k) {
            const float at = AT[r * NL + k];
            az = fmaf(at, wzt[j * N + k], az);
            ar = fmaf(at, wrt[j * N + k], ar);
        }
        Z[r * NL + j] = lg_sigmoid(az);
        R[r * NL + j] = lg_sigmoid(ar);
    }
    __syncthreads();
    for (int i = tid; i < N * N; i += LG_GB) {
        const int r = i / N, j = i - r * N;
        float ah = wh[N * N + j] + lds[l.PH + r * NL + j];
#pragma unroll 4
        for (int k = 0; k < N; ++k) ah = fmaf(R[r * NL + k], wh[j * N + k], ah);
        ah = tanhf(ah);
        AH[r * NL + j] = ah;
        const float z = Z[r * NL + j];
        const float f = (1.0f - z) * AT[r * NL + j] + z * ah;
        Cm[r * NL + j] = r == j ? f - LG_DIAG : f;
    }
    __syncthreads();
    lg_softmax_rows(Cm, N);
    __syncthreads();
    for (int i = tid; i < N * p2; i += LG_GB) {
        const int n = i / p2, c = i - n * p2;
        float a = 0.f;
        for (int k = 0; k < N; ++k) a = fmaf(Cm[n * NL + k], E[k * EL + c], a);
        CE[n * EL + c] = a;
    }
    if (!BWD)
        for (int i = tid; i < N * N; i += LG_GB) {
            const int a = i / N, c = i - a * N;
            float d = 0.f;
            for (int j = 0; j < p; ++j) { const float df = X[a * XL + j] - X[c * XL + j]; d = fmaf(df, df, d); }
            const float cv = Cm[a * NL + c];
            s1 = fmaf(d, cv, s1);
            s2 = fmaf(cv, cv, s2);
        }
    __syncthreads();
}

// hg [q = t N + n][b][3p]; glpart [b][2] = the sample's sum(D . C), sum(C^2).  ST: lgb_graph_fwd, x = the raw windows [b][T][P]
// (the body of the single kernel and of the grouped one below: they differ only in where the pointers come from)
template <bool ST>
__device__ __forceinline__ void lg_graph_fwd_body(LgGeom g, const float* __restrict__ x, const float* __restrict__ prm, float* __restrict__ hg,
                                                  float* __restrict__ glpart) {
    extern __shared__ float lds[];
    const int N = g.N, p2 = g.p2, p3 = g.p3, EL = p2 + 1, tid = threadIdx.x;
    const LgLds l = lg_lds(N, g.L, g.p, g.CW, false, g.ns, g.P);
    const float* th = prm + g.o_th; const float* thb = prm + g.o_thb;
    float* CE = lds + l.CE; float* red = lds + l.red;
    const int64_t xs = ST ? (int64_t)g.T * g.P : (int64_t)N * g.L;
    if (ST) stft_tables(stft_carve(lds + l.stft, g.P, g.ns), g.ns, tid);
    for (int64_t b = blockIdx.x; b < g.B; b += gridDim.x) {
        __syncthreads();
        lg_sample_setup<ST>(g, l, lds, prm, x + b * xs);
        float s1 = 0.f, s2 = 0.f;
        for (int t = 0; t < g.T; ++t) {
            lg_patch<false>(g, l, lds, prm, t, s1, s2);
            for (int i = tid; i < N * p3; i += LG_GB) {
                const int n = i / p3, o = i - n * p3;
                float a = thb[o];
#pragma unroll 4
                for (int c = 0; c < p2; ++c) a = fmaf(CE[n * EL + c], th[o * p2 + c], a);
                hg[(((int64_t)t * N + n) * g.B + b) * p3 + o] = lg_lrelu(a);
            }
        }
        red[tid] = s1; red[LG_GB + tid] = s2;
        __syncthreads();
        if (tid < 2) {
            float a = 0.f;
            for (int i = 0; i < LG_GB; ++i) a += red[tid * LG_GB + i];
            glpart[b * 2 + tid] = a;
        }
    }
}

template <bool ST>
__global__ __launch_bounds__(LG_GB) void lg_graph_fwd(LgGeom g, const float* __restrict__ x, const float* __restrict__ prm, float* __restrict__ hg,
                                                      float* __restrict__ glpart) {
    lg_graph_fwd_body<ST>(g, x, prm, hg, glpart);
}

// Grouped forms of the two graph kernels: several runs of one shape, grid (x, runs).  Run blockIdx.y's pointers and loss weights come from
// a table that travels by value in the kernel arguments (blockIdx.y is wavefront-uniform: scalar loads from the argument segment, as in
// lstm_forward_group_kernel).  LOGO only: the LOGO_bearing (ST) bodies are not instantiated in grouped form.
struct LgGroup {
    const float *x, *prm;            // the run's batch and parameters
    float *hg, *glpart;              // forward: its graph-stage output and per-sample loss sums
    const float *dhg, *glv;          // backward: d Hg and {L_GL, S1, S2}
    float* part;                     // its partial rows
    float coef, gamma;               // d loss / d L_GL (the run's theta) and gamma
};
struct LgGroupTable {
    LgGroup grp[STEP_MAX_GROUPS];
};

__global__ __launch_bounds__(LG_GB) void lg_graph_fwd_group(LgGeom g, LgGroupTable tab) {
    const LgGroup& r = tab.grp[blockIdx.y];
    lg_graph_fwd_body<false>(g, r.x, r.prm, r.hg, r.glpart);
}

// dhg [q][b][3p] -> one partial row [nA + nB] per workgroup; glv = {L_GL, S1, S2}; coef = d loss / d L_GL.  ST: lgb_graph_bwd
template <bool ST>
__device__ __forceinline__ void lg_graph_bwd_body(LgGeom g, const float* __restrict__ x, const float* __restrict__ prm,
                                                  const float* __restrict__ dhg, const float* __restrict__ glv, float coef, float gamma,
                                                  float* __restrict__ part) {
    extern __shared__ float lds[];
    const int N = g.N, p = g.p, p2 = g.p2, p3 = g.p3, XL = g.L + 1, NL = N + 1, EL = p2 + 1, HL = p3 + 1, tid = threadIdx.x, fs = N * N + N;
    const LgLds l = lg_lds(N, g.L, p, g.CW, true, g.ns, g.P);
    const float* th = prm + g.o_th; const float* thb = prm + g.o_thb;
    const float* wzt = prm + g.o_fu; const float* wrt = prm + g.o_fu + 2 * fs; const float* wh = prm + g.o_fu + 5 * fs;
    float* E = lds + l.E; float* CE = lds + l.CE; float* AT = lds + l.AT; float* Z = lds + l.Z; float* R = lds + l.R; float* AH = lds + l.AH;
    float* Cm = lds + l.C; float* G = lds + l.G; float* dC = lds + l.dC; float* dAT = lds + l.dAT; float* dZ = lds + l.dZ; float* dR = lds + l.dR;
    float* dHh = lds + l.dHh; float* SZ = lds + l.SZ; float* SR = lds + l.SR; float* SH = lds + l.SH; float* dH = lds + l.dH; float* dCE = lds + l.dCE;
    float* dE = lds + l.dE; float* acc = lds + l.acc; const float* AG = lds + l.AG;
    // accumulators in the partial row's layout: [Wn | bn | Theta | b | W_Z_T b W_Z_G b W_R_T b W_R_G b W_h_T b W_h b]
    // (ST: [bn | b | fusion] in LDS, W_n and Theta in rWn / rTh)
    float* aWn = acc; float* abn = ST ? acc : aWn + p2 * p; float* aTh = abn + p2; float* aThb = ST ? abn + p2 : aTh + p3 * p2;
    float* aF = ST ? aThb + p3 : acc + g.nA;
    float rTh[ST ? LGB_RTH : 1], rWn[ST ? LGB_RWN : 1];
    if (ST) {
#pragma unroll
        for (int k = 0; k < LGB_RTH; ++k) rTh[ST ? k : 0] = 0.f;
#pragma unroll
        for (int k = 0; k < LGB_RWN; ++k) rWn[ST ? k : 0] = 0.f;
    }
    const int accw = ST ? g.CW - 8 * p * p : g.CW;
    const int64_t xs = ST ? (int64_t)g.T * g.P : (int64_t)N * g.L;
    if (ST) stft_tables(stft_carve(lds + l.stft, g.P, g.ns), g.ns, tid);
    const double cnt = (double)g.B * g.T * N * N;
    const float cD = (float)((double)coef / cnt);
    const float cC = (float)((double)coef * (double)gamma / (cnt * sqrt((double)glv[2] / cnt)));
    for (int i = tid; i < accw; i += LG_GB) acc[i] = 0.f;
    for (int64_t b = blockIdx.x; b < g.B; b += gridDim.x) {
        __syncthreads();
        lg_sample_setup<ST>(g, l, lds, prm, x + b * xs);
        for (int i = tid; i < N * NL; i += LG_GB) { SZ[i] = 0.f; SR[i] = 0.f; SH[i] = 0.f; }
        float u1 = 0.f, u2 = 0.f;
        for (int t = 0; t < g.T; ++t) {
            lg_patch<true>(g, l, lds, prm, t, u1, u2);
            const float* X = lds + l.X + t * p;
            // d (pre-activation of Hg)
            for (int i = tid; i < N * p3; i += LG_GB) {
                const int n = i / p3, o = i - n * p3;
                float a = thb[o];
#pragma unroll 4
                for (int c = 0; c < p2; ++c) a = fmaf(CE[n * EL + c], th[o * p2 + c], a);
                dH[n * HL + o] = dhg[(((int64_t)t * N + n) * g.B + b) * p3 + o] * lg_dlrelu(a);
            }
            __syncthreads();
            if (ST) {
#pragma unroll
                for (int k = 0; k < LGB_RTH; ++k) {
                    const int i = tid + k * LG_GB;
                    if (i < p3 * p2) {
                        const int o = i / p2, c = i - o * p2;
                        float a = 0.f;
                        for (int n = 0; n < N; ++n) a = fmaf(dH[n * HL + o], CE[n * EL + c], a);
                        rTh[ST ? k : 0] += a;
                    }
                }
            } else {
                for (int i = tid; i < p3 * p2; i += LG_GB) {
                    const int o = i / p2, c = i - o * p2;
                    float a = 0.f;
                    for (int n = 0; n < N; ++n) a = fmaf(dH[n * HL + o], CE[n * EL + c], a);
                    aTh[i] += a;
                }
            }
            for (int o = tid; o < p3; o += LG_GB) {
                float a = 0.f;
                for (int n = 0; n < N; ++n) a += dH[n * HL + o];
                aThb[o] += a;
            }
            for (int i = tid; i < N * p2; i += LG_GB) {
                const int n = i / p2, c = i - n * p2;
                float a = 0.f;
#pragma unroll 4
                for (int o = 0; o < p3; ++o) a = fmaf(dH[n * HL + o], th[o * p2 + c], a);
                dCE[n * EL + c] = a;
            }
            __syncthreads();
            // dC = dCE E^T + coef dL_GL/dC;  dE = C^T dCE
            for (int i = tid; i < N * N; i += LG_GB) {
                const int a = i / N, c = i - a * N;
                float v = 0.f;
                for (int k = 0; k < p2; ++k) v = fmaf(dCE[a * EL + k], E[c * EL + k], v);
                float d = 0.f;
                for (int j = 0; j < p; ++j) { const float df = X[a * XL + j] - X[c * XL + j]; d = fmaf(df, df, d); }
                dC[a * NL + c] = v + cD * d + cC * Cm[a * NL + c];
            }
            for (int i = tid; i < N * p2; i += LG_GB) {
                const int n = i / p2, c = i - n * p2;
                float a = 0.f;
                for (int k = 0; k < N; ++k) a = fmaf(Cm[k * NL + n], dCE[k * EL + c], a);
                dE[n * EL + c] = a;
            }
            __syncthreads();
            lg_softmax_rows_bwd(dC, Cm, N);                    // dF over dC
            __syncthreads();
            for (int i = tid; i < N * N; i += LG_GB) {
                const int r = i / N, j = i - r * N, at_ = r * NL + j;
                const float f = dC[at_], z = Z[at_], ah = AH[at_];
                const float dz = f * (ah - AT[at_]) * z * (1.0f - z), dh = f * z * (1.0f - ah * ah);
                dZ[at_] = dz; dHh[at_] = dh;
                dAT[at_] = f * (1.0f - z);
                SZ[at_] += dz; SH[at_] += dh;
            }
            __syncthreads();
            // through W_h: g W_h, g b_h, d r; through W_Z_T: g W_Z_T, g b
            for (int i = tid; i < N * N; i += LG_GB) {
                const int j = i / N, k = i - j * N;
                float a = 0.f, az = 0.f, dr = 0.f;
#pragma unroll 4
                for (int r = 0; r < N; ++r) {
                    a = fmaf(dHh[r * NL + j], R[r * NL + k], a);
                    az = fmaf(dZ[r * NL + j], AT[r * NL + k], az);
                    dr = fmaf(dHh[j * NL + r], wh[r * N + k], dr);          // (row j, column k of d r)
                }
                aF[5 * fs + i] += a;
                aF[0 * fs + i] += az;
                const float rv = R[j * NL + k];
                const float v = dr * rv * (1.0f - rv);
                dR[j * NL + k] = v;
                SR[j * NL + k] += v;
            }
            for (int j = tid; j < N; j += LG_GB) {
                float a = 0.f, az = 0.f;
                for (int r = 0; r < N; ++r) { a += dHh[r * NL + j]; az += dZ[r * NL + j]; }
                aF[5 * fs + N * N + j] += a;
                aF[0 * fs + N * N + j] += az;
            }
            __syncthreads();
            for (int i = tid; i < N * N; i += LG_GB) {
                const int j = i / N, k = i - j * N;
                float a = 0.f, da = 0.f;
#pragma unroll 4
                for (int r = 0; r < N; ++r) {
                    a = fmaf(dR[r * NL + j], AT[r * NL + k], a);
                    da = fmaf(dZ[j * NL + r], wzt[r * N + k], da);
                    da = fmaf(dR[j * NL + r], wrt[r * N + k], da);
                }
                aF[2 * fs + i] += a;
                dAT[j * NL + k] += da;
            }
            for (int j = tid; j < N; j += LG_GB) {
                float a = 0.f;
                for (int r = 0; r < N; ++r) a += dR[r * NL + j];
                aF[2 * fs + N * N + j] += a;
            }
            __syncthreads();
            lg_softmax_rows_bwd(dAT, AT, N);
            __syncthreads();
            for (int i = tid; i < N * N; i += LG_GB) {
                const int a = i / N, c = i - a * N;
                dAT[a * NL + c] *= lg_dlrelu(G[a * NL + c]);       // d G
            }
            __syncthreads();
            for (int i = tid; i < N * p2; i += LG_GB) {
                const int n = i / p2, c = i - n * p2;
                float a = dE[n * EL + c];
                for (int k = 0; k < N; ++k) a = fmaf(dAT[n * NL + k] + dAT[k * NL + n], E[k * EL + c], a);
                dCE[n * EL + c] = a;                                // (d E complete, over d CE)
            }
            __syncthreads();
            if (ST) {
#pragma unroll
                for (int k = 0; k < LGB_RWN; ++k) {
                    const int i = tid + k * LG_GB;
                    if (i < p2 * p) {
                        const int c = i / p, j = i - c * p;
                        float a = 0.f;
                        for (int n = 0; n < N; ++n) a = fmaf(dCE[n * EL + c], X[n * XL + j], a);
                        rWn[ST ? k : 0] += a;
                    }
                }
            } else {
                for (int i = tid; i < p2 * p; i += LG_GB) {
                    const int c = i / p, j = i - c * p;
                    float a = 0.f;
                    for (int n = 0; n < N; ++n) a = fmaf(dCE[n * EL + c], X[n * XL + j], a);
                    aWn[i] += a;
                }
            }
            for (int c = tid; c < p2; c += LG_GB) {
                float a = 0.f;
                for (int n = 0; n < N; ++n) a += dCE[n * EL + c];
                abn[c] += a;
            }
            __syncthreads();
        }
        // the A_G products are per sample: g W_Z_G = (sum_t d z_pre)^T A_G, and so for W_R_G, W_h_T
        for (int i = tid; i < N * N; i += LG_GB) {
            const int j = i / N, k = i - j * N;
            float az = 0.f, ar = 0.f, ah = 0.f;
            for (int r = 0; r < N; ++r) {
                const float ag = AG[r * NL + k];
                az = fmaf(SZ[r * NL + j], ag, az);
                ar = fmaf(SR[r * NL + j], ag, ar);
                ah = fmaf(SH[r * NL + j], ag, ah);
            }
            aF[1 * fs + i] += az; aF[3 * fs + i] += ar; aF[4 * fs + i] += ah;
        }
    }
    __syncthreads();
    // (the biases of a pair of Linears that are added meet the same gradient: W_Z_G's = W_Z_T's, W_R_G's = W_R_T's, W_h_T's = W_h's)
    float* row = part + (int64_t)blockIdx.x * g.CW;
    for (int i = tid; i < g.nB; i += LG_GB) {
        const int f = i / fs, e = i - f * fs;
        row[g.nA + i] = aF[e >= N * N ? (f == 1 ? 0 : f == 3 ? 2 : f == 4 ? 5 : f) * fs + e : i];
    }
    if (ST) {
#pragma unroll
        for (int k = 0; k < LGB_RWN; ++k) {
            const int i = tid + k * LG_GB;
            if (i < p2 * p) row[i] = rWn[ST ? k : 0];
        }
#pragma unroll
        for (int k = 0; k < LGB_RTH; ++k) {
            const int i = tid + k * LG_GB;
            if (i < p3 * p2) row[p2 * p + p2 + i] = rTh[ST ? k : 0];
        }
        for (int c = tid; c < p2; c += LG_GB) row[p2 * p + c] = abn[c];
        for (int o = tid; o < p3; o += LG_GB) row[p2 * p + p2 + p3 * p2 + o] = aThb[o];
    } else {
        for (int i = tid; i < g.nA; i += LG_GB) row[i] = acc[i];
    }
}

template <bool ST>
__global__ __launch_bounds__(LG_GB) void lg_graph_bwd(LgGeom g, const float* __restrict__ x, const float* __restrict__ prm, const float* __restrict__ dhg,
                                                      const float* __restrict__ glv, float coef, float gamma, float* __restrict__ part) {
    lg_graph_bwd_body<ST>(g, x, prm, dhg, glv, coef, gamma, part);
}

// (grid x = LgGeom::rows, as the single kernel's: a run's partial rows hold the single call's sums)
__global__ __launch_bounds__(LG_GB) void lg_graph_bwd_group(LgGeom g, LgGroupTable tab) {
    const LgGroup& r = tab.grp[blockIdx.y];
    lg_graph_bwd_body<false>(g, r.x, r.prm, r.dhg, r.glv, r.coef, r.gamma, r.part);
}

// ---- inter-layer passes -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float lg_keep(uint32_t ctr, uint32_t key, uint32_t thr, float scale) {
    return scale == 0.f ? 1.f : (lowbias32(ctr ^ key) >= thr ? scale : 0.f);
}

// v [q][b][W] *= keep (the forward's dropout behind bi_lstm2 and, with the same key, its backward)
__global__ void lg_drop_kernel(int64_t n, float* __restrict__ v, uint32_t key, uint32_t thr, float scale) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        v[i] *= lg_keep((uint32_t)(i & 0xFFFFFFFFll), key, thr, scale);
}

// forward: td [b][q][W] = leaky(keep o3[q][b][W]); backward: do3 [q][b][W] = dtd[b][q][W] leaky'(td) keep
template <bool BWD>
__global__ void lg_close_kernel(int64_t B, int Q, int W, const float* __restrict__ src, const float* __restrict__ td_in, float* __restrict__ dst,
                                uint32_t key, uint32_t thr, float scale) {
    const int64_t n = B * Q * W;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int j = (int)(i % W);
        const int64_t qb = i / W, q = qb / B, b = qb - q * B;           // i over [q][b][j]
        const int64_t it = (b * Q + q) * W + j;
        const float k = lg_keep((uint32_t)(i & 0xFFFFFFFFll), key, thr, scale);
        if (BWD) dst[i] = src[it] * lg_dlrelu(td_in[it]) * k;
        else dst[it] = lg_lrelu(src[i] * k);
    }
}

// ---- head ---------------------------------------------------------------------------------------------------------------------------------
// a1 = relu(pre1 + b1) in place, a2 = relu(W2 a1 + b2), pred = wc . a2 + bc; with y the squared-error share and d loss / d pred
__global__ void lg_head_kernel(LgGeom g, const float* __restrict__ prm, float* __restrict__ pre1, float* __restrict__ a2o, const float* __restrict__ y,
                               float* __restrict__ pred, float* __restrict__ sq, float* __restrict__ dpred, float inv_gb) {
    for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < g.B; b += (int64_t)gridDim.x * blockDim.x) {
        float a1[LG_F1];
#pragma unroll
        for (int k = 0; k < LG_F1; ++k) {
            a1[k] = lg_relu(pre1[b * LG_F1 + k] + prm[g.o_f1b + k]);
            pre1[b * LG_F1 + k] = a1[k];
        }
        float pv = prm[g.o_cb];
#pragma unroll
        for (int i = 0; i < LG_F2; ++i) {
            float a = prm[g.o_f2b + i];
#pragma unroll
            for (int k = 0; k < LG_F1; ++k) a = fmaf(a1[k], prm[g.o_f2w + i * LG_F1 + k], a);
            a = lg_relu(a);
            a2o[b * LG_F2 + i] = a;
            pv = fmaf(a, prm[g.o_cw + i], pv);
        }
        pred[b] = pv;
        if (y) {
            const float df = pv - y[b];
            sq[b] = df * df * inv_gb;
            dpred[b] = 2.f * df * inv_gb;
        }
    }
}

// prod [b] = [g fc1.bias | g fc2.weight | g fc2.bias | g cls.weight | g cls.bias] of the sample; dpre1 [b][16]
__global__ void lg_head_bwd_kernel(LgGeom g, const float* __restrict__ prm, const float* __restrict__ a1g, const float* __restrict__ a2g,
                                   const float* __restrict__ dpred, float* __restrict__ prod, float* __restrict__ dpre1) {
    for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < g.B; b += (int64_t)gridDim.x * blockDim.x) {
        const float dp = dpred[b];
        float* row = prod + b * LG_HEADROW;
        float a1[LG_F1], da1[LG_F1];
#pragma unroll
        for (int k = 0; k < LG_F1; ++k) { a1[k] = a1g[b * LG_F1 + k]; da1[k] = 0.f; }
#pragma unroll
        for (int i = 0; i < LG_F2; ++i) {
            const float a2 = a2g[b * LG_F2 + i];
            const float d2 = a2 > 0.f ? dp * prm[g.o_cw + i] : 0.f;
#pragma unroll
            for (int k = 0; k < LG_F1; ++k) {
                row[LG_F1 + i * LG_F1 + k] = d2 * a1[k];
                da1[k] = fmaf(d2, prm[g.o_f2w + i * LG_F1 + k], da1[k]);
            }
            row[LG_F1 + LG_F2 * LG_F1 + i] = d2;
            row[LG_F1 + LG_F2 * LG_F1 + LG_F2 + i] = dp * a2;
        }
        row[LG_HEADROW - 1] = dp;
#pragma unroll
        for (int k = 0; k < LG_F1; ++k) {
            const float d1 = a1[k] > 0.f ? da1[k] : 0.f;
            row[k] = d1;
            dpre1[b * LG_F1 + k] = d1;
        }
    }
}

// One workgroup, fixed order: glv = {L_GL, S1, S2} from the samples' sums; with sq, loss = sum(sq) + theta L_GL
__global__ __launch_bounds__(LG_GB) void lg_loss_kernel(int64_t B, double cnt, float theta, float gamma, const float* __restrict__ glpart,
                                                        const float* __restrict__ sq, float* __restrict__ glv, float* __restrict__ gl_out,
                                                        float* __restrict__ loss) {
    __shared__ float red[3][LG_GB];
    const int tid = threadIdx.x;
    float s1 = 0.f, s2 = 0.f, s3 = 0.f;
    for (int64_t b = tid; b < B; b += LG_GB) {
        s1 += glpart[2 * b];
        s2 += glpart[2 * b + 1];
        if (sq) s3 += sq[b];
    }
    red[0][tid] = s1; red[1][tid] = s2; red[2][tid] = s3;
    __syncthreads();
    if (tid == 0) {
        float t1 = 0.f, t2 = 0.f, t3 = 0.f;
        for (int i = 0; i < LG_GB; ++i) { t1 += red[0][i]; t2 += red[1][i]; t3 += red[2][i]; }
        const float gl = (float)((double)t1 / cnt + (double)gamma * sqrt((double)t2 / cnt));
        glv[0] = gl; glv[1] = t1; glv[2] = t2;
        if (gl_out) gl_out[0] = gl;
        if (sq && loss) loss[0] = t3 + theta * gl;
    }
}

int64_t lg_tap_offset(const LgGeom& g, int which) {
    switch (which) {
        case 0: return g.w_hg;
        case 1: return g.w_td;
        case 2: return g.w_gl;
        default: return -1;
    }
}

int lg_run(const LgGeom& g, const rulgnn_logo_args* a, int mode, hipStream_t st);

}  // namespace

// RULGNN_OK, or the code every entry returns for a refused shape: lg_geometry's own.
int Logo::shape_status(const Shape* s) {
    LgGeom g;
    return lg_geometry(s, &g);
}

int64_t Logo::param_count(const Shape* s) {
    LgGeom g;
    return lg_geometry(s, &g) == RULGNN_OK ? g.pcount : -1;
}

size_t Logo::workspace_bytes(const Shape* s) {
    LgGeom g;
    return lg_geometry(s, &g) == RULGNN_OK ? g.total_bytes : 0;
}

int64_t Logo::tap_offset(const Shape* s, int which) {
    LgGeom g;
    return lg_geometry(s, &g) == RULGNN_OK ? lg_tap_offset(g, which) : -1;
}

int Logo::run(const Shape* s, const Args* a, int mode, hipStream_t st) {
    LgGeom g;
    RULGNN_TRY(lg_geometry(s, &g));
    return lg_run(g, a, mode, st);
}

// ---- LOGO_bearing: the same chain behind lgb_geometry ----------------------------------------------------------------------------------------
int Logob::shape_status(const Shape* s) {
    LgGeom g;
    return lgb_geometry(s, &g);
}

int64_t Logob::param_count(const Shape* s) {
    LgGeom g;
    return lgb_geometry(s, &g) == RULGNN_OK ? g.pcount : -1;
}

size_t Logob::workspace_bytes(const Shape* s) {
    LgGeom g;
    return lgb_geometry(s, &g) == RULGNN_OK ? g.total_bytes : 0;
}

int64_t Logob::tap_offset(const Shape* s, int which) {
    LgGeom g;
    return lgb_geometry(s, &g) == RULGNN_OK ? lg_tap_offset(g, which) : -1;
}

int Logob::run(const Shape* s, const Args* a, int mode, hipStream_t st) {
    LgGeom g;
    RULGNN_TRY(lgb_geometry(s, &g));
    return lg_run(g, a, mode, st);
}

namespace {

// One run's view of a call: its workspace, parameters and dropout constants.  The per-run stages below are what lg_run and lg_run_group
// enqueue around the graph kernels and the recurrences, which the one launches per run and the other once for all runs.
struct LgRun {
    const rulgnn_logo_args* a;
    float* ws;
    const float* prm;
    bool drop;
    uint32_t thr, key2, key3;
    float dscale;
};

LgRun lg_run_of(const rulgnn_logo_args* a) {
    LgRun r{};
    r.a = a;
    r.ws = static_cast<float*>(a->workspace);
    r.prm = a->params;
    r.drop = a->training && a->dropout_p > 0.f;
    const DropoutConst dc = dropout_const(r.drop ? a->dropout_p : 0.f);
    r.thr = dc.thr;
    r.dscale = r.drop ? dc.scale : 0.f;
    r.key2 = dropout_layer_key(a->seed, a->step, 0);
    r.key3 = dropout_layer_key(a->seed, a->step, 1);
    return r;
}

// layer l of the run's temporal stack; bwd: with d out, d x and the gradients
void lg_lstm_args(const LgGeom& g, const LgRun& r, int l, bool bwd, rulgnn_bilstm_shape* ls, rulgnn_bilstm_args* la) {
    float* ws = r.ws;
    float* const lin[3] = {ws + g.w_hg, ws + g.w_o1, ws + g.w_o2};
    float* const lout[3] = {ws + g.w_o1, ws + g.w_o2, ws + g.w_o3};
    float* const ldout[3] = {ws + g.w_do1, ws + g.w_do2, ws + g.w_do3};
    float* const ldx[3] = {ws + g.w_dhg, ws + g.w_do1, ws + g.w_do2};
    const LgLstm& k = g.lstm[l];
    *ls = rulgnn_bilstm_shape{g.B, g.Q, k.I, k.H};
    *la = rulgnn_bilstm_args{};
    la->x = lin[l];
    la->out = lout[l];
    for (int d = 0; d < 2; ++d) {
        la->w_ih[d] = r.prm + k.o_wih[d]; la->w_hh[d] = r.prm + k.o_whh[d]; la->b_ih[d] = r.prm + k.o_bih[d]; la->b_hh[d] = r.prm + k.o_bhh[d];
    }
    la->workspace = ws + k.w_ws;
    la->workspace_bytes = k.ws_bytes;
    if (bwd) {
        float* gr = r.a->grads;
        la->dout = ldout[l];
        la->dx = ldx[l];
        for (int d = 0; d < 2; ++d) {
            la->dw_ih[d] = gr + k.o_wih[d]; la->dw_hh[d] = gr + k.o_whh[d]; la->db_ih[d] = gr + k.o_bih[d]; la->db_hh[d] = gr + k.o_bhh[d];
        }
    }
}

// dropout behind bi_lstm2: o2 in the forward, with the same key d o2 in the backward
int lg_mid_drop(const LgGeom& g, const LgRun& r, float* v, hipStream_t st) {
    if (!r.drop) return RULGNN_OK;
    const int64_t n = (int64_t)g.Q * g.B * g.H2;
    return launch_checked(lg_drop_kernel, dim3(lg_blocks(n)), dim3(LG_GB), 0, st, n, v, r.key2, r.thr, r.dscale);
}

// behind the temporal stack: closing pass, fc1, head and loss
int lg_head_fwd(const LgGeom& g, const LgRun& r, hipStream_t st) {
    const rulgnn_logo_args* a = r.a;
    float* ws = r.ws;
    const float* prm = r.prm;
    const int64_t B = g.B, gb = a->global_batch > 0 ? a->global_batch : B, QB = (int64_t)g.Q * B;
    const int Q = g.Q, H1 = g.H1, K1 = g.K1;
    const double cnt = (double)B * g.T * g.N * g.N;
    RULGNN_TRY(launch_checked(lg_close_kernel<false>, dim3(lg_blocks(QB * H1)), dim3(LG_GB), 0, st, B, Q, H1, (const float*)(ws + g.w_o3), (const float*)nullptr,
                              ws + g.w_td, r.key3, r.thr, r.dscale));
    // pre1 [B][16] = td [B][Q 3h] fc1^T: a few tiles over k = Q 3h, in fixed slices
    RULGNN_TRY(sgemm_splitk(ws + g.w_td, K1, 1, prm + g.o_f1w, K1, 1, ws + g.w_pre1, LG_F1, (int)B, LG_F1, K1, false, ws + g.w_split, st));
    RULGNN_TRY(launch_checked(lg_head_kernel, dim3(lg_blocks(B, 4096)), dim3(LG_GB), 0, st, g, prm, ws + g.w_pre1, ws + g.w_a2, a->y, a->pred, ws + g.w_sq,
                              ws + g.w_dpred, 1.0f / (float)gb));
    return launch_checked(lg_loss_kernel, dim3(1), dim3(LG_GB), 0, st, B, cnt, a->theta, a->gamma, (const float*)(ws + g.w_glpart),
                          a->y ? (const float*)(ws + g.w_sq) : (const float*)nullptr, ws + g.w_gl, a->loss_gl, a->loss);
}

// in front of the temporal stack's backward: the head's gradients, d td and the closing pass's backward
int lg_head_bwd(const LgGeom& g, const LgRun& r, hipStream_t st) {
    const rulgnn_logo_args* a = r.a;
    float* ws = r.ws;
    const float* prm = r.prm;
    const int64_t B = g.B, QB = (int64_t)g.Q * B;
    const int Q = g.Q, H1 = g.H1, K1 = g.K1;
    const float* dpred = a->dpred ? a->dpred : ws + g.w_dpred;
    float* gr = a->grads;
    RULGNN_TRY(launch_checked(lg_head_bwd_kernel, dim3(lg_blocks(B, 4096)), dim3(LG_GB), 0, st, g, prm, (const float*)(ws + g.w_pre1), (const float*)(ws + g.w_a2),
                              dpred, ws + g.w_prod, ws + g.w_dpre1));
    // [g fc1.bias .. g cls.bias] = the samples' rows in order (contiguous in the parameter layout)
    RULGNN_TRY(rows_sum(ws + g.w_prod, (int)B, LG_HEADROW, LG_HEADROW, gr + g.o_f1b, st));
    // g fc1.weight [16][Q 3h] = dpre1^T td (k = the batch, one fixed-order product); dtd = dpre1 fc1
    RULGNN_TRY(sgemm(ws + g.w_dpre1, 1, LG_F1, ws + g.w_td, 1, K1, gr + g.o_f1w, K1, LG_F1, K1, (int)B, false, st));
    RULGNN_TRY(sgemm(ws + g.w_dpre1, LG_F1, 1, prm + g.o_f1w, 1, K1, ws + g.w_dtd, K1, (int)B, K1, LG_F1, false, st));
    return launch_checked(lg_close_kernel<true>, dim3(lg_blocks(QB * H1)), dim3(LG_GB), 0, st, B, Q, H1, (const float*)(ws + g.w_dtd),
                          (const float*)(ws + g.w_td), ws + g.w_do3, r.key3, r.thr, r.dscale);
}

// behind the graph backward: the partial rows' two blocks, added in a fixed order
int lg_graph_sums(const LgGeom& g, const LgRun& r, hipStream_t st) {
    float* gr = r.a->grads;
    RULGNN_TRY(rows_sum(r.ws + g.w_part, g.rows, g.CW, g.nA, gr + g.o_wn, st));
    return rows_sum(r.ws + g.w_part + g.nA, g.rows, g.CW, g.nB, gr + g.o_fu, st);
}

// mode bit 0: forward, bit 1: backward (after a forward with the same args / workspace)
int lg_run(const LgGeom& g, const rulgnn_logo_args* a, int mode, hipStream_t st) {
    if (a->workspace_bytes < g.total_bytes) return RULGNN_EWORKSPACE;
    if (g.B == 0) return RULGNN_OK;
    const LgRun r = lg_run_of(a);
    float* ws = r.ws;
    const int64_t B = g.B;
    if (mode & 1) {
        const auto graph_fwd = g.ns > 0 ? lg_graph_fwd<true> : lg_graph_fwd<false>;
        RULGNN_TRY(allow_dynamic_lds(graph_fwd, g.lds_fwd));
        RULGNN_TRY(launch_checked(graph_fwd, dim3((unsigned)(B > 8192 ? 8192 : B)), dim3(LG_GB), g.lds_fwd, st, g, a->x, r.prm, ws + g.w_hg, ws + g.w_glpart));
        for (int l = 0; l < 3; ++l) {
            rulgnn_bilstm_shape ls;
            rulgnn_bilstm_args la;
            lg_lstm_args(g, r, l, false, &ls, &la);
            RULGNN_TRY(bilstm_forward(&ls, &la, st, 2));
            if (l == 1) RULGNN_TRY(lg_mid_drop(g, r, ws + g.w_o2, st));
        }
        RULGNN_TRY(lg_head_fwd(g, r, st));
    }
    if (mode & 2) {
        if (!a->grads) return RULGNN_EINVAL;
        RULGNN_TRY(lg_head_bwd(g, r, st));
        for (int l = 2; l >= 0; --l) {
            rulgnn_bilstm_shape ls;
            rulgnn_bilstm_args la;
            lg_lstm_args(g, r, l, true, &ls, &la);
            RULGNN_TRY(bilstm_backward(&ls, &la, st, 2));
            if (l == 2) RULGNN_TRY(lg_mid_drop(g, r, ws + g.w_do2, st));
        }
        const auto graph_bwd = g.ns > 0 ? lg_graph_bwd<true> : lg_graph_bwd<false>;
        RULGNN_TRY(allow_dynamic_lds(graph_bwd, g.lds_bwd));
        RULGNN_TRY(launch_checked(graph_bwd, dim3((unsigned)g.rows), dim3(LG_GB), g.lds_bwd, st, g, a->x, r.prm, (const float*)(ws + g.w_dhg),
                                  (const float*)(ws + g.w_gl), a->theta, a->gamma, ws + g.w_part));
        RULGNN_TRY(lg_graph_sums(g, r, st));
    }
    return RULGNN_OK;
}

// The fused step (mode 3) of `n` runs of one LOGO shape: the graph forward, each layer's recurrences (bilstm_forward_group /
// bilstm_backward_group) and the graph backward are one grouped launch each for all runs; the dropout passes, the head and the sums
// follow per run in run order, with lg_run's arguments.  The graph backward's grid x stays LgGeom::rows, which fixes each run's
// summation order.  The entry has checked every group.
int lg_run_group(const LgGeom& g, const rulgnn_logo_args* groups, int n, hipStream_t st) {
    if (n < 1 || n > STEP_MAX_GROUPS || g.ns > 0) return RULGNN_EINVAL;
    for (int i = 0; i < n; ++i) {
        if (groups[i].workspace_bytes < g.total_bytes) return RULGNN_EWORKSPACE;
        if (!groups[i].grads) return RULGNN_EINVAL;
    }
    if (g.B == 0) return RULGNN_OK;
    LgRun runs[STEP_MAX_GROUPS];
    LgGroupTable tab{};
    for (int i = 0; i < n; ++i) {
        const LgRun& r = runs[i] = lg_run_of(&groups[i]);
        float* ws = r.ws;
        tab.grp[i] = LgGroup{groups[i].x, r.prm, ws + g.w_hg, ws + g.w_glpart, ws + g.w_dhg, ws + g.w_gl, ws + g.w_part, groups[i].theta, groups[i].gamma};
    }
    const int64_t B = g.B;
    const unsigned ny = (unsigned)n;
    rulgnn_bilstm_shape ls;
    rulgnn_bilstm_args la[STEP_MAX_GROUPS];
    RULGNN_TRY(allow_dynamic_lds(lg_graph_fwd_group, g.lds_fwd));
    RULGNN_TRY(launch_checked(lg_graph_fwd_group, dim3((unsigned)(B > 8192 ? 8192 : B), ny), dim3(LG_GB), g.lds_fwd, st, g, tab));
    for (int l = 0; l < 3; ++l) {
        for (int i = 0; i < n; ++i) lg_lstm_args(g, runs[i], l, false, &ls, &la[i]);
        RULGNN_TRY(bilstm_forward_group(&ls, la, n, st));
        if (l == 1)
            for (int i = 0; i < n; ++i) RULGNN_TRY(lg_mid_drop(g, runs[i], runs[i].ws + g.w_o2, st));
    }
    for (int i = 0; i < n; ++i) RULGNN_TRY(lg_head_fwd(g, runs[i], st));
    for (int i = 0; i < n; ++i) RULGNN_TRY(lg_head_bwd(g, runs[i], st));
    for (int l = 2; l >= 0; --l) {
        for (int i = 0; i < n; ++i) lg_lstm_args(g, runs[i], l, true, &ls, &la[i]);
        RULGNN_TRY(bilstm_backward_group(&ls, la, n, st));
        if (l == 2)
            for (int i = 0; i < n; ++i) RULGNN_TRY(lg_mid_drop(g, runs[i], runs[i].ws + g.w_do2, st));
    }
    RULGNN_TRY(allow_dynamic_lds(lg_graph_bwd_group, g.lds_bwd));
    RULGNN_TRY(launch_checked(lg_graph_bwd_group, dim3((unsigned)g.rows, ny), dim3(LG_GB), g.lds_bwd, st, g, tab));
    for (int i = 0; i < n; ++i) RULGNN_TRY(lg_graph_sums(g, runs[i], st));
    return RULGNN_OK;
}

}  // namespace

int Logo::run_group(const Shape* s, const Args* groups, int n, hipStream_t st) {
    LgGeom g;
    RULGNN_TRY(lg_geometry(s, &g));
    return lg_run_group(g, groups, n, st);
}

}  // namespace rulgnn
