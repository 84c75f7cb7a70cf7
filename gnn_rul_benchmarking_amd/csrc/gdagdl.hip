// GDAGDL on gfx950: STNet's front end and back end around a graph-attention stage.
// Reference path replaced: GDAGDL_model.forward -- models/GDAGDL/Model.py:66-170 (GraphAttentionLayer :6-39, pcc_graph_construction
// :42-63) -- and GDAGDL.update, algorithms/algorithms.py:519-544 (loss = MSE(pred, y) + the auto-encoder's reconstruction MSE).
//
//   x [bs, T * P] -> per (sample, patch) graph: mag = |STFT| (stft_device.hpp) = N frequency nodes x f frames -> the reference's
//   "Pearson" matrix of the nodes over the frames: c = mag - mean_f(mag), pcc = (c reshape(c, [f, N])) / (|c_i| |c_j|) -- the second
//   operand is the tile reshaped, not transposed (Model.py:51), a quirk kept because the mask, and with it every prediction, follows
//   from it; no epsilon: an all-zero patch gives 0 / 0 = NaN -> ni = pcc (mag w_ni + b_ni) -> m = (ni > 0), adjacency
//   M = m m^T (NaN > 0 is false: a NaN graph is masked out) -> L GAT layers: Z = h W^T + b, u_ij = a1 . Z_i + a2 . Z_j + b_att,
//   Pm = softmax_j(leakyrelu(u, 0.1)), Q = Pm o D o M (D: dropout keep mask / (1 - p), train mode), h = ELU(Q Z) -> Y_o [bs, T, N C_L] ->
//   auto-encoder (4 + 4 Linear layers, widths D -> A -> A/2 -> A/4 -> O and back; reconstruction MSE is a loss term) -> LSTM over the T
//   patches -> Linear.
//
// Launches: one front-end kernel per call (gd_front_kernel: magnitude, Pearson matrix, ni and m from the N x f tile in LDS; pcc never
// leaves LDS); per layer one matrix-core GEMM for h W^T (the bias is added where Z is read) and ONE fused attention kernel (gd_att_fwd:
// a wavefront per graph, Z of the graph and everything N x N in LDS); backward per layer one fused kernel (gd_att_bwd: recomputes
// s .. Q from the saved Z, writes dZ and one partial row [da1 | da2 | db_att] per wavefront, summed in a fixed order by rows_sum) and the
// GEMMs dW = dZ^T h, db = sum dZ, dh = dZ W.  Between launches only mag, m, ni, Z_l, h_l, dZ and dh exist: nothing N x N, nothing
// pair-shaped.  No floating-point atomics; the partial-row count is fixed by the launch geometry, so two runs give the same bits.
// The mask has no gradient: node_importance_linear.{weight, bias} (the first f + 1 floats of the flat buffer) get zeros.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sgemm_mfma.hpp"
#include "families_host.hpp"       // (stgcn_host.hpp: dropout_layer_key)
#include "stgcn_device.hpp"        // lowbias32
#include "stft_device.hpp"         // SB, the STFT magnitude
#include "seq_backend.hpp"         // the auto-encoder, the LSTM and the head (shared with stnet.hip and gatlstm.hip)

namespace rulgnn {

namespace {

constexpr int GD_MAXL = RULGNN_GDAGDL_MAX_LAYERS, GD_MAXC = RULGNN_GDAGDL_MAX_WIDTH, GD_MAXNODE = RULGNN_GDAGDL_MAX_NPERSEG / 2 + 1;
constexpr int GD_WAVE = 64, GD_MAXWAVES = 4, GD_CHUNKS = GD_MAXC / GD_WAVE;
constexpr int GD_ATT_MAXGRID = 1024;
constexpr float GD_SLOPE = 0.1f;                // Model.py:7 alpha

struct GdGeom {
    int64_t B, G, R, BT;                        // samples, graphs = B * T, node rows = G * N, patch rows = B * T
    int T, P, nseg, N, f, nl, A, O, E;
    int C[GD_MAXL + 1];                         // channel widths: f, gat_layer_dim...
    int D;                                      // N * C[last]: auto-encoder width
    // flat parameter offsets of the front end and the GAT layers (the two gradless tensors first); the back end's are the plans'
    int o_niw, o_nib, o_w[GD_MAXL], o_b[GD_MAXL], o_aw[GD_MAXL], o_ab[GD_MAXL], pcount;
    AutoEncoderPlan ae;                         // D -> A -> A/2 -> A/4 -> O and back
    LstmHeadPlan lh;                            // one LSTM O -> E over the T patches, Linear(E * T, 1)
    // workspace offsets (floats)
    int64_t w_wal[GD_MAXL];                     // 16-byte aligned copies of the projection weights (see Gdagdl::run)
    int64_t w_mag, w_ni, w_mask, w_z[GD_MAXL], w_h[GD_MAXL], w_dz, w_dh, w_dhs, w_part, w_split, total;
};

// ---- LDS layouts, stated once for kernel and launcher (floats) -------------------------------------------------------------------
// Front end: the STFT's staging area, the magnitude tile [N][f], lin [N], norm [N], pcc [N][N].
__host__ __device__ inline size_t gd_front_lds_floats(int P, int ns, int N, int f) {
    return stft_lds_floats(P, ns) + (size_t)N * f + 2 * (size_t)N + (size_t)N * N;
}
// Attention, per wavefront (= per graph in flight).  Rows of Z / dH' are padded to an odd stride so that lanes walking different rows hit
// different banks.  forward: Z [N][Cs], s, t, m [N] each, Q [N][N]; backward: Z, dH' [N][Cs], s, t, m, ds, dt [N] each and four N x N
// tiles (Pm then Q, D o M, leakyrelu', dQ then du).
__host__ __device__ inline int gd_row_stride(int C) { return C | 1; }
__host__ __device__ inline size_t gd_att_lds_floats(int N, int C, bool bwd) {
    const size_t zs = (size_t)N * gd_row_stride(C), nn = (size_t)N * N;
    return bwd ? 2 * zs + 5 * (size_t)N + 4 * nn : zs + 3 * (size_t)N + nn;
}
// wavefronts (graphs in flight) per workgroup: what one compute unit's LDS holds, at most GD_MAXWAVES; 0: does not fit
inline int gd_att_waves(int N, int C, bool bwd) {
    const size_t v = MAX_LDS_BYTES / (gd_att_lds_floats(N, C, bwd) * sizeof(float));
    return v > (size_t)GD_MAXWAVES ? GD_MAXWAVES : (int)v;
}

int gd_geometry(const rulgnn_gdagdl_shape* s, GdGeom* g) {
    if (!s) return RULGNN_EINVAL;
    if (s->batch < 0 || s->num_patch < 1 || s->patch_size < 2 || s->nperseg < 2 || s->num_gat < 1 || s->lstm_hidden_dim < 1 ||
        s->autoencoder_hidden_dim < 4 || s->autoencoder_out_dim < 1)
        return RULGNN_EINVAL;
    if (s->num_gat > GD_MAXL || s->nperseg > RULGNN_GDAGDL_MAX_NPERSEG || (s->nperseg & 1) || s->patch_size % s->nperseg != 0 ||
        s->patch_size <= s->nperseg / 2)
        return RULGNN_EUNSUPPORTED;              // reflect padding needs more than nperseg / 2 points; frames = 1 + P / nperseg
    g->B = s->batch; g->T = s->num_patch; g->P = s->patch_size; g->nseg = s->nperseg;
    g->N = s->nperseg / 2 + 1;
    g->f = 1 + s->patch_size / s->nperseg;
    if (g->f > RULGNN_GDAGDL_MAX_FRAMES) return RULGNN_EUNSUPPORTED;
    if (s->num_nodes != g->N || s->input_dim != g->f) return RULGNN_EINVAL;         // the reference's kwargs must describe the STFT's shape
    g->nl = s->num_gat; g->A = s->autoencoder_hidden_dim; g->O = s->autoencoder_out_dim; g->E = s->lstm_hidden_dim;
    g->C[0] = g->f;
    int cmax = 0;
    for (int i = 0; i < g->nl; ++i) {
        if (s->gat_layer_dim[i] < 1) return RULGNN_EINVAL;
        if (s->gat_layer_dim[i] > GD_MAXC) return RULGNN_EUNSUPPORTED;
        g->C[i + 1] = s->gat_layer_dim[i];
        if (g->C[i + 1] > cmax) cmax = g->C[i + 1];
        if (gd_att_waves(g->N, g->C[i + 1], true) < 1) return RULGNN_EUNSUPPORTED;
    }
    if (g->E > RULGNN_GDAGDL_MAX_LSTM_HIDDEN || g->A > RULGNN_GDAGDL_MAX_AE_WIDTH || g->O > RULGNN_GDAGDL_MAX_AE_WIDTH) return RULGNN_EUNSUPPORTED;
    if (gd_front_lds_floats(g->P, g->nseg, g->N, g->f) * sizeof(float) > DEFAULT_LDS_BYTES) return RULGNN_EUNSUPPORTED;
    g->G = g->B * g->T; g->R = g->G * g->N; g->BT = g->G;
    g->D = g->N * g->C[g->nl];
    if (g->R * (int64_t)(cmax > g->f ? cmax : g->f) > 0x7fffffff) return RULGNN_EUNSUPPORTED;      // the GEMMs take int extents
    const int A = g->A, D = g->D, O = g->O;
    int o = 0;
    int64_t w = 0;
    SplitKScratch sp(1024);
    auto tk = [&](int n) { const int r = o; o += n; return r; };
    auto wk = [&](int64_t n) { const int64_t r = w; w += (n + 63) & ~(int64_t)63; return r; };
    g->o_niw = tk(g->f); g->o_nib = tk(1);
    for (int i = 0; i < g->nl; ++i) {
        g->o_w[i] = tk(g->C[i + 1] * g->C[i]); g->o_b[i] = tk(g->C[i + 1]);
        g->o_aw[i] = tk(2 * g->C[i + 1]); g->o_ab[i] = tk(1);
    }
    const int64_t R = g->R, BT = g->BT;
    g->w_mag = wk(R * g->f); g->w_ni = wk(R); g->w_mask = wk(R);
    for (int i = 0; i < g->nl; ++i) { g->w_z[i] = wk(R * g->C[i + 1]); g->w_h[i] = wk(R * g->C[i + 1]); }
    const int ein[4] = {D, A, A / 2, A / 4}, eout[4] = {A, A / 2, A / 4, O}, din[4] = {O, A / 4, A / 2, A}, dout[4] = {A / 4, A / 2, A, D};
    g->ae.BT = BT;
    for (int i = 0; i < 4; ++i) { g->ae.ein[i] = ein[i]; g->ae.eout[i] = eout[i]; g->ae.din[i] = din[i]; g->ae.dout[i] = dout[i]; }
    autoencoder_layout(&g->ae, &o, &w, &sp);
    g->lh.B = g->B; g->lh.T = g->T; g->lh.nk = 1; g->lh.H[0] = O; g->lh.H[1] = g->E;
    RULGNN_TRY(lstm_head_layout(&g->lh, &o, &w, &sp));
    g->pcount = o;
    g->w_dz = wk(R * cmax); g->w_dh = wk(R * cmax);
    g->w_dhs = wk(BT * g->E);
    g->w_part = wk((int64_t)GD_ATT_MAXGRID * GD_MAXWAVES * (2 * cmax + 1));
    for (int i = 0; i < g->nl; ++i) g->w_wal[i] = wk((int64_t)g->C[i] * g->C[i + 1]);
    for (int i = 0; i < g->nl; ++i) { sp.need(g->C[i + 1], g->C[i], R); sp.need(1, g->C[i + 1], R); }
    g->w_split = wk((int64_t)sp.floats());
    g->total = w;
    return RULGNN_OK;
}

// ---- front end: STFT magnitude, Pearson matrix, node importance, mask: one workgroup per (sample, patch) ------------------------------
__global__ __launch_bounds__(SB) void gd_front_kernel(GdGeom g, const float* __restrict__ x, const float* __restrict__ prm, float* __restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int P = g.P, ns = g.nseg, N = g.N, f = g.f, tid = threadIdx.x;
    const StftLds l = stft_carve(sm, P, ns);
    float* mg = l.end;                    // [N][f] magnitude, then centred in place
    float* lin = mg + N * f;              // [N] mag_j . w_ni + b_ni
    float* nrm = lin + N;                 // [N] || centred row ||
    float* pc = nrm + N;                  // [N][N] Pearson matrix
    stft_tables(l, ns, tid);
    for (int64_t gi = blockIdx.x; gi < g.G; gi += gridDim.x) {
        stft_load_patch(l, x + gi * P, P, ns, tid);
        __syncthreads();
        for (int i = tid; i < N * f; i += SB) {
            const float a = stft_magnitude(l, ns, i / f, i % f);
            mg[i] = a;
            ws[g.w_mag + gi * N * f + i] = a;
        }
        __syncthreads();
        if (tid < N) {
            float* row = mg + tid * f;
            float li = 0.f, s = 0.f;
            for (int t = 0; t < f; ++t) { li = fmaf(row[t], prm[g.o_niw + t], li); s += row[t]; }
            lin[tid] = li + prm[g.o_nib];
            const float mean = s / (float)f;
            float q = 0.f;
            for (int t = 0; t < f; ++t) { const float c = row[t] - mean; row[t] = c; q = fmaf(c, c, q); }
            nrm[tid] = sqrtf(q);
        }
        __syncthreads();
        for (int i = tid; i < N * N; i += SB) {
            // The reference's second bmm operand is the centred tile RESHAPED to [f][N], not transposed (Model.py:51): kept
            const float *ra = mg + (i / N) * f, *rb = mg + (i % N);
            float d = 0.f;
            for (int t = 0; t < f; ++t) d = fmaf(ra[t], rb[t * N], d);
            pc[i] = d / (nrm[i / N] * nrm[i % N]);             // no epsilon: 0 / 0 = NaN on a constant row, as the reference
        }
        __syncthreads();
        if (tid < N) {
            float v = 0.f;
            for (int j = 0; j < N; ++j) v = fmaf(pc[tid * N + j], lin[j], v);
            ws[g.w_ni + gi * N + tid] = v;
            ws[g.w_mask + gi * N + tid] = v > 0.f ? 1.f : 0.f;   // NaN > 0 is false
        }
        __syncthreads();
    }
}

// ---- fused graph attention ----------------------------------------------------------------------------------------------------------
struct GdAtt {
    int64_t G, g0;                    // graphs of this call; global index of its first graph (dropout counters)
    int N, C, waves;
    const float *z, *bias, *att, *mask;      // Z [G N][C] without its bias, linear.bias [C], attention.{weight [2C], bias [1]} (adjacent), m [G N]
    float* h;                         // forward: ELU(Q Z) [G N][C] (written); backward: the same (read)
    const float* dh;                  // backward: d h
    float* dz;                        // backward: d Z
    float* part;                      // backward: [gridDim.x * waves][2 C + 1] partial rows [da1 | da2 | db_att]
    uint32_t key, thr;                // dropout: keep where lowbias32(counter ^ key) >= thr
    float scale;                      // 1 / (1 - p); 0: no dropout
};

__device__ __forceinline__ float gd_wave_sum(float v) {
#pragma unroll
    for (int m = GD_WAVE / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, GD_WAVE);
    return v;
}
__device__ __forceinline__ float gd_wave_max(float v) {
#pragma unroll
    for (int m = GD_WAVE / 2; m > 0; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, GD_WAVE));
    return v;
}
__device__ __forceinline__ float gd_keep(const GdAtt& q, int64_t gi, int i, int j) {
    if (q.scale == 0.f) return 1.f;
    const uint32_t ctr = (uint32_t)((((uint64_t)(q.g0 + gi) * q.N + i) * q.N) + j);
    return lowbias32(ctr ^ q.key) >= q.thr ? q.scale : 0.f;
}

// Z + bias of graph gi into zs [N][Cs]; its mask into m [N]
__device__ __forceinline__ void gd_load_graph(const GdAtt& q, int64_t gi, int lane, float* zs, float* m) {
    const int N = q.N, C = q.C, Cs = gd_row_stride(C);
    const float* zg = q.z + gi * N * C;
    for (int idx = lane; idx < N * C; idx += GD_WAVE) {
        const int i = idx / C, c = idx - i * C;
        zs[i * Cs + c] = zg[idx] + q.bias[c];
    }
    if (lane < N) m[lane] = q.mask[gi * N + lane];
}
// s_i = a1 . Z_i, t_i = a2 . Z_i (one wavefront; fixed order)
__device__ __forceinline__ void gd_scores(const GdAtt& q, int lane, const float* zs, float* s, float* t) {
    const int N = q.N, C = q.C, Cs = gd_row_stride(C);
    for (int i = 0; i < N; ++i) {
        float ps = 0.f, pt = 0.f;
        for (int c = lane; c < C; c += GD_WAVE) {
            const float zv = zs[i * Cs + c];
            ps = fmaf(q.att[c], zv, ps);
            pt = fmaf(q.att[C + c], zv, pt);
        }
        ps = gd_wave_sum(ps);
        pt = gd_wave_sum(pt);
        if (lane == 0) { s[i] = ps; t[i] = pt; }
    }
}
// row i of the softmax: lane j < N returns Pm_ij (and u_ij through *u); other lanes 0
__device__ __forceinline__ float gd_softmax_row(const GdAtt& q, int lane, int i, const float* s, const float* t, float* u) {
    const bool on = lane < q.N;
    const float uv = on ? s[i] + t[lane] + q.att[2 * q.C] : 0.f;
    const float e = on ? (uv > 0.f ? uv : GD_SLOPE * uv) : -INFINITY;
    const float mx = gd_wave_max(e);
    const float p = on ? expf(e - mx) : 0.f;
    const float sum = gd_wave_sum(p);
    *u = uv;
    return p / sum;
}

// A wavefront per graph, `q.waves` graphs in flight per workgroup (blockDim.x = 64 * waves); every wavefront of a workgroup walks the
// same number of rounds, so the barriers are uniform (a wavefront without a graph only waits).
__global__ __launch_bounds__(GD_WAVE * GD_MAXWAVES) void gd_att_fwd_kernel(GdAtt q) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int N = q.N, C = q.C, Cs = gd_row_stride(C), lane = threadIdx.x % GD_WAVE, w = threadIdx.x / GD_WAVE;
    float* zs = sm + (size_t)w * gd_att_lds_floats(N, C, false);
    float* s = zs + (size_t)N * Cs;
    float* t = s + N;
    float* m = t + N;
    float* Q = m + N;                                    // [N][N]
    for (int64_t base = (int64_t)blockIdx.x * q.waves; base < q.G; base += (int64_t)gridDim.x * q.waves) {
        const int64_t gi = base + w;
        const bool valid = gi < q.G;
        if (valid) gd_load_graph(q, gi, lane, zs, m);
        __syncthreads();
        if (valid) gd_scores(q, lane, zs, s, t);
        __syncthreads();
        if (valid)
            for (int i = 0; i < N; ++i) {
                float u;
                const float p = gd_softmax_row(q, lane, i, s, t, &u);
                if (lane < N) Q[i * N + lane] = p * gd_keep(q, gi, i, lane) * (m[i] * m[lane]);
            }
        __syncthreads();
        if (valid)
            for (int c = lane; c < C; c += GD_WAVE)
                for (int i = 0; i < N; ++i) {
                    float acc = 0.f;
                    for (int j = 0; j < N; ++j) acc = fmaf(Q[i * N + j], zs[j * Cs + c], acc);
                    q.h[(gi * N + i) * C + c] = acc > 0.f ? acc : expm1f(acc);          // ELU
                }
        __syncthreads();
    }
}

__global__ __launch_bounds__(GD_WAVE * GD_MAXWAVES) void gd_att_bwd_kernel(GdAtt q) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int N = q.N, C = q.C, Cs = gd_row_stride(C), lane = threadIdx.x % GD_WAVE, w = threadIdx.x / GD_WAVE;
    float* zs = sm + (size_t)w * gd_att_lds_floats(N, C, true);
    float* dhs = zs + (size_t)N * Cs;                    // dH' = dh o ELU'(H')
    float* s = dhs + (size_t)N * Cs;
    float* t = s + N;
    float* m = t + N;
    float* ds = m + N;
    float* dt = ds + N;
    float* Pq = dt + N;                                  // Pm, then Q = Pm o D o M
    float* DM = Pq + N * N;                              // D o M
    float* sl = DM + N * N;                              // leakyrelu'(u)
    float* dq = sl + N * N;                              // dQ, then du
    float da1[GD_CHUNKS], da2[GD_CHUNKS], db = 0.f;
#pragma unroll
    for (int k = 0; k < GD_CHUNKS; ++k) { da1[k] = 0.f; da2[k] = 0.f; }
    for (int64_t base = (int64_t)blockIdx.x * q.waves; base < q.G; base += (int64_t)gridDim.x * q.waves) {
        const int64_t gi = base + w;
        const bool valid = gi < q.G;
        if (valid) {
            gd_load_graph(q, gi, lane, zs, m);
            const float *hg = q.h + gi * N * C, *dg = q.dh + gi * N * C;
            for (int idx = lane; idx < N * C; idx += GD_WAVE) {
                const int i = idx / C, c = idx - i * C;
                const float hv = hg[idx];
                dhs[i * Cs + c] = dg[idx] * (hv > 0.f ? 1.f : hv + 1.f);               // ELU' = 1, or exp(H') = h + 1
            }
        }
        __syncthreads();
        if (valid) gd_scores(q, lane, zs, s, t);
        __syncthreads();
        if (valid)
            for (int i = 0; i < N; ++i) {
                float u;
                const float p = gd_softmax_row(q, lane, i, s, t, &u);
                if (lane < N) {
                    Pq[i * N + lane] = p;
                    DM[i * N + lane] = gd_keep(q, gi, i, lane) * (m[i] * m[lane]);
                    sl[i * N + lane] = u > 0.f ? 1.f : GD_SLOPE;
                }
            }
        if (valid)                                       // dQ_ij = dH'_i . Z_j (reads zs / dhs only: no barrier needed in front)
            for (int idx = lane; idx < N * N; idx += GD_WAVE) {
                const float *ra = dhs + (idx / N) * Cs, *rb = zs + (idx % N) * Cs;
                float d = 0.f;
                for (int c = 0; c < C; ++c) d = fmaf(ra[c], rb[c], d);
                dq[idx] = d;
            }
        __syncthreads();
        if (valid) {
            float dtj = 0.f;
            for (int i = 0; i < N; ++i) {
                const bool on = lane < N;
                const float p = on ? Pq[i * N + lane] : 0.f, dm = on ? DM[i * N + lane] : 0.f;
                const float dpm = on ? dq[i * N + lane] * dm : 0.f;
                const float rs = gd_wave_sum(dpm * p);
                const float du = on ? p * (dpm - rs) * sl[i * N + lane] : 0.f;
                const float dsi = gd_wave_sum(du);
                dtj += du;
                if (on) Pq[i * N + lane] = p * dm;
                if (lane == 0) ds[i] = dsi;
            }
            if (lane < N) dt[lane] = dtj;
        }
        __syncthreads();
        if (valid) {
#pragma unroll
            for (int k = 0; k < GD_CHUNKS; ++k) {
                const int c = lane + k * GD_WAVE;
                if (c < C) {
                    const float a1 = q.att[c], a2 = q.att[C + c];
                    float g1 = 0.f, g2 = 0.f;
                    for (int j = 0; j < N; ++j) {
                        float acc = fmaf(ds[j], a1, dt[j] * a2);
                        for (int i = 0; i < N; ++i) acc = fmaf(Pq[i * N + j], dhs[i * Cs + c], acc);
                        q.dz[(gi * N + j) * C + c] = acc;
                        const float zv = zs[j * Cs + c];
                        g1 = fmaf(ds[j], zv, g1);
                        g2 = fmaf(dt[j], zv, g2);
                    }
                    da1[k] += g1;
                    da2[k] += g2;
                }
            }
            if (lane == 0) {
                float v = 0.f;
                for (int i = 0; i < N; ++i) v += ds[i];
                db += v;
            }
        }
        __syncthreads();
    }
    float* row = q.part + ((size_t)blockIdx.x * q.waves + w) * (2 * C + 1);
#pragma unroll
    for (int k = 0; k < GD_CHUNKS; ++k) {
        const int c = lane + k * GD_WAVE;
        if (c < C) { row[c] = da1[k]; row[C + c] = da2[k]; }
    }
    if (lane == 0) row[2 * C] = db;
}

// launch geometry of an attention kernel: wavefronts per workgroup, LDS bytes, workgroups (fixed by the shape and the device)
struct GdLaunch {
    int waves, grid;
    size_t lds;
};
template <typename K>
int gd_att_launch(K kernel, const GdGeom& g, int C, bool bwd, GdLaunch* L) {
    L->waves = gd_att_waves(g.N, C, bwd);
    if (L->waves < 1) return RULGNN_EUNSUPPORTED;
    L->lds = (size_t)L->waves * gd_att_lds_floats(g.N, C, bwd) * sizeof(float);
    RULGNN_TRY(allow_dynamic_lds(kernel, L->lds));
    L->grid = resident_rows(kernel, GD_WAVE * L->waves, L->lds, (g.G + L->waves - 1) / L->waves, GD_ATT_MAXGRID);
    return RULGNN_OK;
}

}  // namespace

// RULGNN_OK, or the code every entry returns for a refused shape: unsupported for anything gd_geometry refuses, a negative batch included.
int Gdagdl::shape_status(const Shape* s) {
    GdGeom g;
    return gd_geometry(s, &g) == RULGNN_OK ? RULGNN_OK : RULGNN_EUNSUPPORTED;
}

int64_t Gdagdl::param_count(const Shape* s) {
    GdGeom g;
    return gd_geometry(s, &g) == RULGNN_OK ? g.pcount : -1;
}

int64_t Gdagdl::adam_first(const Shape* s) { return s->input_dim + 1; }

size_t Gdagdl::workspace_bytes(const Shape* s) {
    GdGeom g;
    return gd_geometry(s, &g) == RULGNN_OK ? (size_t)g.total * sizeof(float) : 0;
}

int64_t Gdagdl::tap_offset(const Shape* s, int which) {
    GdGeom g;
    if (gd_geometry(s, &g) != RULGNN_OK) return -1;
    switch (which) {
    case 0: return g.w_mag;
    case 1: return g.w_ni;
    case 2: return g.w_mask;
    case 3: return g.w_h[g.nl - 1];
    case 4: return g.ae.w_enc[3];
    default: return -1;
    }
}

// mode bit 0: forward, bit 1: backward (after a forward with the same args / workspace)
int Gdagdl::run(const Shape* s, const Args* a, int mode, hipStream_t st) {
    GdGeom g;
    RULGNN_TRY(gd_geometry(s, &g));
    if (a->workspace_bytes < (size_t)g.total * sizeof(float)) return RULGNN_EWORKSPACE;
    if (g.B == 0) return RULGNN_OK;
    float* ws = static_cast<float*>(a->workspace);
    const float* prm = a->params;
    const int64_t gb = a->global_batch > 0 ? a->global_batch : g.B;
    const float inv_gb = 1.0f / (float)gb;
    const int nl = g.nl, R = (int)g.R;
    const float rscale = 1.0f / ((float)gb * (float)g.T * (float)g.D);          // 1 / elements of the global batch's Y_o
    float* split = ws + g.w_split;
    float* one = ws + g.lh.w_one;                 // [0] = 1 (backward), [1] the reconstruction term, [2] the MSE, [3] = 0
    const float* yo = ws + g.w_h[nl - 1];         // Y_o as [BT, D] rows
    const float* henc = ws + g.ae.w_enc[3];       // the encoder's output: the LSTM's input
    const unsigned ggrid = (unsigned)(g.G < 4096 ? g.G : 4096);
    // The projection weights as GEMM operands: the flat buffer puts them behind f + 1 floats and odd-sized tensors, off a 16-byte
    // boundary (seq_backend.hpp: aligned_operand).
    const float* wop[GD_MAXL];
    for (int i = 0; i < nl; ++i) {
        wop[i] = aligned_operand(prm + g.o_w[i], (size_t)g.C[i] * g.C[i + 1], ws + g.w_wal[i], st);
        if (!wop[i]) return RULGNN_EHIP;
    }
    GdAtt q{};
    q.G = g.G; q.g0 = a->sample_offset * (int64_t)g.T; q.N = g.N; q.mask = ws + g.w_mask;
    const DropoutConst dc = dropout_const(a->training ? a->dropout_p : 0.f);
    q.thr = dc.thr; q.scale = dc.thr ? dc.scale : 0.f;
    if (mode & 1) {
        const size_t lds = sizeof(float) * gd_front_lds_floats(g.P, g.nseg, g.N, g.f);
        if (lds > DEFAULT_LDS_BYTES) return RULGNN_EUNSUPPORTED;
        RULGNN_TRY(fill_f32(one + 3, 1, 0.0f, st));
        RULGNN_TRY(launch_checked(gd_front_kernel, dim3(ggrid), dim3(SB), lds, st, g, a->x, prm, ws));
        const float* cur = ws + g.w_mag;
        for (int i = 0; i < nl; ++i) {
            const int Ci = g.C[i], Co = g.C[i + 1];
            RULGNN_TRY(sgemm(cur, Ci, 1, wop[i], Ci, 1, ws + g.w_z[i], Co, R, Co, Ci, false, st));
            GdLaunch L;
            RULGNN_TRY(gd_att_launch(gd_att_fwd_kernel, g, Co, false, &L));
            q.C = Co; q.waves = L.waves; q.z = ws + g.w_z[i]; q.bias = prm + g.o_b[i]; q.att = prm + g.o_aw[i]; q.h = ws + g.w_h[i];
            q.key = dropout_layer_key(a->seed, a->step, i);
            RULGNN_TRY(launch_checked(gd_att_fwd_kernel, dim3(L.grid), dim3(GD_WAVE * L.waves), L.lds, st, q));
            cur = ws + g.w_h[i];
        }
        RULGNN_TRY(autoencoder_forward(g.ae, yo, prm, ws, rscale, one + 1, split, st));
        RULGNN_TRY(lstm_head_forward(g.lh, henc, prm, ws, a->y, a->pred, inv_gb, st));
        if (a->recon) RULGNN_TRY(sum_pair(one + 1, one + 3, a->recon, st));
        if (a->y && a->loss) {
            RULGNN_TRY(block_sum((const float*)(ws + g.lh.w_sq), g.B, one + 2, st));
            RULGNN_TRY(sum_pair(one + 1, one + 2, a->loss, st));
        }
    }
    if (mode & 2) {
        if (!a->grads) return RULGNN_EINVAL;
        float* gr = a->grads;
        const float* dpred = a->dpred ? a->dpred : ws + g.lh.w_dpred;
        RULGNN_TRY(fill_f32(one, 1, 1.0f, st));
        RULGNN_TRY(fill_f32(gr + g.o_niw, g.f + 1, 0.0f, st));          // the mask has no gradient
        float* const dseq[2] = {ws + g.w_dhs, ws + g.ae.w_dH};
        RULGNN_TRY(lstm_head_backward(g.lh, henc, prm, ws, dpred, gr, dseq, split, st));
        RULGNN_TRY(autoencoder_backward(g.ae, yo, prm, ws, gr, one, a->recon_weight, split, st));
        const float* dcur = ws + g.ae.w_dD1;          // d Y_o = d h_last [R, C_last]
        for (int i = nl - 1; i >= 0; --i) {
            const int Ci = g.C[i], Co = g.C[i + 1];
            GdLaunch L;
            RULGNN_TRY(gd_att_launch(gd_att_bwd_kernel, g, Co, true, &L));
            q.C = Co; q.waves = L.waves; q.z = ws + g.w_z[i]; q.bias = prm + g.o_b[i]; q.att = prm + g.o_aw[i]; q.h = ws + g.w_h[i];
            q.dh = dcur; q.dz = ws + g.w_dz; q.part = ws + g.w_part;
            q.key = dropout_layer_key(a->seed, a->step, i);
            RULGNN_TRY(launch_checked(gd_att_bwd_kernel, dim3(L.grid), dim3(GD_WAVE * L.waves), L.lds, st, q));
            // attention.weight [2 Co] and attention.bias [1] are adjacent in the flat layout: one fixed-order sum of the partial rows
            RULGNN_TRY(rows_sum(ws + g.w_part, L.grid * L.waves, 2 * Co + 1, 2 * Co + 1, gr + g.o_aw[i], st));
            const float* hin = i > 0 ? ws + g.w_h[i - 1] : ws + g.w_mag;
            // (d h of layer i is consumed: one buffer serves every layer; the magnitude carries no gradient)
            RULGNN_TRY(dense_backward(ws + g.w_dz, hin, wop[i], one, gr + g.o_w[i], gr + g.o_b[i], i > 0 ? DENSE_PLAIN : DENSE_NO_DATA, ws + g.w_dh, R, Co,
                                      Ci, split, st));
            dcur = ws + g.w_dh;
        }
    }
    return RULGNN_OK;
}

}  // namespace rulgnn
