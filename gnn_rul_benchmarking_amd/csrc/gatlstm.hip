// GAT_LSTM on gfx950: patch statistics, graph attention under a banded adjacency, a stack of LSTMs over the nodes, a linear head.
// Reference path replaced: GAT_LSTM_model.forward -- models/GAT_LSTM/Model.py:112-165 (extract_features :8-72, GraphAttentionLayer
// :76-109) -- and GAT_LSTM.update, algorithms/algorithms.py:492-517 (loss = MSE(pred, y)).
//
//   x [bs, T * P] -> 11 statistics per patch -> one graph per sample, T nodes, adj_ij = [|i - j| <= 1] -> L GAT layers: Z = h W^T + b,
//   u_ij = a1 . Z_i + a2 . Z_j + c, p = softmax_j(leakyrelu(u, 0.1)) over ALL j, q = p o D o adj (D: dropout keep mask / (1 - p_drop),
//   train mode), h = leakyrelu(q Z, 0.01) -> K stacked unidirectional LSTMs over the T nodes -> Linear(E_K T -> 1).
//
// The band collapses the N x N stage.  leakyrelu is increasing, so the row maximum of the logits is m_i = leakyrelu(s_i + max_j t_j + c)
// with s = Z a1, t = Z a2, and the denominator D_i = sum_j exp(leakyrelu(s_i + t_j + c) - m_i) needs the two vectors alone: O(N^2)
// scalar work, nothing N x N stored.  The exponent is formed in fp64 from the fp32 vectors (gl_expo): at the full widths s and t reach
// thousands, and rounding s_i + t_j to fp32 (1e-4 absolute there) would enter every probability as relative error.  Three probabilities per row survive the band: y_i = sum_{j = i-1 .. i+1} p_ij d_ij Z_j.
//
// Launches: one front-end kernel per call (gl_feat_kernel: a wavefront per patch, the patch held in registers between the two passes);
// per layer one matrix-core GEMM for h W^T (the bias is added where Z is read) and ONE attention kernel (gl_att_fwd_kernel: a workgroup
// per graph, a wavefront per node strip; s, t, m, D in LDS); backward per layer one kernel (gl_att_bwd_kernel: recomputes s, t, m, D
// from the saved Z, takes the sign of y from the saved h, writes dZ and one partial row [da1 | da2 | dc] per wavefront, summed in a
// fixed order by rows_sum) and the GEMMs dW = dZ^T h, db = sum dZ, dh = dZ W.  The LSTMs are bilstm.hip's persistent kernels (one
// direction), the head and the loss seq_backend.hip's.  Between launches only feat, Z_l, h_l, dZ, dh, the LSTM tensors and the partial
// rows exist.  No floating-point atomics; the partial-row count is fixed by the launch geometry, so two runs give the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sgemm_mfma.hpp"
#include "families_host.hpp"       // (stgcn_host.hpp: dropout_layer_key)
#include "stgcn_device.hpp"        // lowbias32
#include "seq_backend.hpp"         // the LSTM stack and the head (shared with stnet.hip and gdagdl.hip)

namespace rulgnn {

namespace {

constexpr int GL_MAXL = RULGNN_GATLSTM_MAX_LAYERS, GL_MAXC = RULGNN_GATLSTM_MAX_WIDTH, GL_MAXK = RULGNN_GATLSTM_MAX_LSTM_LAYERS;
constexpr int GL_F = 11;                         // statistics per patch
constexpr int GL_WAVE = 64, GL_WAVES = 4, GL_BLOCK = GL_WAVE * GL_WAVES, GL_CHUNKS = GL_MAXC / GL_WAVE;
constexpr int GL_PREG = RULGNN_GATLSTM_MAX_PATCH_SIZE / GL_WAVE;      // patch values a lane holds
constexpr int GL_ATT_MAXGRID = 1024;
constexpr float GL_SLOPE = 0.1f;                 // Model.py:77 alpha (the logits)
constexpr double GL_SLOPE_D = 0.1;               // ... where the logits are formed in fp64 (gl_expo)
constexpr float GL_OUT_SLOPE = 0.01f;            // Model.py:100 F.leaky_relu's default (the layer output)
static_assert(RULGNN_GATLSTM_MAX_NUM_PATCH <= GL_BLOCK / 2, "the backward sums ds and dt with a thread per node each");

struct GlGeom {
    int64_t B, R;                                // samples = graphs, node rows = B * T
    int T, P, nl;
    int C[GL_MAXL + 1];                          // channel widths: 11, hidden_dim...
    int o_w[GL_MAXL], o_b[GL_MAXL], o_aw[GL_MAXL], o_ab[GL_MAXL], pcount;      // flat parameter offsets of the GAT layers; the back end's are the plan's
    LstmHeadPlan lh;                             // LSTM widths C[nl], lstm_hidden_dim... over the T nodes, Linear(E_K * T, 1)
    // workspace offsets (floats)
    int64_t w_wal[GL_MAXL];                      // 16-byte aligned copies of the projection weights (see Gatlstm::run)
    int64_t w_feat, w_z[GL_MAXL], w_h[GL_MAXL], w_dz, w_d1, w_d2, w_part, w_split, total;
};
static_assert(GL_MAXK <= SEQ_MAX_LSTM, "the plan holds every LSTM layer");

// ---- LDS layout of the attention kernels, stated once for kernel and launcher (floats) ------------------------------------------------
// forward: s, t, m (max_j t_j, the same in every entry), D [N] each; backward: the same, then g [N][3] (d_ij dy_i . Z_j on the band), q [N][3] (p_ij d_ij), r, ds, dt [N] each.
__host__ __device__ inline size_t gl_att_lds_floats(int N, bool bwd) { return (size_t)N * (bwd ? 13 : 4); }

int gl_geometry(const rulgnn_gatlstm_shape* s, GlGeom* g) {
    if (!s) return RULGNN_EINVAL;
    if (s->batch < 0 || s->num_patch < 1 || s->patch_size < 1 || s->num_gat < 1 || s->num_lstm < 1) return RULGNN_EINVAL;
    if (s->num_patch > RULGNN_GATLSTM_MAX_NUM_PATCH || s->patch_size < RULGNN_GATLSTM_MIN_PATCH_SIZE ||
        s->patch_size > RULGNN_GATLSTM_MAX_PATCH_SIZE || s->num_gat > GL_MAXL || s->num_lstm > GL_MAXK)
        return RULGNN_EUNSUPPORTED;
    g->B = s->batch; g->T = s->num_patch; g->P = s->patch_size; g->nl = s->num_gat;
    LstmHeadPlan& lh = g->lh;
    lh.B = g->B; lh.T = g->T; lh.nk = s->num_lstm;
    g->C[0] = GL_F;
    int wmax = GL_F;
    for (int i = 0; i < g->nl; ++i) {
        if (s->hidden_dim[i] < 1) return RULGNN_EINVAL;
        if (s->hidden_dim[i] > GL_MAXC) return RULGNN_EUNSUPPORTED;
        g->C[i + 1] = s->hidden_dim[i];
        if (g->C[i + 1] > wmax) wmax = g->C[i + 1];
    }
    lh.H[0] = g->C[g->nl];
    for (int k = 0; k < lh.nk; ++k) {
        if (s->lstm_hidden_dim[k] < 1) return RULGNN_EINVAL;
        if (s->lstm_hidden_dim[k] > RULGNN_GATLSTM_MAX_LSTM_HIDDEN) return RULGNN_EUNSUPPORTED;
        lh.H[k + 1] = s->lstm_hidden_dim[k];
        if (lh.H[k + 1] > wmax) wmax = lh.H[k + 1];
    }
    g->R = g->B * g->T;
    if (g->R * (int64_t)wmax > 0x7fffffff) return RULGNN_EUNSUPPORTED;      // the GEMMs take int extents
    int o = 0;
    int64_t w = 0;
    SplitKScratch sp(1024);
    auto tk = [&](int n) { const int r = o; o += n; return r; };
    auto wk = [&](int64_t n) { const int64_t r = w; w += (n + 63) & ~(int64_t)63; return r; };
    for (int i = 0; i < g->nl; ++i) {
        g->o_w[i] = tk(g->C[i + 1] * g->C[i]); g->o_b[i] = tk(g->C[i + 1]);
        g->o_aw[i] = tk(2 * g->C[i + 1]); g->o_ab[i] = tk(1);
    }
    const int64_t R = g->R;
    g->w_feat = wk(R * GL_F);
    for (int i = 0; i < g->nl; ++i) { g->w_z[i] = wk(R * g->C[i + 1]); g->w_h[i] = wk(R * g->C[i + 1]); }
    RULGNN_TRY(lstm_head_layout(&lh, &o, &w, &sp));
    g->pcount = o;
    g->w_dz = wk(R * wmax); g->w_d1 = wk(R * wmax); g->w_d2 = wk(R * wmax);
    g->w_part = wk((int64_t)GL_ATT_MAXGRID * GL_WAVES * (2 * wmax + 1));
    for (int i = 0; i < g->nl; ++i) g->w_wal[i] = wk((int64_t)g->C[i] * g->C[i + 1]);
    for (int i = 0; i < g->nl; ++i) { sp.need(g->C[i + 1], g->C[i], R); sp.need(1, g->C[i + 1], R); }
    g->w_split = wk((int64_t)sp.floats());
    g->total = w;
    return RULGNN_OK;
}

__device__ __forceinline__ float gl_wave_sum(float v) {
#pragma unroll
    for (int m = GL_WAVE / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, GL_WAVE);
    return v;
}
__device__ __forceinline__ float gl_wave_max(float v) {
#pragma unroll
    for (int m = GL_WAVE / 2; m > 0; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, GL_WAVE));
    return v;
}

// ---- front end: the 11 statistics of a patch (Model.py:8-72), one wavefront per patch ------------------------------------------------
// The patch is read from HBM once: lane l holds x[l], x[l + 64], ... (at most GL_PREG values) in registers for the second pass, which
// takes the central moments about the mean of the first.  std is the unbiased one from the centred sum; no raw-moment formula anywhere
// (the kurtosis column reaches 1e4 while the others are O(1)).  No epsilon: 0 / 0 = NaN on a constant patch, as the reference.
__global__ __launch_bounds__(GL_BLOCK) void gl_feat_kernel(int64_t G, int P, float cskew, float ckurt, const float* __restrict__ x,
                                                           float* __restrict__ feat) {
    const int lane = threadIdx.x % GL_WAVE;
    const float inv = 1.0f / (float)P;
    for (int64_t gi = (int64_t)blockIdx.x * GL_WAVES + threadIdx.x / GL_WAVE; gi < G; gi += (int64_t)gridDim.x * GL_WAVES) {
        const float* px = x + gi * P;
        float v[GL_PREG];
        float sum = 0.f, sabs = 0.f, ssqrt = 0.f, ssq = 0.f, mx = -INFINITY, mn = INFINITY, mxabs = 0.f;
#pragma unroll
        for (int k = 0; k < GL_PREG; ++k) {
            const int idx = k * GL_WAVE + lane;
            v[k] = 0.f;
            if (idx < P) {
                const float a = px[idx], b = fabsf(a);
                v[k] = a;
                sum += a; sabs += b; ssqrt += sqrtf(b); ssq = fmaf(a, a, ssq);
                mx = fmaxf(mx, a); mn = fminf(mn, a); mxabs = fmaxf(mxabs, b);
            }
        }
        sum = gl_wave_sum(sum); sabs = gl_wave_sum(sabs); ssqrt = gl_wave_sum(ssqrt); ssq = gl_wave_sum(ssq);
        mx = gl_wave_max(mx); mn = -gl_wave_max(-mn); mxabs = gl_wave_max(mxabs);
        const float mean = sum * inv;
        float d2 = 0.f, d3 = 0.f, d4 = 0.f;
#pragma unroll
        for (int k = 0; k < GL_PREG; ++k)
            if (k * GL_WAVE + lane < P) {
                const float d = v[k] - mean, dd = d * d;
                d2 += dd; d3 = fmaf(dd, d, d3); d4 = fmaf(dd, dd, d4);
            }
        d2 = gl_wave_sum(d2); d3 = gl_wave_sum(d3); d4 = gl_wave_sum(d4);
        if (lane == 0) {
            const float sd = sqrtf(d2 / (float)(P - 1));
            const float ra = ssqrt * inv, rmsa = ra * ra, rms = sqrtf(ssq * inv), mabs = sabs * inv;
            float* o = feat + gi * GL_F;
            o[0] = mean;
            o[1] = sd;
            o[2] = rmsa;
            o[3] = rms;
            o[4] = 0.5f * (mx - mn);
            o[5] = cskew * d3 / (sd * sd * sd);
            o[6] = ckurt * d4 / ((sd * sd) * (sd * sd));
            o[7] = mxabs / rms;
            o[8] = mxabs / rmsa;
            o[9] = rms / mabs;
            o[10] = mxabs / mabs;
        }
    }
}

// ---- banded graph attention ----------------------------------------------------------------------------------------------------------
struct GlAtt {
    int64_t G, g0;                    // graphs (= samples) of this call; global index of its first (dropout counters)
    int N, C;
    const float *z, *bias, *att;      // Z [G N][C] without its bias, linear.bias [C], attention.{weight [2C], bias [1]} (adjacent)
    float* h;                         // forward: leakyrelu(q Z) [G N][C] (written); backward: the same (read)
    const float* dh;                  // backward: d h
    float* dz;                        // backward: d Z
    float* part;                      // backward: [gridDim.x * GL_WAVES][2 C + 1] partial rows [da1 | da2 | dc]
    uint32_t key, thr;                // dropout: keep where lowbias32(counter ^ key) >= thr
    float scale;                      // 1 / (1 - p); 0: no dropout
};

// keep mask / (1 - p) of band entry (i, i - 1 + b) of graph gi
__device__ __forceinline__ float gl_keep(const GlAtt& q, int64_t gi, int i, int b) {
    if (q.scale == 0.f) return 1.f;
    const uint32_t ctr = (uint32_t)((((uint64_t)(q.g0 + gi) * q.N + i) * 3) + b);
    return lowbias32(ctr ^ q.key) >= q.thr ? q.scale : 0.f;
}
// s_i = a1 . Z_i, t_i = a2 . Z_i: a wavefront per node, nodes strided over the workgroup's wavefronts
__device__ __forceinline__ void gl_scores(const GlAtt& q, const float* __restrict__ zg, int lane, int w, float* s, float* t) {
    const int N = q.N, C = q.C;
    for (int i = w; i < N; i += GL_WAVES) {
        const float* zr = zg + (int64_t)i * C;
        float ps = 0.f, pt = 0.f;
        for (int c = lane; c < C; c += GL_WAVE) {
            const float zv = zr[c] + q.bias[c];
            ps = fmaf(q.att[c], zv, ps);
            pt = fmaf(q.att[C + c], zv, pt);
        }
        ps = gl_wave_sum(ps);
        pt = gl_wave_sum(pt);
        if (lane == 0) { s[i] = ps; t[i] = pt; }
    }
}
// exp(leakyrelu(u_ij) - leakyrelu(u_i,max)) with u_ij = (s_i + c) + t_j and u_i,max = (s_i + c) + max_j t_j: the two sums and their
// difference in fp64 (exact on fp32 operands), the exponential in fp32.  *u (if given) receives u_ij for the leaky ReLU's derivative.
__device__ __forceinline__ float gl_expo(float si_c, float tj, float tmax, float* u = nullptr) {
    const double uv = (double)si_c + (double)tj, um = (double)si_c + (double)tmax;
    if (u) *u = (float)uv;
    return expf((float)((uv > 0.0 ? uv : GL_SLOPE_D * uv) - (um > 0.0 ? um : GL_SLOPE_D * um)));
}
// m = max_j t_j (every entry), D_i = sum_j exp(leakyrelu(u_ij) - leakyrelu(u_i,max)): a thread per row.  A NaN in s or t makes every D of
// the graph NaN (fmaxf skips a NaN t_j, the sum does not).
__device__ __forceinline__ void gl_row_stats(const GlAtt& q, int tid, const float* s, const float* t, float* m, float* D) {
    const int N = q.N;
    if (tid < N) {
        float tmax = t[0];
        for (int j = 1; j < N; ++j) tmax = fmaxf(tmax, t[j]);
        const float si = s[tid] + q.att[2 * q.C];
        float d = 0.f;
        for (int j = 0; j < N; ++j) d += gl_expo(si, t[j], tmax);
        m[tid] = tmax;
        D[tid] = d;
    }
}
// p_ij = softmax_j(leakyrelu(u_i.))_j from the vectors
__device__ __forceinline__ float gl_prob(float si_c, float tj, float tmax, float Di) { return gl_expo(si_c, tj, tmax) / Di; }

// A workgroup per graph (grid-stride), a wavefront per node strip.
__global__ __launch_bounds__(GL_BLOCK) void gl_att_fwd_kernel(GlAtt q) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int N = q.N, C = q.C, tid = threadIdx.x, lane = tid % GL_WAVE, w = tid / GL_WAVE;
    float* s = sm;
    float* t = s + N;
    float* m = t + N;
    float* D = m + N;
    const float cb = q.att[2 * C];
    for (int64_t gi = blockIdx.x; gi < q.G; gi += gridDim.x) {
        const float* zg = q.z + gi * N * C;
        gl_scores(q, zg, lane, w, s, t);
        __syncthreads();
        gl_row_stats(q, tid, s, t, m, D);
        __syncthreads();
        for (int i = w; i < N; i += GL_WAVES) {
            const float si = s[i] + cb, tm = m[i], Di = D[i];
            const bool lo = i > 0, hi = i + 1 < N;
            const float q0 = lo ? gl_prob(si, t[i - 1], tm, Di) * gl_keep(q, gi, i, 0) : 0.f;
            const float q1 = gl_prob(si, t[i], tm, Di) * gl_keep(q, gi, i, 1);
            const float q2 = hi ? gl_prob(si, t[i + 1], tm, Di) * gl_keep(q, gi, i, 2) : 0.f;
            const float* zr = zg + (int64_t)i * C;
            float* hr = q.h + (gi * N + i) * C;
            for (int c = lane; c < C; c += GL_WAVE) {
                const float b = q.bias[c];
                float acc = q1 * (zr[c] + b);
                if (lo) acc = fmaf(q0, zr[c - C] + b, acc);
                if (hi) acc = fmaf(q2, zr[c + C] + b, acc);
                hr[c] = acc > 0.f ? acc : GL_OUT_SLOPE * acc;
            }
        }
        __syncthreads();                                 // s .. D are rewritten by the next graph
    }
}

__global__ __launch_bounds__(GL_BLOCK) void gl_att_bwd_kernel(GlAtt q) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int N = q.N, C = q.C, tid = threadIdx.x, lane = tid % GL_WAVE, w = tid / GL_WAVE;
    float* s = sm;
    float* t = s + N;
    float* m = t + N;
    float* D = m + N;
    float* gb = D + N;                                   // [N][3] g_ij = d_ij (dy_i . Z_j)
    float* qb = gb + 3 * N;                              // [N][3] q_ij = p_ij d_ij
    float* r = qb + 3 * N;                               // r_i = sum_band p_ij g_ij
    float* ds = r + N;
    float* dt = ds + N;
    const float cb = q.att[2 * C];
    float da1[GL_CHUNKS], da2[GL_CHUNKS], dc = 0.f;
#pragma unroll
    for (int k = 0; k < GL_CHUNKS; ++k) { da1[k] = 0.f; da2[k] = 0.f; }
    for (int64_t gi = blockIdx.x; gi < q.G; gi += gridDim.x) {
        const float* zg = q.z + gi * N * C;
        const float* hg = q.h + gi * N * C;
        const float* dg = q.dh + gi * N * C;
        gl_scores(q, zg, lane, w, s, t);
        __syncthreads();
        gl_row_stats(q, tid, s, t, m, D);
        __syncthreads();
        // the band: dy_i = dh_i o leakyrelu'(y_i) (the sign of y is the saved h's), g_ij = d_ij (dy_i . Z_j), q_ij, r_i
        for (int i = w; i < N; i += GL_WAVES) {
            const bool lo = i > 0, hi = i + 1 < N;
            const float* zr = zg + (int64_t)i * C;
            float p0 = 0.f, p1 = 0.f, p2 = 0.f;
            for (int c = lane; c < C; c += GL_WAVE) {
                const float b = q.bias[c];
                const float dy = dg[(int64_t)i * C + c] * (hg[(int64_t)i * C + c] > 0.f ? 1.f : GL_OUT_SLOPE);
                p1 = fmaf(dy, zr[c] + b, p1);
                if (lo) p0 = fmaf(dy, zr[c - C] + b, p0);
                if (hi) p2 = fmaf(dy, zr[c + C] + b, p2);
            }
            p0 = gl_wave_sum(p0); p1 = gl_wave_sum(p1); p2 = gl_wave_sum(p2);
            if (lane == 0) {
                const float si = s[i] + cb, tm = m[i], Di = D[i];
                const float dot[3] = {p0, p1, p2};
                float ri = 0.f;
                for (int b = 0; b < 3; ++b) {
                    const int j = i - 1 + b;
                    float gv = 0.f, qv = 0.f;
                    if (j >= 0 && j < N) {
                        const float p = gl_prob(si, t[j], tm, Di), k = gl_keep(q, gi, i, b);
                        gv = k * dot[b];
                        qv = p * k;
                        ri = fmaf(p, gv, ri);
                    }
                    gb[3 * i + b] = gv;
                    qb[3 * i + b] = qv;
                }
                r[i] = ri;
            }
        }
        __syncthreads();
        // du_ij = p_ij (adj_ij g_ij - r_i) leakyrelu'(u_ij) for ALL j: ds_i = sum_j du_ij (threads 0 .. N-1), dt_j = sum_i du_ij (threads
        // GL_BLOCK / 2 .. GL_BLOCK / 2 + N-1); both halves evaluate du with the same expression
        {
            const bool rowsum = tid < GL_BLOCK / 2;
            const int a = rowsum ? tid : tid - GL_BLOCK / 2;
            if (a < N) {
                float acc = 0.f;
                for (int o = 0; o < N; ++o) {
                    const int i = rowsum ? a : o, j = rowsum ? o : a;
                    float u;
                    const float p = gl_expo(s[i] + cb, t[j], m[i], &u) / D[i];
                    const int b = j - i + 1;
                    const float gv = (b >= 0 && b < 3) ? gb[3 * i + b] : 0.f;
                    acc += p * (gv - r[i]) * (u > 0.f ? 1.f : GL_SLOPE);
                }
                (rowsum ? ds : dt)[a] = acc;
            }
        }
        __syncthreads();
        if (tid == 0) {
            float v = 0.f;
            for (int i = 0; i < N; ++i) v += ds[i];
            dc += v;
        }
        // dZ_j = sum_{band i} q_ij dy_i + ds_j a1 + dt_j a2;  da1 += ds_j Z_j, da2 += dt_j Z_j
        for (int j = w; j < N; j += GL_WAVES) {
            const bool lo = j > 0, hi = j + 1 < N;
            const float dsj = ds[j], dtj = dt[j];
            const float q0 = lo ? qb[3 * (j - 1) + 2] : 0.f, q1 = qb[3 * j + 1], q2 = hi ? qb[3 * (j + 1)] : 0.f;
            const int64_t ro = (int64_t)j * C;
#pragma unroll
            for (int k = 0; k < GL_CHUNKS; ++k) {
                const int c = lane + k * GL_WAVE;
                if (c < C) {
                    const float zv = zg[ro + c] + q.bias[c];
                    float acc = fmaf(dsj, q.att[c], dtj * q.att[C + c]);
                    acc = fmaf(q1, dg[ro + c] * (hg[ro + c] > 0.f ? 1.f : GL_OUT_SLOPE), acc);
                    if (lo) acc = fmaf(q0, dg[ro - C + c] * (hg[ro - C + c] > 0.f ? 1.f : GL_OUT_SLOPE), acc);
                    if (hi) acc = fmaf(q2, dg[ro + C + c] * (hg[ro + C + c] > 0.f ? 1.f : GL_OUT_SLOPE), acc);
                    q.dz[gi * N * C + ro + c] = acc;
                    da1[k] = fmaf(dsj, zv, da1[k]);
                    da2[k] = fmaf(dtj, zv, da2[k]);
                }
            }
        }
        __syncthreads();
    }
    float* row = q.part + ((size_t)blockIdx.x * GL_WAVES + w) * (2 * C + 1);
#pragma unroll
    for (int k = 0; k < GL_CHUNKS; ++k) {
        const int c = lane + k * GL_WAVE;
        if (c < C) { row[c] = da1[k]; row[C + c] = da2[k]; }
    }
    if (lane == 0) row[2 * C] = dc;                      // (wavefront 0 carries the workgroup's dc, the others 0)
}

// launch geometry of an attention kernel: LDS bytes, workgroups (fixed by the shape and the device)
struct GlLaunch {
    int grid;
    size_t lds;
};
template <typename K>
int gl_att_launch(K kernel, const GlGeom& g, bool bwd, GlLaunch* L) {
    L->lds = gl_att_lds_floats(g.T, bwd) * sizeof(float);
    RULGNN_TRY(allow_dynamic_lds(kernel, L->lds));
    L->grid = resident_rows(kernel, GL_BLOCK, L->lds, g.B, GL_ATT_MAXGRID);
    return RULGNN_OK;
}

}  // namespace

// RULGNN_OK, or the code every entry returns for a refused shape: unsupported for anything gl_geometry refuses, a negative batch included.
int Gatlstm::shape_status(const Shape* s) {
    GlGeom g;
    return gl_geometry(s, &g) == RULGNN_OK ? RULGNN_OK : RULGNN_EUNSUPPORTED;
}

int64_t Gatlstm::param_count(const Shape* s) {
    GlGeom g;
    return gl_geometry(s, &g) == RULGNN_OK ? g.pcount : -1;
}

size_t Gatlstm::workspace_bytes(const Shape* s) {
    GlGeom g;
    return gl_geometry(s, &g) == RULGNN_OK ? (size_t)g.total * sizeof(float) : 0;
}

int64_t Gatlstm::tap_offset(const Shape* s, int which) {
    GlGeom g;
    if (gl_geometry(s, &g) != RULGNN_OK) return -1;
    if (which == 0) return g.w_feat;
    if (which >= 1 && which <= g.nl) return g.w_h[which - 1];
    if (which == RULGNN_GATLSTM_TAP_LSTM) return g.lh.w_hseq[g.lh.nk - 1];
    return -1;
}

// mode bit 0: forward, bit 1: backward (after a forward with the same args / workspace)
int Gatlstm::run(const Shape* s, const Args* a, int mode, hipStream_t st) {
    GlGeom g;
    RULGNN_TRY(gl_geometry(s, &g));
    if (a->workspace_bytes < (size_t)g.total * sizeof(float)) return RULGNN_EWORKSPACE;
    if (g.B == 0) return RULGNN_OK;
    float* ws = static_cast<float*>(a->workspace);
    const float* prm = a->params;
    const int64_t gb = a->global_batch > 0 ? a->global_batch : g.B;
    const float inv_gb = 1.0f / (float)gb;
    const int nl = g.nl, R = (int)g.R;
    float* split = ws + g.w_split;
    const float* hgat = ws + g.w_h[nl - 1];       // the last GAT layer's output: the LSTM stack's input
    // The projection weights as GEMM operands: the flat buffer puts them behind odd-sized tensors, off a 16-byte boundary
    // (seq_backend.hpp: aligned_operand).
    const float* wop[GL_MAXL];
    for (int i = 0; i < nl; ++i) {
        wop[i] = aligned_operand(prm + g.o_w[i], (size_t)g.C[i] * g.C[i + 1], ws + g.w_wal[i], st);
        if (!wop[i]) return RULGNN_EHIP;
    }
    GlAtt q{};
    q.G = g.B; q.g0 = a->sample_offset; q.N = g.T;
    const DropoutConst dc = dropout_const(a->training ? a->dropout_p : 0.f);
    q.thr = dc.thr; q.scale = dc.thr ? dc.scale : 0.f;
    if (mode & 1) {
        const double m = (double)g.P;
        const float cskew = (float)(m / ((m - 1) * (m - 2)));
        const float ckurt = (float)((m * (m + 1) - 3 * (m - 1) * (m - 1) * (m - 1)) / ((m - 1) * (m - 2) * (m - 3)));
        const int64_t fb = (g.R + GL_WAVES - 1) / GL_WAVES;
        RULGNN_TRY(launch_checked(gl_feat_kernel, dim3((unsigned)(fb < 4096 ? fb : 4096)), dim3(GL_BLOCK), 0, st, g.R, g.P, cskew, ckurt, a->x,
                                  ws + g.w_feat));
        GlLaunch L;                                  // the same for every layer: the LDS request depends on T alone
        RULGNN_TRY(gl_att_launch(gl_att_fwd_kernel, g, false, &L));
        const float* cur = ws + g.w_feat;
        for (int i = 0; i < nl; ++i) {
            const int Ci = g.C[i], Co = g.C[i + 1];
            RULGNN_TRY(sgemm(cur, Ci, 1, wop[i], Ci, 1, ws + g.w_z[i], Co, R, Co, Ci, false, st));
            q.C = Co; q.z = ws + g.w_z[i]; q.bias = prm + g.o_b[i]; q.att = prm + g.o_aw[i]; q.h = ws + g.w_h[i];
            q.key = dropout_layer_key(a->seed, a->step, i);
            RULGNN_TRY(launch_checked(gl_att_fwd_kernel, dim3(L.grid), dim3(GL_BLOCK), L.lds, st, q));
            cur = ws + g.w_h[i];
        }
        RULGNN_TRY(lstm_head_forward(g.lh, hgat, prm, ws, a->y, a->pred, inv_gb, st));
        if (a->y && a->loss) RULGNN_TRY(block_sum((const float*)(ws + g.lh.w_sq), g.B, a->loss, st));
    }
    if (mode & 2) {
        if (!a->grads) return RULGNN_EINVAL;
        float* gr = a->grads;
        const float* dpred = a->dpred ? a->dpred : ws + g.lh.w_dpred;
        float* one = ws + g.lh.w_one;
        RULGNN_TRY(fill_f32(one, 1, 1.0f, st));
        float* const dbuf[2] = {ws + g.w_d1, ws + g.w_d2};      // the data gradient walks down through two buffers
        RULGNN_TRY(lstm_head_backward(g.lh, hgat, prm, ws, dpred, gr, dbuf, split, st));
        int cur = g.lh.nk & 1;                       // d h of the last GAT layer
        GlLaunch L;
        RULGNN_TRY(gl_att_launch(gl_att_bwd_kernel, g, true, &L));
        for (int i = nl - 1; i >= 0; --i) {
            const int Ci = g.C[i], Co = g.C[i + 1];
            q.C = Co; q.z = ws + g.w_z[i]; q.bias = prm + g.o_b[i]; q.att = prm + g.o_aw[i]; q.h = ws + g.w_h[i];
            q.dh = dbuf[cur]; q.dz = ws + g.w_dz; q.part = ws + g.w_part;
            q.key = dropout_layer_key(a->seed, a->step, i);
            RULGNN_TRY(launch_checked(gl_att_bwd_kernel, dim3(L.grid), dim3(GL_BLOCK), L.lds, st, q));
            // attention.weight [2 Co] and attention.bias [1] are adjacent in the flat layout: one fixed-order sum of the partial rows
            RULGNN_TRY(rows_sum(ws + g.w_part, L.grid * GL_WAVES, 2 * Co + 1, 2 * Co + 1, gr + g.o_aw[i], st));
            const float* hin = i > 0 ? ws + g.w_h[i - 1] : ws + g.w_feat;
            // (the features have no parameters upstream)
            RULGNN_TRY(dense_backward(ws + g.w_dz, hin, wop[i], one, gr + g.o_w[i], gr + g.o_b[i], i > 0 ? DENSE_PLAIN : DENSE_NO_DATA, dbuf[cur ^ 1], R,
                                      Co, Ci, split, st));
            cur ^= 1;
        }
    }
    return RULGNN_OK;
}

}  // namespace rulgnn
