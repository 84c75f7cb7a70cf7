// STFA on gfx950: multi-head graph attention on the fixed prior-knowledge graph of the 14 C-MAPSS sensors, one LSTM, a last-step head.
// Reference path replaced: STFA_model.forward -- models/STFA/Model.py:93-126 (GraphAttentionLayer :11-45, GAT :47-58, prior_knowledge_graph
// :61-77) -- and STFA.update, algorithms/algorithms.py:183-192 (loss = MSE(pred, y)).
//
//   x [bs, 14, T * P] -> G = bs * T graphs of 14 nodes with P features -> per head h: Z = x W^T + b [14, C], u_ij = a1 . Z_i + a2 . Z_j + c,
//   p = softmax_j(leakyrelu(u, 0.1)) over ALL 14 nodes, q = p o D o A (D: dropout keep mask / (1 - p_drop), train mode; A: the 22 undirected
//   edges, no self-loops, applied BEHIND the softmax: rows do not sum to one), h' = q Z -> relu(mean over heads) [G, 14, C] -> the LSTM's
//   input row [1 x T | 14 C features] -> one LSTM -> Linear(E, 1) on the last step.
//
// Reference quirks kept: the "ASE" softmax acts on a singleton and is exactly 1 (Model.py:115), so the T "global feature" columns are
// ones and v.{weight, bias} get gradients that are exactly zero (zeros, not None: Adam's weight decay still moves v); hidden_dim is unused.
//
// Launches of the graph stage: ONE forward kernel and ONE backward kernel (no GEMM: with P = 2 and C = 5 a projection GEMM would be all
// overhead).  A wavefront per graph, SF_WAVES graphs in flight per workgroup; the x tile, Z of all heads and the two score vectors per head
// live in LDS; lanes walk (head, row) pairs, each taking its row's softmax over the 14 columns in registers and h' over the row's at most
// 6 neighbours.  The adjacency is the neighbour table below, not a tensor.  The forward writes relu(mean h') straight into the LSTM's
// input row behind the T ones it also writes; nothing N x N exists outside LDS and registers.  The backward recomputes Z, the scores and
// p from the x tile (the only saved activation is the stage output, for the ReLU gate), redraws the masks and accumulates one partial
// row of all Hd (C P + C + 2 C + 1) parameter gradients per wavefront -- in the flat parameter order, so one fixed-order rows_sum lands
// them in the gradient buffer.  No floating-point atomics; the partial-row count follows from the launch geometry: same bits every run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sgemm_mfma.hpp"
#include "families_host.hpp"       // (stgcn_host.hpp: dropout_layer_key)
#include "stgcn_device.hpp"        // lowbias32
#include "seq_backend.hpp"         // the LSTM and the last-step head

namespace rulgnn {

namespace {

constexpr int SF_N = RULGNN_STFA_NUM_NODES, SF_MAXC = RULGNN_STFA_MAX_OUTPUT_DIM;
constexpr int SF_WAVE = 64, SF_WAVES = 2, SF_BLOCK = SF_WAVE * SF_WAVES;
constexpr int SF_FWD_MAXGRID = 2048;             // workgroups of the forward at most (it writes no partial rows: the cap only bounds the launch)
constexpr int SF_BWD_MAXGRID = 1024;             // ... and of the backward: SF_WAVES partial rows each
constexpr int64_t SF_PART_FLOATS = (int64_t)1 << 23;      // the partial rows take 32 MiB at most: wide rows lower the backward's cap
constexpr int SF_EDGES = 44;                     // directed edges of the graph: the draws of one (graph, head)
constexpr float SF_SLOPE = 0.1f;                 // Model.py:12 alpha
static_assert(SF_N == 14, "the prior-knowledge graph is a 14 x 14 constant");

// prior_knowledge_graph (Model.py:65-68), 0-based: bit j of SF_MASK[i] <=> nodes i and j are connected.  SF_START[i]: directed edges of
// the rows before i (row-major, columns ascending): the edge's index in the dropout counter.
__constant__ uint16_t SF_MASK[SF_N] = {
    (1 << 1) | (1 << 2) | (1 << 3) | (1 << 4) | (1 << 8) | (1 << 11),      // 0: 1 2 3 4 8 11
    (1 << 0) | (1 << 3) | (1 << 6) | (1 << 7) | (1 << 12),                 // 1: 0 3 6 7 12
    (1 << 0) | (1 << 5) | (1 << 9) | (1 << 12) | (1 << 13),                // 2: 0 5 9 12 13
    (1 << 0) | (1 << 1) | (1 << 6) | (1 << 7),                             // 3: 0 1 6 7
    (1 << 0) | (1 << 8) | (1 << 10),                                       // 4: 0 8 10
    (1 << 2) | (1 << 9),                                                   // 5: 2 9
    (1 << 1) | (1 << 3) | (1 << 7),                                        // 6: 1 3 7
    (1 << 1) | (1 << 3) | (1 << 6) | (1 << 12),                            // 7: 1 3 6 12
    (1 << 0) | (1 << 4) | (1 << 10),                                       // 8: 0 4 10
    (1 << 2) | (1 << 5),                                                   // 9: 2 5
    (1 << 4) | (1 << 8),                                                   // 10: 4 8
    (1 << 0),                                                              // 11: 0
    (1 << 1) | (1 << 2) | (1 << 7),                                        // 12: 1 2 7
    (1 << 2),                                                              // 13: 2
};
__constant__ uint8_t SF_START[SF_N] = {0, 6, 11, 16, 20, 23, 25, 28, 32, 35, 37, 39, 40, 43};

struct SfGeom {
    int64_t B, G;                                // samples, graphs = B * T
    int T, P, C, Hd, E;
    int S, W;                                    // floats of one head's parameters: C P + C + 2 C + 1; the LSTM's input width T + 14 C
    int o_vw, o_vb, pcount;                      // flat parameter offsets (the heads start at 0; the back end's are the plan's)
    LstmHeadPlan lh;                             // one LSTM W -> E over the T patches, Linear(E, 1) on the last step
    int bwd_cap, part_rows;                      // workgroups of the backward at most (from the row width), its partial rows at most
    int64_t w_rows, w_d1, w_d2, w_part, w_split, total;      // workspace offsets (floats)
};

// ---- LDS layout of the attention kernels, stated once for kernel and launcher (floats, per wavefront = per graph in flight) ------------
// forward: x [14][P], Z [14][Hd C], s1, s2 [Hd][14] (a1 . Z_i, a2 . Z_i), hp [14][Hd C] (h' per head);
// backward: the same with dZ in hp's place, then m, d, r, ds1, ds2 [Hd][14] (row maximum, denominator, r_i = sum_j p_ij dp_ij, the two score
// gradients) and dh [14][C] (the gated d h' of one head: d out o [out > 0] / Hd).
struct SfLds {
    int x, z, s1, s2, hp, m, d, r, ds1, ds2, dh, total;
};
__host__ __device__ constexpr SfLds sf_lds(int P, int C, int Hd, bool bwd) {
    SfLds l{};
    int o = 0;
    const int hc = Hd * C, hn = Hd * SF_N;
    l.x = o; o += SF_N * P;
    l.z = o; o += SF_N * hc;
    l.s1 = o; o += hn;
    l.s2 = o; o += hn;
    l.hp = o; o += SF_N * hc;
    l.m = l.d = l.r = l.ds1 = l.ds2 = l.dh = o;
    if (bwd) {
        l.m = o; o += hn;
        l.d = o; o += hn;
        l.r = o; o += hn;
        l.ds1 = o; o += hn;
        l.ds2 = o; o += hn;
        l.dh = o; o += SF_N * C;
    }
    l.total = o;
    return l;
}
static_assert((size_t)sf_lds(RULGNN_STFA_MAX_PATCH_SIZE, SF_MAXC, RULGNN_STFA_MAX_HEADS, true).total * SF_WAVES * sizeof(float) <= MAX_LDS_BYTES,
              "the backward at every limit at once fits one compute unit's LDS");

int sf_geometry(const rulgnn_stfa_shape* s, SfGeom* g) {
    if (!s) return RULGNN_EINVAL;
    if (s->batch < 0 || s->num_patch < 1 || s->patch_size < 1 || s->num_nodes < 1 || s->output_dim < 1 || s->num_heads < 1 ||
        s->encoder_hidden_dim < 1)
        return RULGNN_EINVAL;
    if (s->num_nodes != SF_N || s->num_patch > RULGNN_STFA_MAX_NUM_PATCH || s->patch_size > RULGNN_STFA_MAX_PATCH_SIZE ||
        s->output_dim > SF_MAXC || s->num_heads > RULGNN_STFA_MAX_HEADS || s->encoder_hidden_dim > RULGNN_STFA_MAX_LSTM_HIDDEN)
        return RULGNN_EUNSUPPORTED;
    g->B = s->batch; g->T = s->num_patch; g->P = s->patch_size; g->C = s->output_dim; g->Hd = s->num_heads; g->E = s->encoder_hidden_dim;
    g->G = g->B * g->T;
    g->S = g->C * g->P + 3 * g->C + 1;
    g->W = g->T + SF_N * g->C;
    if (g->G * (int64_t)(g->W > g->E ? g->W : g->E) > 0x7fffffff) return RULGNN_EUNSUPPORTED;      // the LSTM's GEMMs take int extents
    int o = g->Hd * g->S;
    int64_t w = 0;
    SplitKScratch sp(1024);
    auto tk = [&](int n) { const int r = o; o += n; return r; };
    auto wk = [&](int64_t n) { const int64_t r = w; w += (n + 63) & ~(int64_t)63; return r; };
    g->o_vw = tk(SF_N * g->C); g->o_vb = tk(1);
    LstmHeadPlan& lh = g->lh;
    lh.B = g->B; lh.T = g->T; lh.nk = 1; lh.H[0] = g->W; lh.H[1] = g->E; lh.last_step = 1;
    g->w_rows = wk(g->G * g->W);
    RULGNN_TRY(lstm_head_layout(&lh, &o, &w, &sp));
    g->pcount = o;
    g->w_d1 = wk(g->G * (int64_t)(g->W > g->E ? g->W : g->E));
    g->w_d2 = wk(g->G * (int64_t)(g->W > g->E ? g->W : g->E));
    const int64_t blocks = (g->G + SF_WAVES - 1) / SF_WAVES;
    int64_t cap = SF_PART_FLOATS / ((int64_t)g->Hd * g->S) / SF_WAVES;      // a function of the shape alone: part of the bits
    cap = cap > SF_BWD_MAXGRID ? SF_BWD_MAXGRID : (cap < 64 ? 64 : cap);
    g->bwd_cap = (int)cap;
    g->part_rows = (int)(blocks < cap ? (blocks < 1 ? 1 : blocks) : cap) * SF_WAVES;
    g->w_part = wk((int64_t)g->part_rows * g->Hd * g->S);
    g->w_split = wk((int64_t)sp.floats());
    g->total = w;
    return RULGNN_OK;
}

struct SfAtt {
    int64_t G, g0;                    // graphs of this call; global index of its first SAMPLE (dropout counters)
    int T, P, C, Hd, S, W;
    const float *x, *prm;             // x [B][14][T P]; the heads' parameters, S floats each: linear.weight [C][P], linear.bias [C], attention.weight [2 C], attention.bias [1]
    float* rows;                      // [G][W]: forward writes [1 x T | relu(mean h') [14][C]]; backward reads the features (ReLU gate)
    const float* drows;               // backward: d rows [G][W]
    float* part;                      // backward: [gridDim.x * SF_WAVES][Hd S] partial rows
    uint32_t key, thr;                // dropout: keep where lowbias32(counter ^ key) >= thr
    float scale;                      // 1 / (1 - p); 0: no dropout
};

__device__ __forceinline__ float sf_lrelu(float u) { return u > 0.f ? u : SF_SLOPE * u; }
// keep mask / (1 - p) of directed edge `e` (row-major over the adjacency) of head h of graph gi = (sample, patch)
__device__ __forceinline__ float sf_keep(const SfAtt& q, int64_t gi, int h, int e) {
    if (q.scale == 0.f) return 1.f;
    const int64_t b = gi / q.T, t = gi % q.T;
    const uint32_t ctr = (uint32_t)(((((uint64_t)(q.g0 + b) * q.T + t) * q.Hd + h) * SF_EDGES) + e);
    return lowbias32(ctr ^ q.key) >= q.thr ? q.scale : 0.f;
}
__device__ __forceinline__ int sf_edge(int i, int j) { return SF_START[i] + __popc((uint32_t)SF_MASK[i] & ((1u << j) - 1u)); }

// x tile, Z of every head (bias added), s1 = a1 . Z_i and s2 = a2 . Z_i per head: the part both kernels share.  Ends in a barrier.
__device__ __forceinline__ void sf_project(const SfAtt& q, const SfLds& L, float* sm, int64_t gi, bool valid, int lane) {
    const int P = q.P, C = q.C, HC = q.Hd * q.C;
    if (valid) {
        const int64_t b = gi / q.T, t = gi % q.T;
        const float* xg = q.x + (b * SF_N * q.T + t) * P;              // node i: + i * T * P
        for (int k = lane; k < SF_N * P; k += SF_WAVE) sm[L.x + k] = xg[(int64_t)(k / P) * q.T * P + k % P];
    }
    __syncthreads();
    if (valid)
        for (int k = lane; k < SF_N * HC; k += SF_WAVE) {
            const int i = k / HC, hc = k % HC, h = hc / C, c = hc % C;
            const float* wr = q.prm + (size_t)h * q.S + c * P;
            const float* xr = sm + L.x + i * P;
            float acc = q.prm[(size_t)h * q.S + C * P + c];
            for (int p = 0; p < P; ++p) acc = fmaf(xr[p], wr[p], acc);
            sm[L.z + k] = acc;
        }
    __syncthreads();
    if (valid)
        for (int k = lane; k < q.Hd * SF_N; k += SF_WAVE) {
            const int h = k / SF_N, i = k % SF_N;
            const float* a = q.prm + (size_t)h * q.S + C * P + C;
            const float* zr = sm + L.z + i * HC + h * C;
            float p1 = 0.f, p2 = 0.f;
            for (int c = 0; c < C; ++c) { p1 = fmaf(a[c], zr[c], p1); p2 = fmaf(a[C + c], zr[c], p2); }
            sm[L.s1 + k] = p1;
            sm[L.s2 + k] = p2;
        }
    __syncthreads();
}

// row maximum and denominator of softmax_j(leakyrelu(si + s2_j)); a NaN score makes the denominator NaN (fmaxf skips it, the sum does not)
__device__ __forceinline__ void sf_row_stats(float si, const float* s2, float* mx, float* den) {
    float m = sf_lrelu(si + s2[0]);
#pragma unroll
    for (int j = 1; j < SF_N; ++j) m = fmaxf(m, sf_lrelu(si + s2[j]));
    float d = 0.f;
#pragma unroll
    for (int j = 0; j < SF_N; ++j) d += expf(sf_lrelu(si + s2[j]) - m);
    *mx = m;
    *den = d;
}

__global__ __launch_bounds__(SF_BLOCK) void sf_att_fwd_kernel(SfAtt q) {
    extern __shared__ __attribute__((aligned(16))) float sf_sm[];
    const int C = q.C, HC = q.Hd * q.C, lane = threadIdx.x % SF_WAVE, w = threadIdx.x / SF_WAVE;
    const SfLds L = sf_lds(q.P, C, q.Hd, false);
    float* sm = sf_sm + (size_t)w * L.total;
    // every wavefront of a workgroup walks the same number of rounds (the barriers are the workgroup's)
    for (int64_t base = (int64_t)blockIdx.x * SF_WAVES; base < q.G; base += (int64_t)gridDim.x * SF_WAVES) {
        const int64_t gi = base + w;
        const bool valid = gi < q.G;
        sf_project(q, L, sm, gi, valid, lane);
        if (valid)
            for (int k = lane; k < q.Hd * SF_N; k += SF_WAVE) {
                const int h = k / SF_N, i = k % SF_N;
                const float* s2 = sm + L.s2 + h * SF_N;
                const float si = sm[L.s1 + k] + q.prm[(size_t)h * q.S + C * q.P + 3 * C];
                float mx, den;
                sf_row_stats(si, s2, &mx, &den);
                float acc[SF_MAXC];
#pragma unroll
                for (int c = 0; c < SF_MAXC; ++c) acc[c] = 0.f;
                int e = SF_START[i];
                for (uint32_t m = SF_MASK[i]; m; m &= m - 1, ++e) {
                    const int j = __ffs(m) - 1;
                    const float qv = expf(sf_lrelu(si + s2[j]) - mx) / den * sf_keep(q, gi, h, e);
                    const float* zr = sm + L.z + j * HC + h * C;
#pragma unroll
                    for (int c = 0; c < SF_MAXC; ++c)
                        if (c < C) acc[c] = fmaf(qv, zr[c], acc[c]);
                }
                float* hr = sm + L.hp + i * HC + h * C;
#pragma unroll
                for (int c = 0; c < SF_MAXC; ++c)
                    if (c < C) hr[c] = acc[c];
            }
        __syncthreads();
        if (valid) {
            float* row = q.rows + gi * q.W;
            for (int k = lane; k < q.T; k += SF_WAVE) row[k] = 1.0f;      // the singleton softmax (Model.py:115)
            const float inv = 1.0f / (float)q.Hd;
            for (int k = lane; k < SF_N * C; k += SF_WAVE) {
                const float* hr = sm + L.hp + (k / C) * HC + k % C;
                float v = 0.f;
                for (int h = 0; h < q.Hd; ++h) v += hr[h * C];
                v *= inv;
                row[q.T + k] = v < 0.f ? 0.f : v;                         // (a NaN stays a NaN, as F.relu)
            }
        }
        __syncthreads();                                                  // the tile is rewritten by the next round
    }
}

__global__ __launch_bounds__(SF_BLOCK) void sf_att_bwd_kernel(SfAtt q) {
    extern __shared__ __attribute__((aligned(16))) float sf_sm[];
    const int P = q.P, C = q.C, HC = q.Hd * q.C, lane = threadIdx.x % SF_WAVE, w = threadIdx.x / SF_WAVE;
    const int nel = q.Hd * q.S;
    const SfLds L = sf_lds(P, C, q.Hd, true);
    float* sm = sf_sm + (size_t)w * L.total;
    // this wavefront's partial row: element e is lane e % 64's from the first write to the last (program order, no atomics)
    float* prow = q.part + ((size_t)blockIdx.x * SF_WAVES + w) * nel;
    for (int e = lane; e < nel; e += SF_WAVE) prow[e] = 0.f;
    for (int64_t base = (int64_t)blockIdx.x * SF_WAVES; base < q.G; base += (int64_t)gridDim.x * SF_WAVES) {
        const int64_t gi = base + w;
        const bool valid = gi < q.G;
        if (valid) {
            const float* orow = q.rows + gi * q.W + q.T;
            const float* drow = q.drows + gi * q.W + q.T;
            const float inv = 1.0f / (float)q.Hd;
            for (int k = lane; k < SF_N * C; k += SF_WAVE) sm[L.dh + k] = orow[k] > 0.f ? drow[k] * inv : 0.f;
        }
        sf_project(q, L, sm, gi, valid, lane);
        // rows: m_i, d_i, r_i = sum_j p_ij dp_ij with dp_ij = adj_ij keep_ij (dh_i . Z_j), ds1_i = sum_j p_ij (dp_ij - r_i) leakyrelu'(u_ij)
        if (valid)
            for (int k = lane; k < q.Hd * SF_N; k += SF_WAVE) {
                const int h = k / SF_N, i = k % SF_N;
                const float* s2 = sm + L.s2 + h * SF_N;
                const float si = sm[L.s1 + k] + q.prm[(size_t)h * q.S + C * P + 3 * C];
                float mx, den;
                sf_row_stats(si, s2, &mx, &den);
                float pl = 0.f;                                           // sum_j p_ij leakyrelu'(u_ij)
#pragma unroll
                for (int j = 0; j < SF_N; ++j) {
                    const float u = si + s2[j];
                    pl += expf(sf_lrelu(u) - mx) / den * (u > 0.f ? 1.f : SF_SLOPE);
                }
                const float* dh = sm + L.dh + i * C;
                float r = 0.f, a = 0.f;                                   // a = sum_nbr p_ij leakyrelu'(u_ij) dp_ij
                int e = SF_START[i];
                for (uint32_t m = SF_MASK[i]; m; m &= m - 1, ++e) {
                    const int j = __ffs(m) - 1;
                    const float* zr = sm + L.z + j * HC + h * C;
                    float dot = 0.f;
                    for (int c = 0; c < C; ++c) dot = fmaf(dh[c], zr[c], dot);
                    const float u = si + s2[j];
                    const float p = expf(sf_lrelu(u) - mx) / den, dp = sf_keep(q, gi, h, e) * dot;
                    r = fmaf(p, dp, r);
                    a = fmaf(p * (u > 0.f ? 1.f : SF_SLOPE), dp, a);
                }
                sm[L.m + k] = mx;
                sm[L.d + k] = den;
                sm[L.r + k] = r;
                sm[L.ds1 + k] = a - r * pl;
            }
        __syncthreads();
        // columns: ds2_j = sum_i p_ij (dp_ij - r_i) leakyrelu'(u_ij); dZ_j = sum_{i ~ j} q_ij dh_i + ds1_j a1 + ds2_j a2
        if (valid)
            for (int k = lane; k < q.Hd * SF_N; k += SF_WAVE) {
                const int h = k / SF_N, j = k % SF_N;
                const float cb = q.prm[(size_t)h * q.S + C * P + 3 * C];
                const float s2j = sm[L.s2 + k];
                const float* s1 = sm + L.s1 + h * SF_N;
                const float* mxs = sm + L.m + h * SF_N;
                const float* dens = sm + L.d + h * SF_N;
                const float* rs = sm + L.r + h * SF_N;
                const float* zj = sm + L.z + j * HC + h * C;
                float ds2 = 0.f;
#pragma unroll
                for (int i = 0; i < SF_N; ++i) {
                    const float u = s1[i] + cb + s2j;
                    ds2 -= expf(sf_lrelu(u) - mxs[i]) / dens[i] * (u > 0.f ? 1.f : SF_SLOPE) * rs[i];
                }
                float acc[SF_MAXC];
#pragma unroll
                for (int c = 0; c < SF_MAXC; ++c) acc[c] = 0.f;
                for (uint32_t m = SF_MASK[j]; m; m &= m - 1) {            // (the graph is undirected: column j's rows are row j's columns)
                    const int i = __ffs(m) - 1;
                    const float* dh = sm + L.dh + i * C;
                    float dot = 0.f;
                    for (int c = 0; c < C; ++c) dot = fmaf(dh[c], zj[c], dot);
                    const float u = s1[i] + cb + s2j;
                    const float p = expf(sf_lrelu(u) - mxs[i]) / dens[i], kp = sf_keep(q, gi, h, sf_edge(i, j));
                    ds2 = fmaf(p * (u > 0.f ? 1.f : SF_SLOPE), kp * dot, ds2);
                    const float qv = p * kp;
#pragma unroll
                    for (int c = 0; c < SF_MAXC; ++c)
                        if (c < C) acc[c] = fmaf(qv, dh[c], acc[c]);
                }
                const float ds1 = sm[L.ds1 + k];
                const float* a = q.prm + (size_t)h * q.S + C * P + C;
                float* dz = sm + L.hp + j * HC + h * C;
#pragma unroll
                for (int c = 0; c < SF_MAXC; ++c)
                    if (c < C) dz[c] = fmaf(ds2, a[C + c], fmaf(ds1, a[c], acc[c]));
                sm[L.ds2 + k] = ds2;
            }
        __syncthreads();
        // this graph's parameter gradients, in the flat order of a head: dW [C][P] = dZ^T x, db = sum_j dZ_j, da1 = sum_j ds1_j Z_j,
        // da2 = sum_j ds2_j Z_j, dc = sum_j ds1_j
        if (valid)
            for (int e = lane; e < nel; e += SF_WAVE) {
                const int h = e / q.S, r = e % q.S;
                float v = 0.f;
                if (r < C * P) {
                    const int c = r / P, p = r % P;
                    for (int j = 0; j < SF_N; ++j) v = fmaf(sm[L.hp + j * HC + h * C + c], sm[L.x + j * P + p], v);
                } else if (r < C * P + C) {
                    const int c = r - C * P;
                    for (int j = 0; j < SF_N; ++j) v += sm[L.hp + j * HC + h * C + c];
                } else if (r < C * P + 3 * C) {
                    const bool first = r < C * P + 2 * C;
                    const int c = r - C * P - (first ? C : 2 * C);
                    const float* ds = sm + (first ? L.ds1 : L.ds2) + h * SF_N;
                    for (int j = 0; j < SF_N; ++j) v = fmaf(ds[j], sm[L.z + j * HC + h * C + c], v);
                } else {
                    for (int j = 0; j < SF_N; ++j) v += sm[L.ds1 + h * SF_N + j];
                }
                prow[e] += v;
            }
        __syncthreads();                                                  // the tile is rewritten by the next round
    }
}

// launch geometry of an attention kernel: LDS bytes, workgroups (fixed by the shape and the device)
struct SfLaunch {
    int grid;
    size_t lds;
};
template <typename K>
int sf_att_launch(K kernel, const SfGeom& g, bool bwd, SfLaunch* L) {
    L->lds = (size_t)sf_lds(g.P, g.C, g.Hd, bwd).total * SF_WAVES * sizeof(float);
    RULGNN_TRY(allow_dynamic_lds(kernel, L->lds));
    L->grid = resident_rows(kernel, SF_BLOCK, L->lds, (g.G + SF_WAVES - 1) / SF_WAVES, bwd ? g.bwd_cap : SF_FWD_MAXGRID);
    return RULGNN_OK;
}

}  // namespace

// RULGNN_OK, or the code every entry returns for a refused shape: RULGNN_EINVAL for a value that is no shape at all (a null pointer, a
// negative batch, an extent below 1), RULGNN_EUNSUPPORTED beyond a limit or for num_nodes != 14.
int Stfa::shape_status(const Shape* s) {
    SfGeom g;
    return sf_geometry(s, &g);
}

int64_t Stfa::param_count(const Shape* s) {
    SfGeom g;
    return sf_geometry(s, &g) == RULGNN_OK ? g.pcount : -1;
}

size_t Stfa::workspace_bytes(const Shape* s) {
    SfGeom g;
    return sf_geometry(s, &g) == RULGNN_OK ? (size_t)g.total * sizeof(float) : 0;
}

int64_t Stfa::tap_offset(const Shape* s, int which) {
    SfGeom g;
    if (sf_geometry(s, &g) != RULGNN_OK) return -1;
    if (which == RULGNN_STFA_TAP_ROWS) return g.w_rows;
    if (which == RULGNN_STFA_TAP_LSTM) return g.lh.w_hseq[0];
    return -1;
}

// mode bit 0: forward, bit 1: backward (after a forward with the same args / workspace)
int Stfa::run(const Shape* s, const Args* a, int mode, hipStream_t st) {
    SfGeom g;
    RULGNN_TRY(sf_geometry(s, &g));
    if (a->workspace_bytes < (size_t)g.total * sizeof(float)) return RULGNN_EWORKSPACE;
    if (g.B == 0) return RULGNN_OK;
    float* ws = static_cast<float*>(a->workspace);
    const float* prm = a->params;
    const int64_t gb = a->global_batch > 0 ? a->global_batch : g.B;
    const float inv_gb = 1.0f / (float)gb;
    SfAtt q{};
    q.G = g.G; q.g0 = a->sample_offset; q.T = g.T; q.P = g.P; q.C = g.C; q.Hd = g.Hd; q.S = g.S; q.W = g.W;
    q.x = a->x; q.prm = prm; q.rows = ws + g.w_rows;
    const DropoutConst dc = dropout_const(a->training ? a->dropout_p : 0.f);
    q.thr = dc.thr; q.scale = dc.thr ? dc.scale : 0.f;
    q.key = dropout_layer_key(a->seed, a->step, 0);
    // the path is picked before any launch: both kernels' LDS requests and grids
    SfLaunch Lf{}, Lb{};
    if (mode & 1) RULGNN_TRY(sf_att_launch(sf_att_fwd_kernel, g, false, &Lf));
    if (mode & 2) {
        if (!a->grads) return RULGNN_EINVAL;
        RULGNN_TRY(sf_att_launch(sf_att_bwd_kernel, g, true, &Lb));
        if (Lb.grid * SF_WAVES > g.part_rows) return RULGNN_EWORKSPACE;
    }
    if (mode & 1) {
        RULGNN_TRY(launch_checked(sf_att_fwd_kernel, dim3(Lf.grid), dim3(SF_BLOCK), Lf.lds, st, q));
        RULGNN_TRY(lstm_head_forward(g.lh, ws + g.w_rows, prm, ws, a->y, a->pred, inv_gb, st));
        if (a->y && a->loss) RULGNN_TRY(block_sum((const float*)(ws + g.lh.w_sq), g.B, a->loss, st));
    }
    if (mode & 2) {
        float* gr = a->grads;
        const float* dpred = a->dpred ? a->dpred : ws + g.lh.w_dpred;
        RULGNN_TRY(fill_f32(ws + g.lh.w_one, 1, 1.0f, st));
        float* const dbuf[2] = {ws + g.w_d1, ws + g.w_d2};
        RULGNN_TRY(lstm_head_backward(g.lh, ws + g.w_rows, prm, ws, dpred, gr, dbuf, ws + g.w_split, st));
        // v reaches the loss through a softmax over one element: its gradient is exactly zero (and v stays a live Adam parameter)
        RULGNN_TRY(fill_f32(gr + g.o_vw, SF_N * g.C + 1, 0.0f, st));
        q.drows = dbuf[1];                           // (one LSTM layer: d x is left in dbuf[nk & 1])
        q.part = ws + g.w_part;
        RULGNN_TRY(launch_checked(sf_att_bwd_kernel, dim3(Lb.grid), dim3(SF_BLOCK), Lb.lds, st, q));
        // the partial rows are in the flat order of the heads' parameters, which open the buffer: one fixed-order sum
        RULGNN_TRY(rows_sum(ws + g.w_part, Lb.grid * SF_WAVES, g.Hd * g.S, g.Hd * g.S, gr, st));
    }
    return RULGNN_OK;
}

}  // namespace rulgnn
