// GRU_CM for gfx950 (reference models/GRU_CM/Model.py:6-82, algorithms/algorithms.py:355-380): the graph stage, the head and the
// family entries; the recurrence is csrc/gru_seq.hip (one launch over all steps) or csrc/gru.hip (the step loop).
//
// x [bs, N, L], h = N / 2.  Per (sample, time step) a graph of the N sensors with h channels:
//   x0_i = (x[b, i, t] w_in + b_in) . drop0                                       Linear(1, h), Dropout       (Model.py:61-65)
//   S_i  = sum_j relu(W_e [x0_i ; x0_j] + b_e)   over ALL j, j = i included      edge MLP + sum              (Model.py:22-32)
//   n_i  = relu(W_n [x0_i ; S_i] + b_n) . drop1                                   node MLP, Dropout           (Model.py:35-38,69)
//   pooled = max_i n_i                                                            max over the nodes          (Model.py:72)
// W_e [x_i ; x_j] = P_i + Q_j with P = W_e[:, :h] x0, Q = W_e[:, h:] x0, so the [bs, L, N, N, 2h] tensors of the reference are never
// formed: a lane owns one node (16 or 32 lanes per graph, several graphs per wavefront), keeps x0 / P / S in registers and meets the
// other nodes' Q through LDS.  Then nn.GRU(h, H) over the L steps, Dropout, Linear(H L, 1) (Model.py:74-80).
//
// Backward: one kernel reverses the graph stage from x and d pooled alone -- it recomputes x0, P, Q, the ReLU signs and the arg max
// (first index on ties, as torch.max; ties at 0 carry a zero derivative) --
//   dP_i = dS_i . sum_j 1[P_i + Q_j + b_e > 0],   dQ_j = sum_i dS_i . 1[P_i + Q_j + b_e > 0],
// and reduces the six parameter gradients in a fixed order: every lane stages its row of factors in LDS, thread e of the workgroup sums
// its (factor, factor) product over the workgroup's rows and keeps the sum in a register across the grid-stride loop, one partial row
// per workgroup, rows_sum at the end (sgemm.hip).  The head and its gradients are row dots / column sums.
//
// Dropout: the counter hash of the other families (stgcn_device.hpp lowbias32, key = dropout_layer_key(seed, step, site));
// sites 0, 1: counter (((b + sample_offset) L + t) N + i) h + c; site 2: ((b + sample_offset) L + t) H + c; both mod 2^32.
#include "sgemm_mfma.hpp"
#include "families_host.hpp"

namespace rulgnn {

namespace {

struct GcGeom {
    int64_t B, G;          // samples, graphs = B * L
    int N, L, h, H;
    int RW, HC, BLKB;      // lanes per graph, padded channel count of the instantiation, threads per workgroup of the backward kernel
};

__host__ int gc_geometry(const rulgnn_grucm_shape* s, GcGeom* g) {
    if (!s) return RULGNN_EINVAL;
    if (s->batch < 0 || s->num_nodes < 2 || s->time_length < 1 || s->gru_hidden_dim < 1) return RULGNN_EINVAL;
    if (s->num_nodes > 32 || s->time_length > 1024 || s->gru_hidden_dim > 1024) return RULGNN_EUNSUPPORTED;
    if ((int64_t)s->gru_hidden_dim * s->time_length > 65536) return RULGNN_EUNSUPPORTED;
    // 32-bit dropout counters and int GEMM indices
    if (s->batch * (int64_t)s->time_length * s->num_nodes * (s->num_nodes / 2) > ((int64_t)1 << 31) - 1) return RULGNN_EUNSUPPORTED;
    if (s->batch * (int64_t)s->time_length * 3 * s->gru_hidden_dim > ((int64_t)1 << 31) - 1) return RULGNN_EUNSUPPORTED;
    g->B = s->batch;
    g->N = s->num_nodes; g->L = s->time_length; g->h = g->N / 2; g->H = s->gru_hidden_dim;
    g->G = g->B * g->L;
    g->RW = g->N <= 16 ? 16 : 32;
    g->HC = g->h <= 4 ? 4 : (g->h <= 7 ? 7 : (g->h <= 10 ? 10 : 16));
    g->BLKB = g->HC == 4 ? 256 : (g->HC == 16 ? 64 : 128);       // keeps the backward kernel's staging rows within 64 KB of LDS
    return RULGNN_OK;
}

struct GcOff {
    int win, bin, we, be, wn, bn, wih, whh, bih, bhh, wout, bout, total, graph;   // graph: floats of the first six tensors
};
__host__ __device__ inline GcOff gc_offsets(int h, int H, int L) {
    GcOff o;
    int t = 0;
    o.win = t; t += h;
    o.bin = t; t += h;
    o.we = t; t += 2 * h * h;
    o.be = t; t += h;
    o.wn = t; t += 2 * h * h;
    o.bn = t; t += h;
    o.graph = t;
    o.wih = t; t += 3 * H * h;
    o.whh = t; t += 3 * H * H;
    o.bih = t; t += 3 * H;
    o.bhh = t; t += 3 * H;
    o.wout = t; t += H * L;
    o.bout = t; t += 1;
    o.total = t;
    return o;
}

struct GcDrop {
    uint32_t key[3], thr[3];
    float scale[3];
    uint32_t sample_offset;
};

__device__ __forceinline__ float gc_keep(const GcDrop& d, int site, uint32_t ctr) {
    if (d.thr[site] == 0u) return 1.f;
    return lowbias32(ctr ^ d.key[site]) >= d.thr[site] ? d.scale[site] : 0.f;
}

// LDS image of the six graph-stage tensors, channels padded to HC with zeros (a padded channel is 0 everywhere downstream)
template <int HC>
struct GcW {
    static constexpr int WIN = 0, BIN = HC, WE = 2 * HC, BE = WE + 2 * HC * HC, WN = BE + HC, BN = WN + 2 * HC * HC, COUNT = BN + HC;
};

template <int HC>
__device__ __forceinline__ void gc_load_weights(const GcGeom& g, const float* __restrict__ prm, float* wl, int tid, int nthreads) {
    using W = GcW<HC>;
    const GcOff o = gc_offsets(g.h, g.H, g.L);
    const int h = g.h;
    for (int e = tid; e < W::COUNT; e += nthreads) {
        float v = 0.f;
        if (e < W::WE) {
            const int c = e % HC;
            if (c < h) v = prm[(e < W::BIN ? o.win : o.bin) + c];
        } else if (e < W::BE || (e >= W::WN && e < W::BN)) {
            const bool edge = e < W::BE;
            const int r = e - (edge ? W::WE : W::WN), c = r / (2 * HC), k2 = r % (2 * HC), half = k2 / HC, k = k2 % HC;
            if (c < h && k < h) v = prm[(edge ? o.we : o.wn) + c * 2 * h + half * h + k];
        } else {
            const bool edge = e < W::WN;
            const int c = e - (edge ? W::BE : W::BN);
            if (c < h) v = prm[(edge ? o.be : o.bn) + c];
        }
        wl[e] = v;
    }
}

// what a lane knows of its node after the forward recompute
template <int HC>
struct GcNode {
    float xv, x0[HC], m0[HC], P[HC], Q[HC], S[HC], pre[HC], m1[HC];
};

// forward of node i of graph gidx up to the node MLP; `qs`: this graph's Q rows in LDS ([RW][HC + 1]); two barriers inside
template <int HC>
__device__ __forceinline__ void gc_node_forward(const GcGeom& g, const GcDrop& d, const float* wl, float* qs, int i, int64_t gidx, bool valid,
                                                float xv, GcNode<HC>& n) {
    using W = GcW<HC>;
    const uint32_t ctr0 = (((uint32_t)gidx + d.sample_offset * (uint32_t)g.L) * (uint32_t)g.N + (uint32_t)i) * (uint32_t)g.h;
    n.xv = xv;
#pragma unroll
    for (int c = 0; c < HC; ++c) {
        n.m0[c] = c < g.h ? gc_keep(d, 0, ctr0 + (uint32_t)c) : 1.f;
        n.m1[c] = c < g.h ? gc_keep(d, 1, ctr0 + (uint32_t)c) : 1.f;
        n.x0[c] = fmaf(xv, wl[W::WIN + c], wl[W::BIN + c]) * n.m0[c];
    }
#pragma unroll
    for (int c = 0; c < HC; ++c) {
        float p = 0.f, q = wl[W::BE + c];
#pragma unroll
        for (int k = 0; k < HC; ++k) {
            p = fmaf(wl[W::WE + c * 2 * HC + k], n.x0[k], p);
            q = fmaf(wl[W::WE + c * 2 * HC + HC + k], n.x0[k], q);
        }
        n.P[c] = p;
        n.Q[c] = q;
    }
    __syncthreads();                                   // the previous round's readers of qs are done
    if (valid) {
#pragma unroll
        for (int c = 0; c < HC; ++c) qs[i * (HC + 1) + c] = n.Q[c];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < HC; ++c) n.S[c] = 0.f;
    for (int j = 0; j < g.N; ++j) {
#pragma unroll
        for (int c = 0; c < HC; ++c) n.S[c] += fmaxf(n.P[c] + qs[j * (HC + 1) + c], 0.f);
    }
#pragma unroll
    for (int c = 0; c < HC; ++c) {
        float a = wl[W::BN + c];
#pragma unroll
        for (int k = 0; k < HC; ++k) {
            a = fmaf(wl[W::WN + c * 2 * HC + k], n.x0[k], a);
            a = fmaf(wl[W::WN + c * 2 * HC + HC + k], n.S[k], a);
        }
        n.pre[c] = a;
    }
}

template <int HC, int BLK>
__global__ __launch_bounds__(BLK) void grucm_graph_fwd_kernel(GcGeom g, GcDrop d, const float* __restrict__ x, const float* __restrict__ prm,
                                                              float* __restrict__ pooled) {
    __shared__ float wl[GcW<HC>::COUNT];
    __shared__ float qsm[BLK * (HC + 1)];
    const int tid = threadIdx.x, RW = g.RW, gl = tid / RW, i = tid % RW, GPB = BLK / RW;
    gc_load_weights<HC>(g, prm, wl, tid, BLK);
    __syncthreads();
    float* qs = qsm + gl * RW * (HC + 1);
    const int64_t rounds = (g.G + GPB - 1) / GPB;
    for (int64_t rd = blockIdx.x; rd < rounds; rd += gridDim.x) {
        const int64_t gidx = rd * GPB + gl;
        const bool gok = gidx < g.G, valid = gok && i < g.N;
        const int64_t b = gok ? gidx / g.L : 0;
        const int t = gok ? (int)(gidx % g.L) : 0;
        const float xv = valid ? x[(b * g.N + i) * g.L + t] : 0.f;
        GcNode<HC> n;
        gc_node_forward<HC>(g, d, wl, qs, i, gidx, valid, xv, n);
#pragma unroll
        for (int c = 0; c < HC; ++c) {
            float v = valid ? fmaxf(n.pre[c], 0.f) * n.m1[c] : -INFINITY;
            for (int off = RW >> 1; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, RW));
            if (i == 0 && gok && c < g.h) pooled[gidx * g.h + c] = v;
        }
    }
}

// row of factors a lane stages for the parameter-gradient sums: [da | x0 | S | dP | dQ | dpre | xv | 1]
template <int HC>
struct GcRow {
    static constexpr int DA = 0, X0 = HC, SS = 2 * HC, DP = 3 * HC, DQ = 4 * HC, DPRE = 5 * HC, XV = 6 * HC, ONE = 6 * HC + 1;
    static constexpr int STRIDE = (6 * HC + 2) | 1;                       // odd: lanes write their rows without bank conflicts
    static constexpr int ENTRIES = 4 * HC * HC + 4 * HC;                  // padded gradient entries
};

// entry e of the padded gradient -> the two factor columns of its product and its index among the first six tensors (-1: padding)
template <int HC>
__device__ __forceinline__ void gc_entry(int e, int h, int& ia, int& ib, int& dst) {
    using R = GcRow<HC>;
    if (e < 2 * HC * HC) {                                                // node MLP weight [c][k2]
        const int c = e / (2 * HC), k2 = e % (2 * HC), half = k2 / HC, k = k2 % HC;
        ia = R::DA + c; ib = R::X0 + k2;
        dst = c < h && k < h ? 3 * h + 2 * h * h + c * 2 * h + half * h + k : -1;
    } else if (e < 4 * HC * HC) {                                         // edge MLP weight [c][k2]
        const int r = e - 2 * HC * HC, c = r / (2 * HC), k2 = r % (2 * HC), half = k2 / HC, k = k2 % HC;
        ia = (half ? R::DQ : R::DP) + c; ib = R::X0 + k;
        dst = c < h && k < h ? 2 * h + c * 2 * h + half * h + k : -1;
    } else {
        const int r = e - 4 * HC * HC, which = r / HC, c = r % HC;
        if (which == 0) { ia = R::DPRE + c; ib = R::XV; dst = c; }                              // input_linear.weight
        else if (which == 1) { ia = R::DPRE + c; ib = R::ONE; dst = h + c; }                    // input_linear.bias
        else if (which == 2) { ia = R::DQ + c; ib = R::ONE; dst = 2 * h + 2 * h * h + c; }      // edge bias
        else { ia = R::DA + c; ib = R::ONE; dst = 3 * h + 4 * h * h + c; }                      // node bias
        if (c >= h) dst = -1;
    }
}

template <int HC, int BLK>
__global__ __launch_bounds__(BLK) void grucm_graph_bwd_kernel(GcGeom g, GcDrop d, const float* __restrict__ x, const float* __restrict__ prm,
                                                              const float* __restrict__ dpooled, float* __restrict__ part) {
    using W = GcW<HC>;
    using R = GcRow<HC>;
    constexpr int EPT = (R::ENTRIES + BLK - 1) / BLK;                     // gradient entries per thread
    __shared__ float wl[W::COUNT];
    __shared__ float qsm[BLK * (HC + 1)], psm[BLK * (HC + 1)], dsm[BLK * (HC + 1)];
    __shared__ float rows[BLK * R::STRIDE];
    const int tid = threadIdx.x, RW = g.RW, gl = tid / RW, i = tid % RW, GPB = BLK / RW;
    gc_load_weights<HC>(g, prm, wl, tid, BLK);
    float* qs = qsm + gl * RW * (HC + 1);
    float* ps = psm + gl * RW * (HC + 1);
    float* dss = dsm + gl * RW * (HC + 1);
    int ia[EPT], ib[EPT], dst[EPT];
    float acc[EPT];
#pragma unroll
    for (int u = 0; u < EPT; ++u) {
        const int e = tid + u * BLK;
        ia[u] = ib[u] = 0; dst[u] = -1; acc[u] = 0.f;
        if (e < R::ENTRIES) gc_entry<HC>(e, g.h, ia[u], ib[u], dst[u]);
    }
    __syncthreads();
    const int64_t rounds = (g.G + GPB - 1) / GPB;
    for (int64_t rd = blockIdx.x; rd < rounds; rd += gridDim.x) {
        const int64_t gidx = rd * GPB + gl;
        const bool gok = gidx < g.G, valid = gok && i < g.N;
        const int64_t b = gok ? gidx / g.L : 0;
        const int t = gok ? (int)(gidx % g.L) : 0;
        const float xv = valid ? x[(b * g.N + i) * g.L + t] : 0.f;
        float dp[HC];                                                     // every load ahead of the select that uses it
#pragma unroll
        for (int c = 0; c < HC; ++c) dp[c] = c < g.h ? dpooled[(gok ? gidx : 0) * g.h + c] : 0.f;
        GcNode<HC> n;
        gc_node_forward<HC>(g, d, wl, qs, i, gidx, valid, xv, n);
        // max over the nodes: the first index of the largest value takes the gradient
        float da[HC];
#pragma unroll
        for (int c = 0; c < HC; ++c) {
            float v = valid ? fmaxf(n.pre[c], 0.f) * n.m1[c] : -INFINITY;
            int idx = i;
            for (int off = RW >> 1; off > 0; off >>= 1) {
                const float ov = __shfl_xor(v, off, RW);
                const int oi = __shfl_xor(idx, off, RW);
                const bool take = ov > v || (ov == v && oi < idx);
                v = take ? ov : v;
                idx = take ? oi : idx;
            }
            da[c] = (valid && idx == i && n.pre[c] > 0.f) ? dp[c] * n.m1[c] : 0.f;
        }
        float dx0[HC], dS[HC];
#pragma unroll
        for (int k = 0; k < HC; ++k) {
            float a = 0.f, s = 0.f;
#pragma unroll
            for (int c = 0; c < HC; ++c) {
                a = fmaf(wl[W::WN + c * 2 * HC + k], da[c], a);
                s = fmaf(wl[W::WN + c * 2 * HC + HC + k], da[c], s);
            }
            dx0[k] = a;
            dS[k] = s;
        }
        if (valid) {
#pragma unroll
            for (int c = 0; c < HC; ++c) {
                ps[i * (HC + 1) + c] = n.P[c];
                dss[i * (HC + 1) + c] = dS[c];
            }
        }
        __syncthreads();
        float dP[HC], dQ[HC];
#pragma unroll
        for (int c = 0; c < HC; ++c) dP[c] = dQ[c] = 0.f;
        for (int j = 0; j < g.N; ++j) {
#pragma unroll
            for (int c = 0; c < HC; ++c) {
                dP[c] += (n.P[c] + qs[j * (HC + 1) + c] > 0.f) ? dS[c] : 0.f;
                const float pj = ps[j * (HC + 1) + c], dj = dss[j * (HC + 1) + c];
                dQ[c] += (pj + n.Q[c] > 0.f) ? dj : 0.f;
            }
        }
        float* row = rows + tid * R::STRIDE;
#pragma unroll
        for (int k = 0; k < HC; ++k) {
            float a = dx0[k];
#pragma unroll
            for (int c = 0; c < HC; ++c) {
                a = fmaf(wl[W::WE + c * 2 * HC + k], dP[c], a);
                a = fmaf(wl[W::WE + c * 2 * HC + HC + k], dQ[c], a);
            }
            row[R::DPRE + k] = valid ? a * n.m0[k] : 0.f;
        }
#pragma unroll
        for (int c = 0; c < HC; ++c) {
            row[R::DA + c] = da[c];
            row[R::X0 + c] = valid ? n.x0[c] : 0.f;               // (a lane without a node may hold anything: keep 0 x it finite)
            row[R::SS + c] = valid ? n.S[c] : 0.f;
            row[R::DP + c] = valid ? dP[c] : 0.f;
            row[R::DQ + c] = valid ? dQ[c] : 0.f;
        }
        row[R::XV] = xv;
        row[R::ONE] = 1.f;
        __syncthreads();
#pragma unroll
        for (int u = 0; u < EPT; ++u) {
            float s = 0.f;
            for (int r = 0; r < BLK; ++r) s = fmaf(rows[r * R::STRIDE + ia[u]], rows[r * R::STRIDE + ib[u]], s);
            acc[u] += s;
        }
        // (the next round's first barrier, inside gc_node_forward, separates these reads from the next writes of qs; rows / ps / dss are
        // written only behind that round's barriers)
    }
    const int PC = 4 * g.h * g.h + 4 * g.h;
#pragma unroll
    for (int u = 0; u < EPT; ++u)
        if (dst[u] >= 0) part[(int64_t)blockIdx.x * PC + dst[u]] = acc[u];
}

// ---- head: Dropout + Linear(H L, 1) (Model.py:75-80) ------------------------------------------------------------------------------
constexpr int GC_HB = 256;

// pred[b] = sum_q hs[b][q] keep(b, q) w[q] + bias; with y also d loss / d pred and the squared error
__global__ __launch_bounds__(GC_HB) void grucm_head_kernel(GcGeom g, GcDrop d, const float* __restrict__ hs, const float* __restrict__ w,
                                                           const float* __restrict__ bias, const float* __restrict__ y, float* __restrict__ pred,
                                                           float* __restrict__ dpred, float* __restrict__ sqerr, float inv_gb) {
    __shared__ float red[GC_HB];
    const int64_t b = blockIdx.x;
    const int Q = g.L * g.H;
    const uint32_t ctr0 = ((uint32_t)b + d.sample_offset) * (uint32_t)Q;
    float a = 0.f;
    for (int q = threadIdx.x; q < Q; q += GC_HB) a = fmaf(hs[b * Q + q] * gc_keep(d, 2, ctr0 + (uint32_t)q), w[q], a);
    red[threadIdx.x] = a;
    __syncthreads();
    for (int m = GC_HB / 2; m > 0; m >>= 1) {
        if ((int)threadIdx.x < m) red[threadIdx.x] += red[threadIdx.x + m];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float p = red[0] + bias[0];
        pred[b] = p;
        if (y) {
            const float e = p - y[b];
            dpred[b] = 2.f * e * inv_gb;
            sqerr[b] = e * e * inv_gb;
        }
    }
}

constexpr int GC_SLICE = 128;      // samples per column-sum slice

// d hs[b][q] = dpred[b] w[q] keep(b, q);  part[slice][q] = sum_{b in slice} dpred[b] hs[b][q] keep(b, q),  part[slice][Q] = sum dpred[b]
__global__ __launch_bounds__(GC_HB) void grucm_head_bwd_kernel(GcGeom g, GcDrop d, const float* __restrict__ hs, const float* __restrict__ w,
                                                               const float* __restrict__ dpred, float* __restrict__ dhs, float* __restrict__ part) {
    const int Q = g.L * g.H;
    const int q = blockIdx.x * GC_HB + threadIdx.x;
    const int64_t b0 = (int64_t)blockIdx.y * GC_SLICE;
    const int64_t b1 = b0 + GC_SLICE < g.B ? b0 + GC_SLICE : g.B;
    if (q > Q) return;
    float a = 0.f;
    if (q == Q) {
        for (int64_t b = b0; b < b1; ++b) a += dpred[b];
    } else {
        const float wq = w[q];
        for (int64_t b = b0; b < b1; ++b) {
            const float dpb = dpred[b], v = hs[b * Q + q];
            const float k = gc_keep(d, 2, ((uint32_t)b + d.sample_offset) * (uint32_t)Q + (uint32_t)q);
            a = fmaf(dpb, v * k, a);
            dhs[b * Q + q] = dpb * wq * k;
        }
    }
    part[(int64_t)blockIdx.y * (Q + 1) + q] = a;
}

struct GcWs {
    size_t pooled, hs, dhs, dpooled, dpred, sqerr, gpart, hpart, gru, total;
    size_t gru_bytes;
    int fblocks, gblocks, hslices;         // workgroups of the graph forward / backward kernels, column-sum slices of the head
};

constexpr int GC_MAX_BLOCKS = 1024;
constexpr int GC_FB = 256;        // threads per workgroup of the graph forward kernel

// the recurrence's path: the persistent kernel where it applies (measured faster at every batch of profiles/r11_grucm.md), else the step loop
bool gc_use_persistent(const GcGeom& g, int gru_path) {
    rulgnn_gru_shape gs{g.B, g.L, g.h, g.H};
    return gru_path != RULGNN_GRUCM_GRU_STEP_LOOP && gru_persistent_workspace_bytes(&gs) > 0;
}

void gc_ws(const GcGeom& g, GcWs* w) {
    const size_t G = (size_t)g.G, B = (size_t)(g.B > 0 ? g.B : 1);
    WsCarver c;
    w->pooled = c.take<float>(G * g.h);
    w->hs = c.take<float>(G * g.H);
    w->dhs = c.take<float>(G * g.H);
    w->dpooled = c.take<float>(G * g.h);
    w->dpred = c.take<float>(B);
    w->sqerr = c.take<float>(B);
    auto blocks = [&](int blk) {
        const int64_t rounds = (g.G + blk / g.RW - 1) / (blk / g.RW);
        return (int)(rounds < 1 ? 1 : (rounds > GC_MAX_BLOCKS ? GC_MAX_BLOCKS : rounds));
    };
    w->fblocks = blocks(GC_FB);
    w->gblocks = blocks(g.BLKB);
    w->gpart = c.take<float>((size_t)w->gblocks * (4 * g.h * g.h + 4 * g.h));
    w->hslices = (int)((B + GC_SLICE - 1) / GC_SLICE);
    w->hpart = c.take<float>((size_t)w->hslices * ((size_t)g.L * g.H + 1));
    // the larger of the two recurrences' needs: the path is a per-call switch (rulgnn_grucm_args.gru_path)
    rulgnn_gru_shape gs{g.B, g.L, g.h, g.H};
    const size_t loop = gru_workspace_bytes(&gs), pers = gru_persistent_workspace_bytes(&gs);
    w->gru_bytes = loop > pers ? loop : pers;
    w->gru = c.take_bytes(w->gru_bytes);
    w->total = c.total();
}

template <int HC, int BLK>
int gc_launch_graph(const GcGeom& g, const GcDrop& d, const GcWs& w, bool bwd, const float* x, const float* prm, float* pooled,
                    const float* dpooled, float* part, hipStream_t st) {
    if (!bwd) return launch_checked((grucm_graph_fwd_kernel<HC, GC_FB>), dim3(w.fblocks), dim3(GC_FB), 0, st, g, d, x, prm, pooled);
    return launch_checked((grucm_graph_bwd_kernel<HC, BLK>), dim3(w.gblocks), dim3(BLK), 0, st, g, d, x, prm, dpooled, part);
}

int gc_graph(const GcGeom& g, const GcDrop& d, const GcWs& w, bool bwd, const float* x, const float* prm, float* pooled, const float* dpooled,
             float* part, hipStream_t st) {
    switch (g.HC) {
    case 4: return gc_launch_graph<4, 256>(g, d, w, bwd, x, prm, pooled, dpooled, part, st);
    case 7: return gc_launch_graph<7, 128>(g, d, w, bwd, x, prm, pooled, dpooled, part, st);
    case 10: return gc_launch_graph<10, 128>(g, d, w, bwd, x, prm, pooled, dpooled, part, st);
    default: return gc_launch_graph<16, 64>(g, d, w, bwd, x, prm, pooled, dpooled, part, st);
    }
}

}  // namespace

// RULGNN_OK, or the code every entry returns for a refused shape: gc_geometry's own, and unsupported where the GRU layer underneath has no
// workspace for the sequence.
int Grucm::shape_status(const Shape* s) {
    GcGeom g;
    RULGNN_TRY(gc_geometry(s, &g));
    GcWs w;
    gc_ws(g, &w);
    return w.gru_bytes == 0 ? RULGNN_EUNSUPPORTED : RULGNN_OK;
}

int64_t Grucm::param_count(const Shape* s) {
    GcGeom g;
    if (gc_geometry(s, &g) != RULGNN_OK) return -1;
    return gc_offsets(g.h, g.H, g.L).total;
}

size_t Grucm::workspace_bytes(const Shape* s) {
    GcGeom g;
    if (gc_geometry(s, &g) != RULGNN_OK) return 0;
    GcWs w;
    gc_ws(g, &w);
    return w.gru_bytes == 0 ? 0 : w.total;
}

// mode bit 0: forward (pred; with y also d pred and the loss terms), bit 1: backward (gradients; d pred from args->dpred or from the
// forward of this call)
int Grucm::run(const Shape* s, const Args* a, int mode, hipStream_t st) {
    GcGeom g;
    RULGNN_TRY(gc_geometry(s, &g));
    GcWs w;
    gc_ws(g, &w);
    if (w.gru_bytes == 0) return RULGNN_EUNSUPPORTED;
    if (!a->workspace || a->workspace_bytes < w.total) return RULGNN_EWORKSPACE;
    const GcOff o = gc_offsets(g.h, g.H, g.L);
    if (g.B == 0) {
        if ((mode & 2) && hipMemsetAsync(a->grads, 0, sizeof(float) * o.total, st) != hipSuccess) return RULGNN_EHIP;
        if ((mode & 2) && a->loss && hipMemsetAsync(a->loss, 0, sizeof(float), st) != hipSuccess) return RULGNN_EHIP;
        return RULGNN_OK;
    }
    GcDrop d{};
    for (int site = 0; site < 3; ++site) {
        const DropoutConst dc = dropout_const(a->training ? a->dropout_p[site] : 0.f);
        d.thr[site] = dc.thr;
        d.scale[site] = dc.scale;
        d.key[site] = dropout_layer_key(a->seed, a->step, site);
    }
    d.sample_offset = (uint32_t)a->sample_offset;
    const Workspace ws(a->workspace);
    auto Fp = [&](size_t off) { return ws.at<float>(off); };
    const float* prm = a->params;
    const int Q = g.L * g.H;
    const bool persistent = gc_use_persistent(g, a->gru_path);
    if (a->gru_path == RULGNN_GRUCM_GRU_PERSISTENT && !persistent) return RULGNN_EUNSUPPORTED;      // (nothing launched yet)
    rulgnn_gru_shape gs{g.B, g.L, g.h, g.H};
    rulgnn_gru_args ga{};
    ga.w_ih = prm + o.wih; ga.w_hh = prm + o.whh; ga.b_ih = prm + o.bih; ga.b_hh = prm + o.bhh;
    ga.workspace = ws.at<void>(w.gru); ga.workspace_bytes = w.gru_bytes;
    ga.x = Fp(w.pooled);
    if (mode & 1) {
        RULGNN_TRY(gc_graph(g, d, w, false, a->x, prm, Fp(w.pooled), nullptr, nullptr, st));
        ga.out = Fp(w.hs);
        RULGNN_TRY(persistent ? gru_persistent_forward(&gs, &ga, st) : gru_forward(&gs, &ga, st));
        const float inv_gb = 1.0f / (float)(a->global_batch > 0 ? a->global_batch : g.B);
        RULGNN_TRY(launch_checked(grucm_head_kernel, dim3((unsigned)g.B), dim3(GC_HB), 0, st, g, d, (const float*)Fp(w.hs), prm + o.wout, prm + o.bout,
                                  a->y, a->pred, Fp(w.dpred), Fp(w.sqerr), inv_gb));
    }
    if (mode & 2) {
        const float* dpred = a->dpred ? a->dpred : Fp(w.dpred);
        float* gr = a->grads;
        RULGNN_TRY(launch_checked(grucm_head_bwd_kernel, dim3((unsigned)((Q + 1 + GC_HB - 1) / GC_HB), (unsigned)w.hslices), dim3(GC_HB), 0, st, g, d,
                                  (const float*)Fp(w.hs), prm + o.wout, dpred, Fp(w.dhs), w.hslices == 1 ? gr + o.wout : Fp(w.hpart)));
        if (w.hslices > 1) RULGNN_TRY(rows_sum(Fp(w.hpart), w.hslices, Q + 1, Q + 1, gr + o.wout, st));
        ga.dout = Fp(w.dhs); ga.dx = Fp(w.dpooled);
        ga.dw_ih = gr + o.wih; ga.dw_hh = gr + o.whh; ga.db_ih = gr + o.bih; ga.db_hh = gr + o.bhh;
        RULGNN_TRY(persistent ? gru_persistent_backward(&gs, &ga, st) : gru_backward(&gs, &ga, st));
        RULGNN_TRY(gc_graph(g, d, w, true, a->x, prm, nullptr, Fp(w.dpooled), Fp(w.gpart), st));
        RULGNN_TRY(rows_sum(Fp(w.gpart), w.gblocks, o.graph, o.graph, gr, st));
        if (!a->dpred && a->loss) RULGNN_TRY(block_sum((const float*)Fp(w.sqerr), g.B, a->loss, st));
    }
    return RULGNN_OK;
}

}  // namespace rulgnn
