// One-layer GRU over A FEW HUNDRED MEDIUM-LENGTH sequences for gfx950 (GRU_CM: batch = 100 .. 4096 sequences of 50 steps, hidden 64):
// nn.GRU(input_dim, 64, batch_first=True), h0 = 0, gate order (r, z, n); forward and backward.  Same arithmetic as csrc/gru.hip:1-13.
//
// The regime between csrc/gru.hip (100 k sequences of 1-5 steps: a GEMM launch + a gate launch per step, the step loop on the host) and
// csrc/bilstm.hip (a handful of sequences of thousands of steps): here the step loop of gru.hip is ~250 dependent launches per training
// step on [100 x 64] tiles.  The sequences are independent, so ONE launch walks all steps: a workgroup owns a tile of 16 sequences,
//   * W_hh stays in registers for the whole launch: wavefront w owns hidden units 16w .. 16w+15 of the three gates, lane l holds
//     W_hh[gate*64 + 16w + (l & 15)][16 (l >> 4) .. +16] -- 48 values, the B operands of v_mfma_f32_16x16x4_f32;
//   * h_{t-1} of the tile sits in LDS (ping-pong, one barrier per step) and is the A operand: gh_t = h_{t-1} W_hh^T is 48 matrix
//     instructions per wavefront and step (three independent accumulators), the gates follow in the accumulator registers, where lane l
//     holds unit 16w + (l & 15) of sequences 4 (l >> 4) .. +4 -- the same lane keeps that unit's previous state;
//   * no cross-workgroup synchronisation.
// The k index of a matrix instruction is free as long as both operands agree: step s of lane group q = l >> 4 stands for k = 16 q + s, so
// that a lane's sixteen A values are contiguous in LDS (four 16-byte reads).
// The input projection of ALL steps is one GEMM in front; the forward leaves the tape (gi, gh without biases, h_{t-1}).  Backward: the same
// ownership walking the steps in reverse -- gates recomputed from the tape, d h carried in registers, d gh_t of the tile through LDS as the
// A operand of d h_{t-1} += d gh_t W_hh (again 48 instructions per wavefront and step); the d gi / d gh rows go to memory and the four
// weight-gradient products over all (sequence, step) rows are one batched split-K pair at the end (fixed reduction order: deterministic).
#include "sgemm_mfma.hpp"
#include "families_host.hpp"

namespace rulgnn {

namespace {

constexpr int GS_H = 64, GS_H3 = 192, GS_TILE = 16, GS_BLOCK = 256;
constexpr int GS_HS = 68;      // LDS row stride of the state tile (floats): 16-byte aligned rows
constexpr int GS_DS = 196;     // ... of the d gh tile

struct GsGeom {
    int64_t S, R;      // sequences, rows = S * L
    int L, I;
};

__host__ int gs_geometry(const rulgnn_gru_shape* s, GsGeom* g) {
    if (!s) return RULGNN_EINVAL;
    if (s->num_seq < 0 || s->seq_len < 1 || s->input_dim < 1 || s->hidden_dim < 1) return RULGNN_EINVAL;
    if (s->hidden_dim != GS_H || s->input_dim > 64 || s->seq_len > 1024) return RULGNN_EUNSUPPORTED;
    if (s->num_seq * (int64_t)s->seq_len * GS_H3 > ((int64_t)1 << 31) - 1) return RULGNN_EUNSUPPORTED;   // GEMM indices are int
    g->S = s->num_seq;
    g->L = s->seq_len;
    g->I = s->input_dim;
    g->R = g->S * g->L;
    return RULGNN_OK;
}

__device__ __forceinline__ float gs_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }
__device__ __forceinline__ f32x4t gs_mfma(float a, float b, f32x4t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// sixteen consecutive floats of a 16-byte aligned LDS row
__device__ __forceinline__ void gs_read16(const float* p, float (&a)[16]) {
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const float4 q = *reinterpret_cast<const float4*>(p + 4 * v);
        a[4 * v] = q.x; a[4 * v + 1] = q.y; a[4 * v + 2] = q.z; a[4 * v + 3] = q.w;
    }
}

__global__ __launch_bounds__(GS_BLOCK) void gru_seq_fwd_kernel(GsGeom g, const float* __restrict__ gi, const float* __restrict__ w_hh,
                                                               const float* __restrict__ b_ih, const float* __restrict__ b_hh,
                                                               float* __restrict__ out, float* __restrict__ gh, float* __restrict__ hprev) {
    __shared__ __attribute__((aligned(16))) float hs[2][GS_TILE * GS_HS];
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, col = l & 15, kq = l >> 4;
    const int j = 16 * w + col;                                   // the hidden unit of this lane's results
    const int64_t s0 = (int64_t)blockIdx.x * GS_TILE;
    float wb[3][16];
#pragma unroll
    for (int gate = 0; gate < 3; ++gate)
#pragma unroll
        for (int s = 0; s < 16; ++s) wb[gate][s] = w_hh[(gate * GS_H + j) * GS_H + 16 * kq + s];
    const float br = b_ih[j] + b_hh[j], bz = b_ih[GS_H + j] + b_hh[GS_H + j], bin = b_ih[2 * GS_H + j], bhn = b_hh[2 * GS_H + j];
    for (int e = tid; e < 2 * GS_TILE * GS_HS; e += GS_BLOCK) (&hs[0][0])[e] = 0.f;
    int64_t rowbase[4];
    bool ok[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t seq = s0 + 4 * kq + q;
        ok[q] = seq < g.S;
        rowbase[q] = (ok[q] ? seq : g.S - 1) * g.L;               // rows beyond the last sequence compute on a copy of it and store nothing
    }
    float hp[4] = {0.f, 0.f, 0.f, 0.f};
    __syncthreads();
    for (int t = 0; t < g.L; ++t) {
        const float* hb = hs[t & 1];
        float* hn = hs[(t + 1) & 1];
        float gir[4], giz[4], gin[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {                             // issued ahead of the matrix chain that hides them
            const float* p = gi + (rowbase[q] + t) * GS_H3;
            gir[q] = p[j]; giz[q] = p[GS_H + j]; gin[q] = p[2 * GS_H + j];
        }
        float a[16];
        gs_read16(hb + col * GS_HS + 16 * kq, a);
        f32x4t ar = {0.f, 0.f, 0.f, 0.f}, az = {0.f, 0.f, 0.f, 0.f}, an = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            ar = gs_mfma(a[s], wb[0][s], ar);
            az = gs_mfma(a[s], wb[1][s], az);
            an = gs_mfma(a[s], wb[2][s], an);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float r = gs_sigmoid(gir[q] + ar[q] + br);
            const float z = gs_sigmoid(giz[q] + az[q] + bz);
            const float n = tanhf(gin[q] + bin + r * (an[q] + bhn));
            const float h = (1.f - z) * n + z * hp[q];
            hn[(4 * kq + q) * GS_HS + j] = h;
            if (ok[q]) {
                const int64_t row = rowbase[q] + t;
                out[row * GS_H + j] = h;
                hprev[row * GS_H + j] = hp[q];
                float* gr = gh + row * GS_H3;
                gr[j] = ar[q]; gr[GS_H + j] = az[q]; gr[2 * GS_H + j] = an[q];
            }
            hp[q] = h;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(GS_BLOCK) void gru_seq_bwd_kernel(GsGeom g, const float* __restrict__ gi, const float* __restrict__ gh,
                                                               const float* __restrict__ hprev, const float* __restrict__ w_hh,
                                                               const float* __restrict__ b_ih, const float* __restrict__ b_hh,
                                                               const float* __restrict__ dout, float* __restrict__ dgi, float* __restrict__ dgh) {
    __shared__ __attribute__((aligned(16))) float ds[2][GS_TILE * GS_DS];
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, col = l & 15, kq = l >> 4;
    const int j = 16 * w + col;
    const int64_t s0 = (int64_t)blockIdx.x * GS_TILE;
    float wb[3][16];                                              // W_hh[gate*64 + 16 kq + s][j]: d h[j] = sum_q d gh[q] W_hh[q][j]
#pragma unroll
    for (int gate = 0; gate < 3; ++gate)
#pragma unroll
        for (int s = 0; s < 16; ++s) wb[gate][s] = w_hh[(gate * GS_H + 16 * kq + s) * GS_H + j];
    const float br = b_ih[j] + b_hh[j], bz = b_ih[GS_H + j] + b_hh[GS_H + j], bin = b_ih[2 * GS_H + j], bhn = b_hh[2 * GS_H + j];
    int64_t rowbase[4];
    bool ok[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t seq = s0 + 4 * kq + q;
        ok[q] = seq < g.S;
        rowbase[q] = (ok[q] ? seq : g.S - 1) * g.L;
    }
    float dh[4] = {0.f, 0.f, 0.f, 0.f};
    for (int t = g.L - 1; t >= 0; --t) {
        float* db = ds[t & 1];
        float vgi[4][3], vgh[4][3], vhp[4], vdo[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {                             // every load of the step ahead of the arithmetic that selects on it
            const int64_t row = rowbase[q] + t;
            const float* p = gi + row * GS_H3;
            const float* c = gh + row * GS_H3;
            vgi[q][0] = p[j]; vgi[q][1] = p[GS_H + j]; vgi[q][2] = p[2 * GS_H + j];
            vgh[q][0] = c[j]; vgh[q][1] = c[GS_H + j]; vgh[q][2] = c[2 * GS_H + j];
            vhp[q] = hprev[row * GS_H + j];
            vdo[q] = dout[row * GS_H + j];
        }
        f32x4t acc0, acc1 = {0.f, 0.f, 0.f, 0.f}, acc2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float ghn = vgh[q][2] + bhn;
            const float r = gs_sigmoid(vgi[q][0] + vgh[q][0] + br);
            const float z = gs_sigmoid(vgi[q][1] + vgh[q][1] + bz);
            const float n = tanhf(vgi[q][2] + bin + r * ghn);
            const float gg = ok[q] ? vdo[q] + dh[q] : 0.f;
            const float dn = gg * (1.f - z);
            const float dz = gg * (vhp[q] - n);
            const float dpn = dn * (1.f - n * n);
            const float dpr = dpn * ghn * r * (1.f - r);
            const float dpz = dz * z * (1.f - z);
            float* dr = db + (4 * kq + q) * GS_DS;
            dr[j] = dpr; dr[GS_H + j] = dpz; dr[2 * GS_H + j] = dpn * r;
            if (ok[q]) {
                const int64_t row = rowbase[q] + t;
                float* a = dgi + row * GS_H3;
                float* b = dgh + row * GS_H3;
                a[j] = dpr; a[GS_H + j] = dpz; a[2 * GS_H + j] = dpn;
                b[j] = dpr; b[GS_H + j] = dpz; b[2 * GS_H + j] = dpn * r;
            }
            acc0[q] = gg * z;                                     // the direct path to h_{t-1}
        }
        __syncthreads();
        if (t > 0) {
#pragma unroll
            for (int gate = 0; gate < 3; ++gate) {
                float a[16];
                gs_read16(db + col * GS_DS + gate * GS_H + 16 * kq, a);
#pragma unroll
                for (int s = 0; s < 16; s += 3) {
                    acc0 = gs_mfma(a[s], wb[gate][s], acc0);
                    if (s + 1 < 16) acc1 = gs_mfma(a[s + 1], wb[gate][s + 1], acc1);
                    if (s + 2 < 16) acc2 = gs_mfma(a[s + 2], wb[gate][s + 2], acc2);
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) dh[q] = acc0[q] + (acc1[q] + acc2[q]);
        }
    }
}

struct GsWs {
    size_t gi, gh, hprev, dgi, dgh, one, split, split_floats, total;
};

void gs_jobs(const GsGeom& g, SplitKJob (&jobs)[4]) {             // shapes only: the scratch the batched split-K needs
    const int K = (int)g.R;
    jobs[0] = SplitKJob{nullptr, 1, GS_H3, nullptr, 1, g.I, nullptr, g.I, GS_H3, g.I, K};
    jobs[1] = SplitKJob{nullptr, 1, GS_H3, nullptr, 1, GS_H, nullptr, GS_H, GS_H3, GS_H, K};
    jobs[2] = SplitKJob{nullptr, 1, GS_H3, nullptr, 0, 1, nullptr, 1, GS_H3, 1, K};
    jobs[3] = jobs[2];
}

void gs_ws(const GsGeom& g, GsWs* w) {
    WsCarver c;
    const size_t R = (size_t)g.R;
    w->gi = c.take<float>(R * GS_H3);            // tape: W_ih x (no bias)
    w->gh = c.take<float>(R * GS_H3);            // tape: W_hh h_{t-1} (no bias)
    w->hprev = c.take<float>(R * GS_H);          // tape: h_{t-1}
    w->dgi = c.take<float>(R * GS_H3);
    w->dgh = c.take<float>(R * GS_H3);
    w->one = c.take<float>(R > 0 ? R : 1);
    SplitKJob jobs[4];
    gs_jobs(g, jobs);
    w->split_floats = g.R > 0 ? sgemm_splitk_batch_floats(jobs, 4) : 1;
    w->split = c.take<float>(w->split_floats);
    w->total = c.total();
}

inline unsigned gs_tiles(const GsGeom& g) { return (unsigned)((g.S + GS_TILE - 1) / GS_TILE); }

}  // namespace

size_t gru_persistent_workspace_bytes(const rulgnn_gru_shape* s) {
    GsGeom g;
    if (gs_geometry(s, &g) != RULGNN_OK) return 0;
    GsWs w;
    gs_ws(g, &w);
    return w.total;
}

int gru_persistent_forward(const rulgnn_gru_shape* s, const rulgnn_gru_args* a, hipStream_t st) {
    GsGeom g;
    RULGNN_TRY(gs_geometry(s, &g));
    GsWs w;
    gs_ws(g, &w);
    if (!a->workspace || a->workspace_bytes < w.total) return RULGNN_EWORKSPACE;
    if (g.S == 0) return RULGNN_OK;
    const Workspace ws(a->workspace);
    auto Fp = [&](size_t off) { return ws.at<float>(off); };
    // gi[row][q] = sum_i x[row][i] W_ih[q][i]
    RULGNN_TRY(sgemm(a->x, g.I, 1, a->w_ih, g.I, 1, Fp(w.gi), GS_H3, (int)g.R, GS_H3, g.I, false, st));
    return launch_checked(gru_seq_fwd_kernel, dim3(gs_tiles(g)), dim3(GS_BLOCK), 0, st, g, (const float*)Fp(w.gi), a->w_hh, a->b_ih, a->b_hh,
                          a->out, Fp(w.gh), Fp(w.hprev));
}

int gru_persistent_backward(const rulgnn_gru_shape* s, const rulgnn_gru_args* a, hipStream_t st) {
    GsGeom g;
    RULGNN_TRY(gs_geometry(s, &g));
    GsWs w;
    gs_ws(g, &w);
    if (!a->workspace || a->workspace_bytes < w.total) return RULGNN_EWORKSPACE;
    if (g.S == 0) {
        if (hipMemsetAsync(a->dw_ih, 0, sizeof(float) * GS_H3 * g.I, st) != hipSuccess || hipMemsetAsync(a->dw_hh, 0, sizeof(float) * GS_H3 * GS_H, st) != hipSuccess ||
            hipMemsetAsync(a->db_ih, 0, sizeof(float) * GS_H3, st) != hipSuccess || hipMemsetAsync(a->db_hh, 0, sizeof(float) * GS_H3, st) != hipSuccess)
            return RULGNN_EHIP;
        return RULGNN_OK;
    }
    const Workspace ws(a->workspace);
    auto Fp = [&](size_t off) { return ws.at<float>(off); };
    RULGNN_TRY(launch_checked(gru_seq_bwd_kernel, dim3(gs_tiles(g)), dim3(GS_BLOCK), 0, st, g, (const float*)Fp(w.gi), (const float*)Fp(w.gh),
                              (const float*)Fp(w.hprev), a->w_hh, a->b_ih, a->b_hh, a->dout, Fp(w.dgi), Fp(w.dgh)));
    RULGNN_TRY(fill_f32(Fp(w.one), g.R, 1.0f, st));
    // dW_ih[q][i] = sum_row dgi[row][q] x[row][i];  dW_hh[q][j] = sum_row dgh[row][q] hprev[row][j];  biases: column sums
    SplitKJob jobs[4];
    gs_jobs(g, jobs);
    jobs[0].A = Fp(w.dgi); jobs[0].B = a->x; jobs[0].C = a->dw_ih;
    jobs[1].A = Fp(w.dgh); jobs[1].B = Fp(w.hprev); jobs[1].C = a->dw_hh;
    jobs[2].A = Fp(w.dgi); jobs[2].B = Fp(w.one); jobs[2].C = a->db_ih;
    jobs[3].A = Fp(w.dgh); jobs[3].B = Fp(w.one); jobs[3].C = a->db_hh;
    RULGNN_TRY(sgemm_splitk_batch(jobs, 4, Fp(w.split), w.split_floats, st));
    if (a->dx)   // dx[row][i] = sum_q dgi[row][q] W_ih[q][i]
        RULGNN_TRY(sgemm(Fp(w.dgi), GS_H3, 1, a->w_ih, 1, g.I, a->dx, g.I, (int)g.R, g.I, GS_H3, false, st));
    return RULGNN_OK;
}

}  // namespace rulgnn
