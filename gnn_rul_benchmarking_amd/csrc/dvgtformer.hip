// DVGTformer for gfx950 (reference models/DVGTformer/Model.py, algorithms/algorithms.py:326-351): the fold / unfold launches, the fused
// encoder forward and backward, the head and the family entries.  The per-sample arithmetic and every layout are in
// dvgtformer_device.hpp.
//
// Fold: with X~ = [X | 1], W~ = [W | b], a head's scores are Q K^T / sqrt(d) = X~ M_h X~^T with M_h = W~q^T W~k / sqrt(d) ([Fa][Fa]) and
// its share of W_O's output is P_h X~ U_h with U_h = W~v^T W_O[:, h-slice]^T ([Fa][F]).  dv_fold_kernel builds all M and U (blocks x
// views x heads) and the positional-encoding constant once per call; the encoder kernels never form Q, K, V or the concatenation, so
// d_model (144 / 248) never meets the batch.  dv_unfold_kernel turns the batch sums dM, dU back into dWq, dbq, dWk, dWv, dbv, dW_O
// (one short dot product per element) and copies the gradients that were never folded; the K biases, whose gradient is zero in exact
// arithmetic (a K bias shifts a score row by a constant, which the softmax ignores), are written as exact zeros.
//
// Encoder kernels: one workgroup of DV_BLK (512) threads per sample, grid-strided; the sample's X, both graph softmaxes, a head's scores and
// softmaxes, the LayerNorm statistics and the FF hidden layer live in LDS for all 2 num_blocks half-blocks (DvLds).  The forward keeps
// the input of every half-block and the encoder output ([2 nb + 1][B][E] floats); the backward recomputes everything else.  Plain VALU
// throughout: the attention operands are [51 x 16] / [15 x 52] per head, whose 16 x 16 x 4 matrix-core tiles would be 6 to 30 % padding
// on one axis and would need the operands re-laid per view; the kernels are bound by LDS traffic and the row softmaxes, not by FMAs.
// Parameter gradients: each workgroup adds its samples, in order, into its own partial row (one owner thread per entry), rows_sum adds
// the rows in a fixed order: no floating-point atomics, two runs give the same bits.
//
// Dropout (temporal halves, train mode): the counter hash of the other families, key = dropout_layer_key(seed, step, block), counter =
// ((sample_offset + b) (L + 1) + l) (N + 1) + n mod 2^32; the backward redraws it.
#include "sgemm_mfma.hpp"
#include "families_host.hpp"
#include "dvgtformer_device.hpp"

namespace rulgnn {

namespace {

constexpr int DV_BLK = 512;                           // a half-block's phases are 765-3 672 independent outputs: eight wavefronts hide the LDS / L2 latency of one sample
constexpr int DV_MAX_ROWS = 256;                       // partial-gradient rows (= workgroups of the backward kernel) at most
constexpr int64_t DV_MAX_PART_FLOATS = (int64_t)1 << 26;

__host__ int dv_geometry(const rulgnn_dvgtformer_shape* s, DvGeom* g) {
    if (!s) return RULGNN_EINVAL;
    if (s->batch < 0 || s->num_nodes < 1 || s->time_length < 1 || s->num_heads < 1 || s->num_blocks < 1) return RULGNN_EINVAL;
    for (int v = 0; v < 2; ++v)
        if (s->d_model[v] < 1 || s->d_ff[v] < 1) return RULGNN_EINVAL;
    if (!(s->lambda_param >= 0.f && s->lambda_param <= 1.f)) return RULGNN_EINVAL;
    if (s->num_nodes < 2 || s->num_nodes > RULGNN_DVGT_MAX_NODES || s->time_length > RULGNN_DVGT_MAX_TIME ||
        s->num_heads > RULGNN_DVGT_MAX_HEADS || s->num_blocks > RULGNN_DVGT_MAX_BLOCKS)
        return RULGNN_EUNSUPPORTED;
    for (int v = 0; v < 2; ++v)
        if (s->d_model[v] > RULGNN_DVGT_MAX_D_MODEL || s->d_ff[v] > RULGNN_DVGT_MAX_D_FF) return RULGNN_EUNSUPPORTED;
    g->B = s->batch;
    g->N = s->num_nodes; g->L = s->time_length; g->H = s->num_heads; g->nb = s->num_blocks;
    for (int v = 0; v < 2; ++v) { g->d[v] = s->d_model[v]; g->ff[v] = s->d_ff[v]; }
    g->lam = s->lambda_param;
    dv_derive(g);
    // 32-bit dropout counters and int GEMM indices
    if (g->B * (int64_t)g->E * (2 * g->nb + 1) > ((int64_t)1 << 31) - 1) return RULGNN_EUNSUPPORTED;
    if (sizeof(float) * (size_t)dv_lds(*g, true).total > MAX_LDS_BYTES) return RULGNN_EUNSUPPORTED;       // (never within the limits above)
    return RULGNN_OK;
}

// ---- fold / unfold --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dv_fold_kernel(DvGeom g, DvOff o, const float* __restrict__ prm, float* __restrict__ fw) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < o.fw_total + g.E) fw[e] = dv_fold_elem(g, o, prm, e);
}

// one thread per flat gradient element in front of the head; R: the reduced partial row
__global__ __launch_bounds__(256) void dv_unfold_kernel(DvGeom g, DvOff o, const float* __restrict__ prm, const float* __restrict__ R,
                                                        float* __restrict__ grads) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < o.hw1) grads[e] = dv_unfold_elem(g, o, prm, R, e);
}

// ---- encoder kernels ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DV_BLK) void dv_encoder_fwd_kernel(DvGeom g, DvOff o, DvLds l, DvDrop drop, const float* __restrict__ x,
                                                                const float* __restrict__ prm, const float* __restrict__ fw, float* hin) {
    extern __shared__ float dv_smem[];
    const DvCtx c{(int)threadIdx.x, DV_BLK, dv_smem};
    const int64_t slot = g.B * (int64_t)g.E;
    for (int64_t b = blockIdx.x; b < g.B; b += gridDim.x)
        dv_sample_fwd(c, g, o, l, drop, b, x + b * g.N * g.L, prm, fw, hin + b * g.E, slot);
}

__global__ __launch_bounds__(DV_BLK) void dv_encoder_bwd_kernel(DvGeom g, DvOff o, DvLds l, DvDrop drop, const float* __restrict__ x,
                                                                const float* __restrict__ prm, const float* __restrict__ fw,
                                                                const float* __restrict__ hin, const float* __restrict__ denc, float* part) {
    extern __shared__ float dv_smem[];
    const DvCtx c{(int)threadIdx.x, DV_BLK, dv_smem};
    const int64_t slot = g.B * (int64_t)g.E;
    float* row = part + (int64_t)blockIdx.x * o.row_total;
    bool first = true;
    for (int64_t b = blockIdx.x; b < g.B; b += gridDim.x) {
        dv_sample_bwd(c, g, o, l, drop, b, x + b * g.N * g.L, prm, fw, hin + b * g.E, slot, denc + b * g.E, row, first);
        first = false;
    }
}

// ---- grouped forms: several runs of one shape, grid (x, runs) ---------------------------------------------------------------------------
// Run blockIdx.y's pointers and dropout keys come from a table that travels by value in the kernel arguments (blockIdx.y is
// wavefront-uniform: scalar loads from the argument segment, as in lstm_forward_group_kernel); the bodies are the single kernels'.
struct DvGroup {
    const float *x, *prm;           // the run's batch and parameters
    float *fw, *hin;                // its folded operands; its half-block inputs and encoder output
    const float* denc;
    float *part, *red, *grads;      // its partial rows, their sum, its gradient
    DvDrop drop;                    // keys of the run's own seed and step
};
struct DvGroupTable {
    DvGroup grp[STEP_MAX_GROUPS];
};

__global__ __launch_bounds__(256) void dv_fold_group_kernel(DvGeom g, DvOff o, DvGroupTable tab) {
    const DvGroup& r = tab.grp[blockIdx.y];
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < o.fw_total + g.E) r.fw[e] = dv_fold_elem(g, o, r.prm, e);
}

__global__ __launch_bounds__(256) void dv_unfold_group_kernel(DvGeom g, DvOff o, DvGroupTable tab) {
    const DvGroup& r = tab.grp[blockIdx.y];
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < o.hw1) r.grads[e] = dv_unfold_elem(g, o, r.prm, r.red, e);
}

__global__ __launch_bounds__(DV_BLK) void dv_encoder_fwd_group_kernel(DvGeom g, DvOff o, DvLds l, DvGroupTable tab) {
    extern __shared__ float dv_smem[];
    const DvGroup& r = tab.grp[blockIdx.y];
    const DvCtx c{(int)threadIdx.x, DV_BLK, dv_smem};
    const int64_t slot = g.B * (int64_t)g.E;
    for (int64_t b = blockIdx.x; b < g.B; b += gridDim.x)
        dv_sample_fwd(c, g, o, l, r.drop, b, r.x + b * g.N * g.L, r.prm, r.fw, r.hin + b * g.E, slot);
}

// (grid x = DvWs::rows, as the single kernel's: a run's partial rows hold the single call's sums)
__global__ __launch_bounds__(DV_BLK) void dv_encoder_bwd_group_kernel(DvGeom g, DvOff o, DvLds l, DvGroupTable tab) {
    extern __shared__ float dv_smem[];
    const DvGroup& r = tab.grp[blockIdx.y];
    const DvCtx c{(int)threadIdx.x, DV_BLK, dv_smem};
    const int64_t slot = g.B * (int64_t)g.E;
    float* row = r.part + (int64_t)blockIdx.x * o.row_total;
    bool first = true;
    for (int64_t b = blockIdx.x; b < g.B; b += gridDim.x) {
        dv_sample_bwd(c, g, o, l, r.drop, b, r.x + b * g.N * g.L, r.prm, r.fw, r.hin + b * g.E, slot, r.denc + b * g.E, row, first);
        first = false;
    }
}

// ---- head: Linear(E, 100) (on the shared SGEMM) - GELU - Linear(100, 1) --------------------------------------------------------------
constexpr int DV_HID = 100;

// h1 [B][100] = enc W1^T (no bias yet): pred, and with y also d loss / d pred and the squared error
__global__ __launch_bounds__(256) void dv_head_kernel(int64_t B, const float* __restrict__ h1, const float* __restrict__ b1,
                                                      const float* __restrict__ w2, const float* __restrict__ b2, const float* __restrict__ y,
                                                      float* __restrict__ pred, float* __restrict__ dpred, float* __restrict__ sqerr, float inv_gb) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    float a = b2[0];
    for (int j = 0; j < DV_HID; ++j) a = fmaf(dv_gelu(h1[b * DV_HID + j] + b1[j]), w2[j], a);
    pred[b] = a;
    if (y) {
        const float e = a - y[b];
        dpred[b] = 2.f * e * inv_gb;
        sqerr[b] = e * e * inv_gb;
    }
}

// dh [B][100] = dpred w2 gelu'(h1 + b1)
__global__ __launch_bounds__(256) void dv_head_dh_kernel(int64_t B, const float* __restrict__ h1, const float* __restrict__ b1,
                                                         const float* __restrict__ w2, const float* __restrict__ dpred, float* __restrict__ dh) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= B * DV_HID) return;
    const int64_t b = e / DV_HID;
    const int j = (int)(e - b * DV_HID);
    dh[e] = dpred[b] * w2[j] * dv_gelu_grad(h1[e] + b1[j]);
}

// db1[j] = sum_b dh[b][j], dw2[j] = sum_b dpred[b] gelu(h1[b][j] + b1[j]), db2 = sum_b dpred[b]: one workgroup, samples in order
__global__ __launch_bounds__(128) void dv_head_small_kernel(int64_t B, const float* __restrict__ h1, const float* __restrict__ b1,
                                                            const float* __restrict__ dpred, const float* __restrict__ dh, float* __restrict__ gb1,
                                                            float* __restrict__ gw2, float* __restrict__ gb2) {
    const int j = threadIdx.x;
    if (j > DV_HID) return;
    float a = 0.f, w = 0.f;
    if (j == DV_HID) {
        for (int64_t b = 0; b < B; ++b) a += dpred[b];
        gb2[0] = a;
        return;
    }
    const float bj = b1[j];
    for (int64_t b = 0; b < B; ++b) {
        a += dh[b * DV_HID + j];
        w = fmaf(dpred[b], dv_gelu(h1[b * DV_HID + j] + bj), w);
    }
    gb1[j] = a;
    gw2[j] = w;
}

struct DvWs {
    size_t fw, hin, h1, dh, denc, dpred, sqerr, part, red, total;
    int rows;
};

void dv_ws(const DvGeom& g, const DvOff& o, DvWs* w) {
    const size_t B = (size_t)(g.B > 0 ? g.B : 1);
    WsCarver c;
    w->fw = c.take<float>((size_t)o.fw_total + g.E);
    w->hin = c.take<float>((size_t)(2 * g.nb + 1) * B * g.E);
    w->h1 = c.take<float>(B * DV_HID);
    w->dh = c.take<float>(B * DV_HID);
    w->denc = c.take<float>(B * g.E);
    w->dpred = c.take<float>(B);
    w->sqerr = c.take<float>(B);
    // one partial row per workgroup of the backward kernel: a function of the shape alone (it fixes the summation order)
    int64_t rows = (int64_t)B < DV_MAX_ROWS ? (int64_t)B : DV_MAX_ROWS;
    const int64_t fit = DV_MAX_PART_FLOATS / o.row_total;
    rows = rows > fit ? fit : rows;
    w->rows = rows < 1 ? 1 : (int)rows;
    w->part = c.take<float>((size_t)w->rows * o.row_total);
    w->red = c.take<float>((size_t)o.row_total);
    w->total = c.total();
}

}  // namespace

int Dvgtformer::shape_status(const Shape* s) {
    DvGeom g;
    return dv_geometry(s, &g);
}

int64_t Dvgtformer::param_count(const Shape* s) {
    DvGeom g;
    if (dv_geometry(s, &g) != RULGNN_OK) return -1;
    return dv_offsets(g).total;
}

size_t Dvgtformer::workspace_bytes(const Shape* s) {
    DvGeom g;
    if (dv_geometry(s, &g) != RULGNN_OK) return 0;
    DvWs w;
    dv_ws(g, dv_offsets(g), &w);
    return w.total;
}

// float offsets into the workspace: 0 X behind the input stage and the positional encoding [B][L+1][N+1], 1 the encoder output (same shape)
int64_t Dvgtformer::tap_offset(const Shape* s, int which) {
    DvGeom g;
    if (dv_geometry(s, &g) != RULGNN_OK || which < 0 || which > 1) return -1;
    DvWs w;
    dv_ws(g, dv_offsets(g), &w);
    const size_t B = (size_t)(g.B > 0 ? g.B : 1);
    return (int64_t)(w.hin / sizeof(float)) + (which == 1 ? (int64_t)(2 * g.nb * B * g.E) : 0);
}

namespace {

// One run's view of a call: its workspace blocks and dropout keys.  The per-run stages below are what run() and run_group() enqueue
// around the fold, the encoder kernels and the unfold, which the one launches per run and the other once for all runs.
struct DvRun {
    const rulgnn_dvgtformer_args* a;
    float *fw, *hin, *enc, *h1, *dh, *denc, *dpred, *sqerr, *part, *red;
    DvDrop drop;
};

DvRun dv_run_of(const DvGeom& g, const DvWs& w, const rulgnn_dvgtformer_args* a) {
    DvRun r{};
    r.a = a;
    const DropoutConst dc = dropout_const(a->training ? a->dropout_p : 0.f);
    r.drop.thr = dc.thr;
    r.drop.scale = dc.scale;
    for (int b = 0; b < g.nb; ++b) r.drop.key[b] = dropout_layer_key(a->seed, a->step, b);
    r.drop.sample_offset = (uint32_t)a->sample_offset;
    const Workspace ws(a->workspace);
    r.fw = ws.at<float>(w.fw); r.hin = ws.at<float>(w.hin); r.h1 = ws.at<float>(w.h1); r.dh = ws.at<float>(w.dh);
    r.denc = ws.at<float>(w.denc); r.dpred = ws.at<float>(w.dpred); r.sqerr = ws.at<float>(w.sqerr); r.part = ws.at<float>(w.part);
    r.red = ws.at<float>(w.red);
    r.enc = r.hin + (size_t)2 * g.nb * g.B * g.E;
    return r;
}

// behind the encoder forward: the head's first layer on the shared SGEMM, then pred (with y also d pred and the loss terms)
int dv_head_fwd(const DvGeom& g, const DvOff& o, const DvRun& r, hipStream_t st) {
    const rulgnn_dvgtformer_args* a = r.a;
    const float* prm = a->params;
    const int B = (int)g.B, E = g.E;
    RULGNN_TRY(sgemm(r.enc, E, 1, prm + o.hw1, E, 1, r.h1, DV_HID, B, DV_HID, E, false, st));
    const float inv_gb = 1.0f / (float)(a->global_batch > 0 ? a->global_batch : g.B);
    return launch_checked(dv_head_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, g.B, (const float*)r.h1, prm + o.hb1, prm + o.hw2,
                          prm + o.hb2, a->y, a->pred, r.dpred, r.sqerr, inv_gb);
}

// in front of the encoder backward: the head's gradients and d enc
int dv_head_bwd(const DvGeom& g, const DvOff& o, const DvRun& r, hipStream_t st) {
    const rulgnn_dvgtformer_args* a = r.a;
    const float* prm = a->params;
    const int B = (int)g.B, E = g.E;
    const float* dpred = a->dpred ? a->dpred : r.dpred;
    float* gr = a->grads;
    RULGNN_TRY(launch_checked(dv_head_dh_kernel, dim3((unsigned)(((int64_t)B * DV_HID + 255) / 256)), dim3(256), 0, st, g.B, (const float*)r.h1,
                              prm + o.hb1, prm + o.hw2, dpred, r.dh));
    RULGNN_TRY(launch_checked(dv_head_small_kernel, dim3(1), dim3(128), 0, st, g.B, (const float*)r.h1, prm + o.hb1, dpred, (const float*)r.dh,
                              gr + o.hb1, gr + o.hw2, gr + o.hb2));
    // dW1 [100][E] = dh^T enc, d enc [B][E] = dh W1
    RULGNN_TRY(sgemm(r.dh, 1, DV_HID, r.enc, 1, E, gr + o.hw1, E, DV_HID, E, B, false, st));
    return sgemm(r.dh, DV_HID, 1, prm + o.hw1, 1, E, r.denc, E, B, E, DV_HID, false, st);
}

int dv_loss_sum(const DvGeom& g, const DvRun& r, hipStream_t st) {
    if (r.a->dpred || !r.a->loss) return RULGNN_OK;
    return block_sum((const float*)r.sqerr, g.B, r.a->loss, st);
}

}  // namespace

// mode bit 0: forward (pred; with y also d pred and the loss terms), bit 1: backward (gradients; d pred from args->dpred or from the
// forward of this call)
int Dvgtformer::run(const Shape* s, const Args* a, int mode, hipStream_t st) {
    DvGeom g;
    RULGNN_TRY(dv_geometry(s, &g));
    const DvOff o = dv_offsets(g);
    DvWs w;
    dv_ws(g, o, &w);
    if (!a->workspace || a->workspace_bytes < w.total) return RULGNN_EWORKSPACE;
    if (g.B == 0) {
        if ((mode & 2) && hipMemsetAsync(a->grads, 0, sizeof(float) * o.total, st) != hipSuccess) return RULGNN_EHIP;
        if ((mode & 2) && a->loss && hipMemsetAsync(a->loss, 0, sizeof(float), st) != hipSuccess) return RULGNN_EHIP;
        return RULGNN_OK;
    }
    const DvRun r = dv_run_of(g, w, a);
    const float* prm = a->params;
    const int E = g.E;
    // the folded operands follow the parameters of THIS call (an optimizer step lies between two calls)
    RULGNN_TRY(launch_checked(dv_fold_kernel, dim3((unsigned)((o.fw_total + E + 255) / 256)), dim3(256), 0, st, g, o, prm, r.fw));
    if (mode & 1) {
        const DvLds l = dv_lds(g, false);
        const size_t lds = sizeof(float) * (size_t)l.total;
        RULGNN_TRY(allow_dynamic_lds(dv_encoder_fwd_kernel, lds));
        const int grid = resident_rows(dv_encoder_fwd_kernel, DV_BLK, lds, g.B, 4096);
        RULGNN_TRY(launch_checked(dv_encoder_fwd_kernel, dim3((unsigned)grid), dim3(DV_BLK), lds, st, g, o, l, r.drop, a->x, prm, (const float*)r.fw,
                                  r.hin));
        RULGNN_TRY(dv_head_fwd(g, o, r, st));
    }
    if (mode & 2) {
        RULGNN_TRY(dv_head_bwd(g, o, r, st));
        const DvLds l = dv_lds(g, true);
        const size_t lds = sizeof(float) * (size_t)l.total;
        RULGNN_TRY(allow_dynamic_lds(dv_encoder_bwd_kernel, lds));
        RULGNN_TRY(launch_checked(dv_encoder_bwd_kernel, dim3((unsigned)w.rows), dim3(DV_BLK), lds, st, g, o, l, r.drop, a->x, prm, (const float*)r.fw,
                                  (const float*)r.hin, (const float*)r.denc, r.part));
        RULGNN_TRY(rows_sum(r.part, w.rows, o.row_total, o.row_total, r.red, st));
        RULGNN_TRY(launch_checked(dv_unfold_kernel, dim3((unsigned)((o.hw1 + 255) / 256)), dim3(256), 0, st, g, o, prm, (const float*)r.red, a->grads));
        RULGNN_TRY(dv_loss_sum(g, r, st));
    }
    return RULGNN_OK;
}

// The fused step (mode 3) of `n` runs of one shape: the fold, the encoder forward, the encoder backward and the unfold are one launch
// each for all runs, grid (x, n); the head, the row sum and the loss sum follow per run in run order, with run()'s arguments.  The
// forward's grid x is sized for the whole group (its samples are independent); the backward's stays DvWs::rows, which fixes each run's
// summation order.  The entry has checked every group.
int Dvgtformer::run_group(const Shape* s, const Args* groups, int n, hipStream_t st) {
    DvGeom g;
    RULGNN_TRY(dv_geometry(s, &g));
    if (n < 1 || n > STEP_MAX_GROUPS) return RULGNN_EINVAL;
    const DvOff o = dv_offsets(g);
    DvWs w;
    dv_ws(g, o, &w);
    for (int i = 0; i < n; ++i)
        if (!groups[i].workspace || groups[i].workspace_bytes < w.total) return RULGNN_EWORKSPACE;
    if (g.B == 0) {
        for (int i = 0; i < n; ++i) RULGNN_TRY(run(s, &groups[i], 3, st));
        return RULGNN_OK;
    }
    DvRun runs[STEP_MAX_GROUPS];
    DvGroupTable tab{};
    for (int i = 0; i < n; ++i) {
        const DvRun& r = runs[i] = dv_run_of(g, w, &groups[i]);
        tab.grp[i] = DvGroup{groups[i].x, groups[i].params, r.fw, r.hin, r.denc, r.part, r.red, groups[i].grads, r.drop};
    }
    const unsigned ny = (unsigned)n;
    RULGNN_TRY(launch_checked(dv_fold_group_kernel, dim3((unsigned)((o.fw_total + g.E + 255) / 256), ny), dim3(256), 0, st, g, o, tab));
    {
        const DvLds l = dv_lds(g, false);
        const size_t lds = sizeof(float) * (size_t)l.total;
        RULGNN_TRY(allow_dynamic_lds(dv_encoder_fwd_group_kernel, lds));
        const int resident = resident_rows(dv_encoder_fwd_group_kernel, DV_BLK, lds, g.B * n, (int64_t)4096 * n);
        RULGNN_TRY(launch_checked(dv_encoder_fwd_group_kernel, dim3((unsigned)((resident + n - 1) / n), ny), dim3(DV_BLK), lds, st, g, o, l, tab));
    }
    for (int i = 0; i < n; ++i) {
        RULGNN_TRY(dv_head_fwd(g, o, runs[i], st));
        RULGNN_TRY(dv_head_bwd(g, o, runs[i], st));
    }
    {
        const DvLds l = dv_lds(g, true);
        const size_t lds = sizeof(float) * (size_t)l.total;
        RULGNN_TRY(allow_dynamic_lds(dv_encoder_bwd_group_kernel, lds));
        RULGNN_TRY(launch_checked(dv_encoder_bwd_group_kernel, dim3((unsigned)w.rows, ny), dim3(DV_BLK), lds, st, g, o, l, tab));
    }
    for (int i = 0; i < n; ++i) RULGNN_TRY(rows_sum(runs[i].part, w.rows, o.row_total, o.row_total, runs[i].red, st));
    RULGNN_TRY(launch_checked(dv_unfold_group_kernel, dim3((unsigned)((o.hw1 + 255) / 256), ny), dim3(256), 0, st, g, o, tab));
    for (int i = 0; i < n; ++i) RULGNN_TRY(dv_loss_sum(g, runs[i], st));
    return RULGNN_OK;
}

}  // namespace rulgnn
