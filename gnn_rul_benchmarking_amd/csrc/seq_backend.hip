// The auto-encoder / LSTM / head back end of STNet, GDAGDL, GAT_LSTM and STFA (seq_backend.hpp): its small kernels, compiled once, and the host
// chain around them.  Every sum has a fixed order; the grids that write per-workgroup partials (rblocks, min(B, 1024)) are part of the bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "seq_backend.hpp"

namespace rulgnn {

namespace {

constexpr int SQB = 256;

__global__ void sq_bias_act_kernel(float* __restrict__ z, const float* __restrict__ bias, int64_t rows, int C, int relu) {
    const int64_t n = rows * C;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float v = z[i] + bias[i % C];
        z[i] = relu ? fmaxf(v, 0.f) : v;
    }
}

__global__ void sq_relu_bwd_kernel(float* __restrict__ d, const float* __restrict__ h, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        d[i] = h[i] > 0.f ? d[i] : 0.f;
}

// a *= w[0], b *= w[0]: the reconstruction term's gradients under a weight other than 1 (autograd path)
__global__ void sq_scale2_kernel(float* __restrict__ a, float* __restrict__ b, int64_t n, const float* __restrict__ w) {
    const float s = w[0];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        a[i] *= s;
        b[i] *= s;
    }
}
__global__ void sq_add_kernel(float* __restrict__ a, const float* __restrict__ b, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) a[i] += b[i];
}

// reconstruction error: partial sums of (Yo - Yp)^2 (one per workgroup, fixed assignment), d Yp = -2 s (Yo - Yp), d Yo = +2 s (Yo - Yp)
__global__ __launch_bounds__(SQB) void sq_recon_kernel(const float* __restrict__ yo, const float* __restrict__ yp, int64_t n, float scale,
                                                       float* __restrict__ dyp, float* __restrict__ dyo, float* __restrict__ part) {
    __shared__ float red[SQB];
    float a = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * SQB + threadIdx.x; i < n; i += (int64_t)gridDim.x * SQB) {
        const float d = yo[i] - yp[i];
        a = fmaf(d, d, a);
        if (dyp) { dyp[i] = -2.f * scale * d; dyo[i] = 2.f * scale * d; }
    }
    red[threadIdx.x] = a;
    __syncthreads();
    for (int m = SQB / 2; m > 0; m >>= 1) {
        if ((int)threadIdx.x < m) red[threadIdx.x] += red[threadIdx.x + m];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0] * scale;
}

// head: pred = hseq_flat . w + b; squared error and d loss / d pred
struct SqHead {
    int64_t B;
    int n;                                       // values per sample the head reads: H * T, or H (the last step's) under last_step
    int64_t stride;                              // floats between two samples' first value (hseq points at sample 0's)
    const float *hseq, *w, *b, *y;               // y may be null: prediction alone
    float *pred, *sq, *dpred;
    float inv_gb;
};
__global__ __launch_bounds__(SQB) void sq_head_kernel(SqHead g) {
    __shared__ float red[SQB];
    const int n = g.n;
    for (int64_t b = blockIdx.x; b < g.B; b += gridDim.x) {
        float a = 0.f;
        for (int i = threadIdx.x; i < n; i += SQB) a = fmaf(g.hseq[b * g.stride + i], g.w[i], a);
        red[threadIdx.x] = a;
        __syncthreads();
        for (int m = SQB / 2; m > 0; m >>= 1) {
            if ((int)threadIdx.x < m) red[threadIdx.x] += red[threadIdx.x + m];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            const float pr = red[0] + g.b[0];
            g.pred[b] = pr;
            if (g.y) {
                const float d = pr - g.y[b];
                g.sq[b] = d * d * g.inv_gb;
                g.dpred[b] = 2.f * d * g.inv_gb;
            }
        }
        __syncthreads();
    }
}

// d hseq[b][i] = dpred[b] w[i]
__global__ void sq_head_bwd_kernel(int64_t B, int n, const float* __restrict__ dpred, const float* __restrict__ w, float* __restrict__ dhs) {
    const int64_t tot = B * n;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < tot; i += (int64_t)gridDim.x * blockDim.x)
        dhs[i] = dpred[i / n] * w[i % n];
}

// last-step head: d hseq[b][t][e] = dpred[b] w[e] at t = T - 1, 0 before
__global__ void sq_head_last_bwd_kernel(int64_t B, int T, int E, const float* __restrict__ dpred, const float* __restrict__ w, float* __restrict__ dhs) {
    const int64_t n = (int64_t)T * E, tot = B * n;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < tot; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i % n;
        dhs[i] = r >= n - E ? dpred[i / n] * w[r - (n - E)] : 0.f;
    }
}

__global__ void sq_sum_pair_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) out[0] = a[0] + b[0];
}

inline dim3 sq_grid(int64_t n) {
    int64_t b = (n + SQB - 1) / SQB;
    return dim3((unsigned)(b < 1 ? 1 : (b > 4096 ? 4096 : b)));
}

int64_t take(int64_t* w, int64_t n) { const int64_t r = *w; *w += (n + 63) & ~(int64_t)63; return r; }
int take(int* o, int n) { const int r = *o; *o += n; return r; }

void lstm_layer_args(const LstmHeadPlan& p, int k, const float* x, const float* prm, float* ws, rulgnn_bilstm_shape* ls, rulgnn_bilstm_args* la,
                     float* grads = nullptr, const float* dout = nullptr, float* dx = nullptr) {
    lstm_uni_args(ls, la, p.T, p.B, p.H[k], p.H[k + 1], k > 0 ? ws + p.w_hseq[k - 1] : x, ws + p.w_hseq[k], ws + p.w_lstm[k], prm, p.o_lstm[k],
                  grads, dout, dx);
}

}  // namespace

int gemm_rows(const float* A, int64_t sAm, int64_t sAk, const float* B, int64_t sBn, int64_t sBk, float* C, int64_t ldc, int M, int N, int K,
              float* split, hipStream_t st) {
    if (K >= 512 && (int64_t)((M + 63) / 64) * ((N + 63) / 64) < 128) return sgemm_splitk(A, sAm, sAk, B, sBn, sBk, C, ldc, M, N, K, false, split, st);
    return sgemm(A, sAm, sAk, B, sBn, sBk, C, ldc, M, N, K, false, st);
}

const float* aligned_operand(const float* p, size_t count, float* slot, hipStream_t st) {
    if (!(reinterpret_cast<uintptr_t>(p) & 15)) return p;
    return hipMemcpyAsync(slot, p, sizeof(float) * count, hipMemcpyDeviceToDevice, st) == hipSuccess ? slot : nullptr;
}

int dense_backward(const float* d, const float* h, const float* W, const float* one, float* gw, float* gb, DenseData data, float* dn, int rows,
                   int out, int in, float* split, hipStream_t st) {
    RULGNN_TRY(sgemm_splitk(d, 1, out, h, 1, in, gw, in, out, in, rows, false, split, st));
    RULGNN_TRY(sgemm_splitk(one, 0, 0, d, 1, out, gb, out, 1, out, rows, false, split, st));
    if (data == DENSE_ROWS) return gemm_rows(d, out, 1, W, 1, in, dn, in, rows, in, out, split, st);
    if (data == DENSE_PLAIN) return sgemm(d, out, 1, W, 1, in, dn, in, rows, in, out, false, st);
    return RULGNN_OK;
}

int sum_pair(const float* a, const float* b, float* out, hipStream_t st) { return launch_checked(sq_sum_pair_kernel, dim3(1), dim3(1), 0, st, a, b, out); }

void lstm_uni_args(rulgnn_bilstm_shape* ls, rulgnn_bilstm_args* la, int T, int64_t B, int I, int E, const float* x, float* out, float* lstm_ws,
                   const float* prm, const int o[4], float* grads, const float* dout, float* dx) {
    *ls = rulgnn_bilstm_shape{T, (int32_t)B, I, E};
    *la = rulgnn_bilstm_args{};
    la->x = x;
    la->out = out;
    la->dout = dout;
    la->dx = dx;
    for (int dir = 0; dir < 2; ++dir) {
        la->w_ih[dir] = prm + o[0]; la->w_hh[dir] = prm + o[1]; la->b_ih[dir] = prm + o[2]; la->b_hh[dir] = prm + o[3];
        if (grads) { la->dw_ih[dir] = grads + o[0]; la->dw_hh[dir] = grads + o[1]; la->db_ih[dir] = grads + o[2]; la->db_hh[dir] = grads + o[3]; }
    }
    la->workspace = lstm_ws;
    la->workspace_bytes = bilstm_workspace_bytes(ls);
}

int lstm_head_layout(LstmHeadPlan* p, int* o, int64_t* w, SplitKScratch* sp) {
    const int E = p->H[p->nk];
    for (int k = 0; k < p->nk; ++k) {
        const int I = p->H[k], Ek = p->H[k + 1];
        p->o_lstm[k][0] = take(o, 4 * Ek * I); p->o_lstm[k][1] = take(o, 4 * Ek * Ek); p->o_lstm[k][2] = take(o, 4 * Ek); p->o_lstm[k][3] = take(o, 4 * Ek);
    }
    const int nhead = p->last_step ? E : E * p->T;
    p->o_lw = take(o, nhead); p->o_lb = take(o, 1);
    for (int k = 0; k < p->nk; ++k) p->w_hseq[k] = take(w, p->B * p->T * p->H[k + 1]);
    p->w_dpred = take(w, p->B); p->w_sq = take(w, p->B);
    p->w_one = take(w, 64);
    sp->need(1, nhead, p->B);
    sp->need(1, 1, p->B);
    for (int k = 0; k < p->nk; ++k) {
        rulgnn_bilstm_shape ls{p->T, (int32_t)(p->B > 0 ? p->B : 1), p->H[k], p->H[k + 1]};
        const size_t lb = bilstm_workspace_bytes(&ls);
        if (lb == 0) return RULGNN_EUNSUPPORTED;
        p->w_lstm[k] = take(w, (int64_t)(lb / sizeof(float)) + 64);
    }
    return RULGNN_OK;
}

int lstm_head_forward(const LstmHeadPlan& p, const float* x, const float* prm, float* ws, const float* y, float* pred, float inv_gb, hipStream_t st) {
    for (int k = 0; k < p.nk; ++k) {
        rulgnn_bilstm_shape ls;
        rulgnn_bilstm_args la;
        lstm_layer_args(p, k, x, prm, ws, &ls, &la);
        RULGNN_TRY(bilstm_forward(&ls, &la, st, 1));
    }
    const int E = p.H[p.nk], ET = E * p.T;
    const float* hseq = ws + p.w_hseq[p.nk - 1];
    const SqHead h{p.B, p.last_step ? E : ET, ET, p.last_step ? hseq + (ET - E) : hseq, prm + p.o_lw, prm + p.o_lb, y, pred, ws + p.w_sq, ws + p.w_dpred,
                   inv_gb};
    return launch_checked(sq_head_kernel, dim3((unsigned)(p.B < 1024 ? p.B : 1024)), dim3(SQB), 0, st, h);
}

int lstm_head_backward(const LstmHeadPlan& p, const float* x, const float* prm, float* ws, const float* dpred, float* grads, float* const dbuf[2],
                       float* split, hipStream_t st) {
    const int E = p.H[p.nk], ET = E * p.T;
    // the weight gradient over B rows of the head's width: the whole sequence, or the last step's E values (rows ET apart)
    const int nh = p.last_step ? E : ET;
    RULGNN_TRY(sgemm_splitk(dpred, 0, 1, ws + p.w_hseq[p.nk - 1] + (ET - nh), 1, ET, grads + p.o_lw, nh, 1, nh, (int)p.B, false, split, st));
    RULGNN_TRY(sgemm_splitk(dpred, 0, 1, ws + p.w_one, 0, 0, grads + p.o_lb, 1, 1, 1, (int)p.B, false, split, st));
    int cur = 0;
    if (p.last_step)
        RULGNN_TRY(launch_checked(sq_head_last_bwd_kernel, sq_grid(p.B * ET), dim3(SQB), 0, st, p.B, p.T, E, dpred, prm + p.o_lw, dbuf[cur]));
    else
        RULGNN_TRY(launch_checked(sq_head_bwd_kernel, sq_grid(p.B * ET), dim3(SQB), 0, st, p.B, ET, dpred, prm + p.o_lw, dbuf[cur]));
    // layer k's dx is layer k - 1's dout
    for (int k = p.nk - 1; k >= 0; --k, cur ^= 1) {
        rulgnn_bilstm_shape ls;
        rulgnn_bilstm_args la;
        lstm_layer_args(p, k, x, prm, ws, &ls, &la, grads, dbuf[cur], dbuf[cur ^ 1]);
        RULGNN_TRY(bilstm_backward(&ls, &la, st, 1));
    }
    return RULGNN_OK;
}

void autoencoder_layout(AutoEncoderPlan* p, int* o, int64_t* w, SplitKScratch* sp) {
    const int64_t BT = p->BT;
    const int D = p->ein[0];
    int amax = 0;                                // the widest data gradient below [BT, D]: the ping-pong pair holds them all
    for (int i = 0; i < 4; ++i) {
        p->o_enc_w[i] = take(o, p->eout[i] * p->ein[i]); p->o_enc_b[i] = take(o, p->eout[i]);
        if (p->din[i] > amax) amax = p->din[i];
        if (i > 0 && p->ein[i] > amax) amax = p->ein[i];
    }
    for (int i = 0; i < 4; ++i) { p->o_dec_w[i] = take(o, p->dout[i] * p->din[i]); p->o_dec_b[i] = take(o, p->dout[i]); }
    for (int i = 0; i < 4; ++i) p->w_enc[i] = take(w, BT * p->eout[i]);
    for (int i = 0; i < 4; ++i) p->w_dec[i] = take(w, BT * p->dout[i]);
    p->rblocks = 1024;
    p->w_rsq = take(w, p->rblocks);
    p->w_dD1 = take(w, BT * D); p->w_dD2 = take(w, BT * D);
    p->w_dA1 = take(w, BT * amax); p->w_dA2 = take(w, BT * amax);
    p->w_dH = take(w, BT * p->eout[3]);
    for (int i = 0; i < 4; ++i) {
        sp->need(p->eout[i], p->ein[i], BT); sp->need(1, p->eout[i], BT); sp->need(p->dout[i], p->din[i], BT); sp->need(1, p->dout[i], BT);
        sp->need((int)BT, p->eout[i], p->ein[i]); sp->need((int)BT, p->din[i], p->dout[i]);      // activations over a long reduction: gemm_rows
    }
}

int autoencoder_forward(const AutoEncoderPlan& p, const float* yo, const float* prm, float* ws, float rscale, float* recon_sum, float* split,
                        hipStream_t st) {
    const int BT = (int)p.BT;
    const float* h = yo;                          // [BT, D] rows
    for (int i = 0; i < 4; ++i) {
        RULGNN_TRY(gemm_rows(h, p.ein[i], 1, prm + p.o_enc_w[i], p.ein[i], 1, ws + p.w_enc[i], p.eout[i], BT, p.eout[i], p.ein[i], split, st));
        RULGNN_TRY(launch_checked(sq_bias_act_kernel, sq_grid(p.BT * p.eout[i]), dim3(SQB), 0, st, ws + p.w_enc[i], prm + p.o_enc_b[i], p.BT, p.eout[i],
                                  i < 3 ? 1 : 0));
        h = ws + p.w_enc[i];
    }
    for (int i = 0; i < 4; ++i) {
        RULGNN_TRY(sgemm(h, p.din[i], 1, prm + p.o_dec_w[i], p.din[i], 1, ws + p.w_dec[i], p.dout[i], BT, p.dout[i], p.din[i], false, st));
        RULGNN_TRY(launch_checked(sq_bias_act_kernel, sq_grid(p.BT * p.dout[i]), dim3(SQB), 0, st, ws + p.w_dec[i], prm + p.o_dec_b[i], p.BT, p.dout[i],
                                  i < 3 ? 1 : 0));
        h = ws + p.w_dec[i];
    }
    // reconstruction error (and, for a backward that may follow, its gradients w.r.t. both of its arguments)
    RULGNN_TRY(launch_checked(sq_recon_kernel, dim3(p.rblocks), dim3(SQB), 0, st, yo, (const float*)(ws + p.w_dec[3]), p.BT * p.ein[0], rscale,
                              ws + p.w_dD1, ws + p.w_dD2, ws + p.w_rsq));
    return block_sum(ws + p.w_rsq, (int64_t)p.rblocks, recon_sum, st);
}

int autoencoder_backward(const AutoEncoderPlan& p, const float* yo, const float* prm, float* ws, float* grads, const float* one,
                         const float* recon_weight, float* split, hipStream_t st) {
    const int BT = (int)p.BT;
    const int64_t nD = p.BT * p.ein[0];
    // decoder, from d Yp = w_dD1 (the reconstruction scale of a data-parallel shard is the global one: recon is in the loss with weight 1)
    if (recon_weight) RULGNN_TRY(launch_checked(sq_scale2_kernel, sq_grid(nD), dim3(SQB), 0, st, ws + p.w_dD1, ws + p.w_dD2, nD, recon_weight));
    float* d = ws + p.w_dD1;
    float* dA[2] = {ws + p.w_dA1, ws + p.w_dA2};
    for (int i = 3; i >= 0; --i) {
        const float* hin = i > 0 ? ws + p.w_dec[i - 1] : ws + p.w_enc[3];
        if (i < 3)
            RULGNN_TRY(launch_checked(sq_relu_bwd_kernel, sq_grid(p.BT * p.dout[i]), dim3(SQB), 0, st, d, (const float*)(ws + p.w_dec[i]), p.BT * p.dout[i]));
        float* dn = dA[i & 1];
        RULGNN_TRY(dense_backward(d, hin, prm + p.o_dec_w[i], one, grads + p.o_dec_w[i], grads + p.o_dec_b[i], DENSE_ROWS, dn, BT, p.dout[i], p.din[i],
                                  split, st));
        d = dn;
    }
    // d H = decoder path + LSTM path
    RULGNN_TRY(launch_checked(sq_add_kernel, sq_grid(p.BT * p.eout[3]), dim3(SQB), 0, st, d, (const float*)(ws + p.w_dH), p.BT * p.eout[3]));
    for (int i = 3; i >= 0; --i) {
        const float* hin = i > 0 ? ws + p.w_enc[i - 1] : yo;
        if (i < 3)
            RULGNN_TRY(launch_checked(sq_relu_bwd_kernel, sq_grid(p.BT * p.eout[i]), dim3(SQB), 0, st, d, (const float*)(ws + p.w_enc[i]), p.BT * p.eout[i]));
        float* dn = i > 0 ? (d == dA[0] ? dA[1] : dA[0]) : ws + p.w_dD1;          // the last one is [BT, D]: d Y_o through the encoder
        RULGNN_TRY(dense_backward(d, hin, prm + p.o_enc_w[i], one, grads + p.o_enc_w[i], grads + p.o_enc_b[i], DENSE_PLAIN, dn, BT, p.eout[i], p.ein[i],
                                  split, st));
        d = dn;
    }
    // d Y_o = encoder path + the reconstruction term's own gradient
    return launch_checked(sq_add_kernel, sq_grid(nD), dim3(SQB), 0, st, d, (const float*)(ws + p.w_dD2), nD);
}

}  // namespace rulgnn
