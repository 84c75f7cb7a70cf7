// STNet on gfx950 (a ChebNet user).
// Reference path replaced: STNet_model.forward -- models/STNet/Model.py:77-169 (ChebNet :7-40) -- and STNet.update,
// algorithms/algorithms.py:454-463 (loss = MSE(pred, y) + the auto-encoder's reconstruction MSE, backward, Adam).
//
//   x [bs, T * P] -> per (sample, patch) graph: |STFT| (n_fft = hop = nperseg, periodic Hann window, reflect-centred: torch.stft's
//   defaults) = N frequency nodes x f frames -> node weight = 1x1 convolution of (mean, max over the frames) -> nodes above 0.7 are
//   fully connected (A = m m^T) -> three ChebNets (K = 3, no non-linearity in between) -> auto-encoder (4 + 4 Linear layers; its
//   reconstruction error is part of the loss) -> LSTM over the T patches -> Linear.
//
// The adjacency is the outer product of a 0/1 mask, so A x is a masked node sum broadcast back (no [N, N] matrix is ever built); the
// Chebyshev terms [T0 | T1 | T2] of a layer are written side by side so that the layer is ONE matrix-core GEMM
// [rows, 3 C_in] x [3 C_in, C_out] (filters [3, C_in, C_out] are exactly that matrix) and its backward one GEMM + one split-K GEMM.
// The auto-encoder and the head are GEMMs over [bs * T] rows; the LSTM runs on the persistent kernels of bilstm.hip (one direction).
// The threshold has no gradient: the 1x1 convolution's parameters stay untouched (grad is None in the reference).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sgemm_mfma.hpp"
#include "families_host.hpp"
#include "stft_device.hpp"         // SB, the STFT magnitude
#include "seq_backend.hpp"         // the auto-encoder, the LSTM and the head (shared with gdagdl.hip and gatlstm.hip)

namespace rulgnn {

namespace {

constexpr int SN_MAX_CHEB = 4, SN_MAXSEG = 64, SN_MAXFR = 64, SN_MAXNODE = 33;
constexpr float SN_THRESHOLD = 0.7f;            // Model.py:106

struct SnGeom {
    int64_t B, G, R, BT;                        // samples, graphs = B * T, node rows = G * N, patch rows = B * T
    int T, P, nseg, N, f, ncheb, A, E;
    int C[SN_MAX_CHEB + 1];                     // channel widths: f, Cheb_layers...
    int D;                                      // N * C[last]: auto-encoder width
    int o_cw, o_cb, o_f[SN_MAX_CHEB], pcount;   // flat parameter offsets of the front end; the back end's are the plans'
    AutoEncoderPlan ae;                         // D -> A -> A -> A -> A and back
    LstmHeadPlan lh;                            // one LSTM A -> E over the T patches, Linear(E * T, 1)
    // workspace offsets (floats)
    int64_t w_fal[SN_MAX_CHEB];          // 16-byte aligned copies of the ChebNet filters (their flat-buffer offsets are odd: the big-tile GEMM needs aligned operands)
    int64_t w_mag, w_mask, w_terms[SN_MAX_CHEB], w_out[SN_MAX_CHEB], w_dterms, w_dc1, w_dc2, w_dhs, w_split, total;
};

int sn_geometry(const rulgnn_stnet_shape* s, SnGeom* g) {
    if (!s) return RULGNN_EINVAL;
    if (s->batch < 0 || s->num_patch < 1 || s->patch_size < 2 || s->nperseg < 2 || s->num_cheb < 1 || s->lstm_hidden_dim < 1 ||
        s->autoencoder_hidden_dim < 1)
        return RULGNN_EINVAL;
    if (s->num_cheb > SN_MAX_CHEB || s->nperseg > SN_MAXSEG || (s->nperseg & 1) || s->patch_size % s->nperseg != 0 ||
        s->patch_size <= s->nperseg / 2)
        return RULGNN_EUNSUPPORTED;              // reflect padding needs more than nperseg / 2 points; frames = 1 + P / nperseg
    g->B = s->batch; g->T = s->num_patch; g->P = s->patch_size; g->nseg = s->nperseg;
    g->N = s->nperseg / 2 + 1;
    g->f = 1 + s->patch_size / s->nperseg;
    if (g->f > SN_MAXFR || g->N > SN_MAXNODE) return RULGNN_EUNSUPPORTED;
    if (s->num_nodes != g->N || s->input_dim != g->f) return RULGNN_EINVAL;         // the reference's kwargs must describe the STFT's shape
    g->ncheb = s->num_cheb; g->A = s->autoencoder_hidden_dim; g->E = s->lstm_hidden_dim;
    g->C[0] = g->f;
    for (int i = 0; i < g->ncheb; ++i) {
        if (s->cheb_layers[i] < 1 || s->cheb_layers[i] > 4096) return RULGNN_EINVAL;
        g->C[i + 1] = s->cheb_layers[i];
    }
    if (g->E > 128 || g->A > 1024) return RULGNN_EUNSUPPORTED;
    g->G = g->B * g->T; g->R = g->G * g->N; g->BT = g->G;
    g->D = g->N * g->C[g->ncheb];
    if (g->R * 3 * 4096 > ((int64_t)1 << 40)) return RULGNN_EUNSUPPORTED;
    int o = 0;
    int64_t w = 0;
    SplitKScratch sp(1024);
    auto tk = [&](int n) { const int r = o; o += n; return r; };
    auto wk = [&](int64_t n) { const int64_t r = w; w += (n + 63) & ~(int64_t)63; return r; };
    g->o_cw = tk(2); g->o_cb = tk(1);
    for (int i = 0; i < g->ncheb; ++i) g->o_f[i] = tk(3 * g->C[i] * g->C[i + 1]);
    const int64_t R = g->R, BT = g->BT;
    g->w_mag = wk(R * g->f); g->w_mask = wk(R);
    int cmax = 0;
    for (int i = 0; i < g->ncheb; ++i) {
        g->w_terms[i] = wk(R * 3 * g->C[i]);
        g->w_out[i] = wk(R * g->C[i + 1]);
        if (g->C[i] > cmax) cmax = g->C[i];
        if (g->C[i + 1] > cmax) cmax = g->C[i + 1];
    }
    const int A = g->A, D = g->D;
    g->ae.BT = BT;
    for (int i = 0; i < 4; ++i) { g->ae.ein[i] = i ? A : D; g->ae.eout[i] = A; g->ae.din[i] = A; g->ae.dout[i] = i < 3 ? A : D; }
    autoencoder_layout(&g->ae, &o, &w, &sp);
    g->lh.B = g->B; g->lh.T = g->T; g->lh.nk = 1; g->lh.H[0] = A; g->lh.H[1] = g->E;
    RULGNN_TRY(lstm_head_layout(&g->lh, &o, &w, &sp));
    g->pcount = o;
    g->w_dterms = wk(R * 3 * cmax); g->w_dc1 = wk(R * cmax); g->w_dc2 = wk(R * cmax);
    g->w_dhs = wk(BT * g->E);
    for (int i = 0; i < g->ncheb; ++i) g->w_fal[i] = wk((int64_t)3 * g->C[i] * g->C[i + 1]);
    for (int i = 0; i < g->ncheb; ++i) sp.need(3 * g->C[i], g->C[i + 1], R);
    g->w_split = wk((int64_t)sp.floats());
    g->total = w;
    return RULGNN_OK;
}

// ---- STFT magnitude, node weights, mask: one workgroup per (sample, patch) --------------------------------------------------------
__global__ __launch_bounds__(SB) void sn_stft_kernel(SnGeom g, const float* __restrict__ x, const float* __restrict__ prm, float* __restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int P = g.P, ns = g.nseg, N = g.N, f = g.f, tid = threadIdx.x;
    const StftLds l = stft_carve(sm, P, ns);
    float* mg = l.end;                    // [N][f]
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
            float s = 0.f, mx = -INFINITY;
            for (int t = 0; t < f; ++t) { s += mg[tid * f + t]; mx = fmaxf(mx, mg[tid * f + t]); }
            const float nw = prm[g.o_cw] * (s / (float)f) + prm[g.o_cw + 1] * mx + prm[g.o_cb];
            ws[g.w_mask + gi * N + tid] = nw > SN_THRESHOLD ? 1.f : 0.f;
        }
        __syncthreads();
    }
}

// ---- Chebyshev terms of A = m m^T: [T0 | T1 | T2] per node row ---------------------------------------------------------------------
__global__ __launch_bounds__(SB) void sn_terms_kernel(SnGeom g, int C, const float* __restrict__ xin, const float* __restrict__ mask,
                                                      float* __restrict__ terms) {
    const int N = g.N;
    for (int64_t gi = blockIdx.x; gi < g.G; gi += gridDim.x) {
        const float* m = mask + gi * N;
        float cnt = 0.f;
        for (int n = 0; n < N; ++n) cnt += m[n];
        for (int c = threadIdx.x; c < C; c += SB) {
            float s = 0.f;
            for (int n = 0; n < N; ++n) s = fmaf(m[n], xin[(gi * N + n) * C + c], s);
            for (int n = 0; n < N; ++n) {
                const float xv = xin[(gi * N + n) * C + c];
                float* tr = terms + (gi * N + n) * 3 * C;
                const float t1 = m[n] * s;
                tr[c] = xv;
                tr[C + c] = t1;
                tr[2 * C + c] = 2.f * m[n] * (cnt * s) - xv;       // 2 A T1 - T0 with A T1 = m (m . T1) = m cnt s
            }
        }
    }
}

// dx = dT0 - dT2 + A (dT1 + 2 A dT2)      (A symmetric)
__global__ __launch_bounds__(SB) void sn_terms_bwd_kernel(SnGeom g, int C, const float* __restrict__ dterms, const float* __restrict__ mask,
                                                          float* __restrict__ dx) {
    const int N = g.N;
    for (int64_t gi = blockIdx.x; gi < g.G; gi += gridDim.x) {
        const float* m = mask + gi * N;
        for (int c = threadIdx.x; c < C; c += SB) {
            float a = 0.f;
            for (int n = 0; n < N; ++n) a = fmaf(m[n], dterms[(gi * N + n) * 3 * C + 2 * C + c], a);
            float b = 0.f;
            for (int n = 0; n < N; ++n) b = fmaf(m[n], dterms[(gi * N + n) * 3 * C + C + c] + 2.f * m[n] * a, b);
            for (int n = 0; n < N; ++n) {
                const float* dr = dterms + (gi * N + n) * 3 * C;
                dx[(gi * N + n) * C + c] = dr[c] - dr[2 * C + c] + m[n] * b;
            }
        }
    }
}

}  // namespace

// RULGNN_OK, or the code every entry returns for a refused shape: unsupported for anything sn_geometry refuses, a negative batch included.
int Stnet::shape_status(const Shape* s) {
    SnGeom g;
    return sn_geometry(s, &g) == RULGNN_OK ? RULGNN_OK : RULGNN_EUNSUPPORTED;
}

int64_t Stnet::param_count(const Shape* s) {
    SnGeom g;
    return sn_geometry(s, &g) == RULGNN_OK ? g.pcount : -1;
}

size_t Stnet::workspace_bytes(const Shape* s) {
    SnGeom g;
    return sn_geometry(s, &g) == RULGNN_OK ? (size_t)g.total * sizeof(float) : 0;
}

// mode bit 0: forward, bit 1: backward (after a forward with the same args / workspace)
int Stnet::run(const Shape* s, const Args* a, int mode, hipStream_t st) {
    SnGeom g;
    RULGNN_TRY(sn_geometry(s, &g));
    if (a->workspace_bytes < (size_t)g.total * sizeof(float)) return RULGNN_EWORKSPACE;
    if (g.B == 0) return RULGNN_OK;
    float* ws = static_cast<float*>(a->workspace);
    const float* prm = a->params;
    const int64_t gb = a->global_batch > 0 ? a->global_batch : g.B;
    const float inv_gb = 1.0f / (float)gb;
    const int nc = g.ncheb, R = (int)g.R;
    const float rscale = 1.0f / ((float)gb * (float)g.T * (float)g.D);          // 1 / elements of the global batch's Y_o
    const float* mask = ws + g.w_mask;
    float* split = ws + g.w_split;
    float* one = ws + g.lh.w_one;                 // [0] = 1 (backward), [1] the reconstruction term, [2] the MSE, [3] = 0
    const float* yo = ws + g.w_out[nc - 1];       // Y_o as [BT, D] rows
    const float* henc = ws + g.ae.w_enc[3];       // the encoder's output: the LSTM's input
    const unsigned ggrid = (unsigned)(g.G < 4096 ? g.G : 4096);
    // The filters as GEMM operands: the flat parameter buffer puts them behind three scalars, 12 bytes off a 16-byte boundary
    // (seq_backend.hpp: aligned_operand; 1 MB at the reference's widths, ~3 us a copy).
    const float* fop[SN_MAX_CHEB];
    for (int i = 0; i < nc; ++i) {
        const bool used_big = i > 0 || (mode & 1);                  // layer 0's transpose product is never formed (the input carries no gradient)
        fop[i] = used_big ? aligned_operand(prm + g.o_f[i], (size_t)3 * g.C[i] * g.C[i + 1], ws + g.w_fal[i], st) : prm + g.o_f[i];
        if (!fop[i]) return RULGNN_EHIP;
    }
    if (mode & 1) {
        const size_t lds = sizeof(float) * (stft_lds_floats(g.P, g.nseg) + (size_t)g.N * g.f);
        if (lds > 48 * 1024) return RULGNN_EUNSUPPORTED;
        RULGNN_TRY(fill_f32(one + 3, 1, 0.0f, st));
        RULGNN_TRY(launch_checked(sn_stft_kernel, dim3(ggrid), dim3(SB), lds, st, g, a->x, prm, ws));
        const float* cur = ws + g.w_mag;
        for (int i = 0; i < nc; ++i) {
            RULGNN_TRY(launch_checked(sn_terms_kernel, dim3(ggrid), dim3(SB), 0, st, g, g.C[i], cur, mask, ws + g.w_terms[i]));
            RULGNN_TRY(sgemm(ws + g.w_terms[i], 3 * g.C[i], 1, fop[i], 1, g.C[i + 1], ws + g.w_out[i], g.C[i + 1], R, g.C[i + 1], 3 * g.C[i],
                        false, st));
            cur = ws + g.w_out[i];
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
        RULGNN_TRY(fill_f32(gr + g.o_cw, 3, 0.0f, st));          // the 1x1 convolution has no gradient
        float* const dseq[2] = {ws + g.w_dhs, ws + g.ae.w_dH};
        RULGNN_TRY(lstm_head_backward(g.lh, henc, prm, ws, dpred, gr, dseq, split, st));
        RULGNN_TRY(autoencoder_backward(g.ae, yo, prm, ws, gr, one, a->recon_weight, split, st));
        const float* dcur = ws + g.ae.w_dD1;          // d Y_o: [R, C_last]
        float* dc[2] = {ws + g.w_dc1, ws + g.w_dc2};
        for (int i = nc - 1; i >= 0; --i) {
            const int Ci = g.C[i], Co = g.C[i + 1];
            RULGNN_TRY(sgemm_splitk(ws + g.w_terms[i], 1, 3 * Ci, dcur, 1, Co, gr + g.o_f[i], Co, 3 * Ci, Co, R, false, split, st));
            if (i == 0) break;                        // the input carries no gradient
            RULGNN_TRY(sgemm(dcur, Co, 1, fop[i], Co, 1, ws + g.w_dterms, 3 * Ci, R, 3 * Ci, Co, false, st));
            float* dn = dc[i & 1];
            RULGNN_TRY(launch_checked(sn_terms_bwd_kernel, dim3(ggrid), dim3(SB), 0, st, g, Ci, (const float*)(ws + g.w_dterms), mask, dn));
            dcur = dn;
        }
    }
    return RULGNN_OK;
}

}  // namespace rulgnn
