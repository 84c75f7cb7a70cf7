// HierCorrPool on gfx950.
// Reference path replaced: HierCorrPool_model.forward -- models/HierCorrPool/Model.py:6-52 (encoder Model_Base.py:30-64, graph
// construction :11-25, cluster assignment :102-117, pooling block :122-145, MPNN_mk :66-96) -- and HierCorrPool.update,
// algorithms/algorithms.py:79-104 (plain MSE + Adam).
//
//   x [bs, N, P p] -> in [bs, C0 = N p, P] -> 3 x (Conv1d k 8 pad 4 -> BatchNorm1d -> ReLU -> MaxPool1d(2, 2, pad 1)) (dropout behind
//   block 1) -> F [bs, L', C3] read flat per sample as X [N, d], X[n][k e + q] = F[(k N + n) e + q] -> G = X X^T,
//   A = softmax_row(leaky(G) off the diagonal) + I -> Z = sigmoid((A X) Wd^T + bd), S = softmax over the nodes of ([A | Z] Wm^T + bm)
//   -> X' = S^T X, A' = S^T A S -> H = leaky((A' X') Wt^T + bt) -> leaky(fc_1(leaky(fc_0(H.flat)))).
//
// Encoder.  Every activation is kept channel-last and time-padded, [b][L + 8][C] with four zero rows on each
// side, so a convolution's im2col operand is the overlapping-row view of that buffer (row stride C, 8 C contiguous k) and the three
// products of a block are calls into the shared matrix-core SGEMM: forward z = view . Wp^T with Wp [out][tap][c]; d input = the same
// view of d z (whose seven rows between two samples are zero, which is the transposed convolution's padding) against Wt [c][7 - tap][out];
// d Wp = d z^T . view.  All three are fixed-slice split-K products (sgemm_splitk): at the reference's batch an output is a few dozen tiles
// over k = 8 C.  The 7 of every L + 8 output rows that straddle two samples are computed and ignored.  BatchNorm sums are per-slice fp64 partials summed in one fixed order (no atomics), the coefficients come from bn_cells.hpp;
// BN -> ReLU -> max-pool -> dropout is one pass that writes the next block's padded input, and the backward recomputes the arg max from
// the saved convolution output.
//
// Graph stage: one workgroup per sample, everything between X and A' X' in LDS (hcp_graph_fwd / hcp_graph_bwd below); products with a
// d-long k run on v_mfma_f32_16x16x4_f32 (hc_mm).  No floating-point atomics anywhere: two runs give the same bits.
//
// HierCorrPool_bearing (models/HierCorrPool_bearing/Model.py:6-67; HierCorrPool_bearing.update, algorithms/algorithms.py:633-658) is the
// same chain behind an STFT front end: x is the raw window [bs, P p], the nodes are the N = nperseg / 2 + 1
// frequency bins of a patch's spectrogram and a node's features its f = 1 + p / nperseg frames, so block 1 reads C0 = N f channels.
// hcpb_stft_input_kernel below takes hc_pack_input_kernel's place and nothing else changes: one geometry function (hc_geometry with a
// front-end description, HcFront) and one host chain (hc_run) serve both families.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bn_cells.hpp"
#include "sgemm_mfma.hpp"
#include "families_host.hpp"       // (stgcn_host.hpp: dropout_layer_key; stgcn_device.hpp: lowbias32)
#include "stft_device.hpp"         // the per-patch STFT magnitude (HierCorrPool_bearing's front end)

namespace rulgnn {

namespace {

constexpr int HC_GB = 256, HC_WAVES = HC_GB / 64;
constexpr int HC_TAPS = 8, HC_PAD = 4;
constexpr int HC_MAXN = 32, HC_MAXM = 16, HC_MAXD = 512, HC_MAXP = 64, HC_MAXC3 = 1024;
constexpr int HCPB_GRID = 2048;               // workgroups of the STFT packing kernel: eight of 256 threads on each of 256 compute units
constexpr int HC_SLICES = 64;                 // row slices of a BatchNorm reduction (fixed: it fixes the summation order)
constexpr float HC_SLOPE = 0.01f;             // F.leaky_relu's default
constexpr float HC_EPS = 1e-5f, HC_MOMENTUM = 0.1f;

struct HcBlock {
    int Cin, Cout, Lin, Lc, Lp;               // the convolution reads Lin steps and writes Lc = Lin + 1; the pool leaves Lp
    int o_w, o_g, o_b, o_bn;                  // parameter offsets (conv weight, BN weight, BN bias); bn_state offset (mean; var at + Cout)
    int64_t R;                                // rows of the padded input: B (Lin + 8)
    // workspace, float offsets
    int64_t w_in, w_z, w_dz, w_din, w_wp, w_wt, w_dwp, w_coef, w_bcoef, w_part;
};

// What stands in front of block 1, and the limits that go with it.  HierCorrPool: the window [N][P p] itself, w = p values per node and
// step.  HierCorrPool_bearing: |STFT| of the raw window [P p] at nperseg ns, w = f frames per frequency bin and patch.
struct HcFront {
    int ns;                                   // nperseg; 0: no STFT
    int w, C0;                                // per-node width (p or f), block 1's channels N w
    int max_nodes, max_patch, max_patch_size, max_d;
};

struct HcGeom {
    int64_t B;
    int p, P, h, e, N, K, M, d, d3, e3, Lq;   // Lq = L'
    int ns, w;                                // the front end: nperseg (0: none) and the per-node width, C0 = N w = blk[0].Cin
    HcBlock blk[3];
    int o_tw, o_tb, o_wd, o_bd, o_wm, o_bm, o_f0w, o_f0b, o_f1w, o_f1b, pcount, bncount;
    int CW;                                   // floats of one sample's [d Wd | d bd | d Wm] contribution
    int64_t w_enc, w_xp, w_ap, w_axp, w_H, w_pre0, w_pre1, w_sq, w_dpred, w_prod, w_dpre0, w_dH, w_dq, w_dxp, w_denc, w_contrib, w_split;
    size_t split_floats, total_bytes, lds_fwd, lds_bwd;
};

// LDS of the graph stage, float offsets, stated once for the kernels and the launcher.  X [N][d + 1] | AX [max(N, M)][d + 1] (forward:
// then X'; backward: then d(AX)) | A [N][N + 1] | Z, S [N][M + 1] | SA [M][N + 1] | A' [M][M + 1]; the backward adds G, dA [N][N + 1],
// dS, AS, AtS, SdA, dZp [N][M + 1], dA' [M][M + 1] and 16 column sums.
struct HcGraphLds {
    int X, AX, A, Z, S, SA, Ap, G, dA, dS, AS, AtS, SdA, dZp, dAp, cs, total;
};
__host__ __device__ inline HcGraphLds hc_graph_lds(int N, int M, int d, bool bwd) {
    HcGraphLds l;
    const int LD = d + 1, NL = N + 1, ML = M + 1, rows = N > M ? N : M;
    int o = 0;
    l.X = o; o += N * LD;
    l.AX = o; o += rows * LD;
    l.A = o; o += N * NL;
    l.Z = o; o += N * ML;
    l.S = o; o += N * ML;
    l.SA = o; o += M * NL;
    l.Ap = o; o += M * ML;
    l.G = l.dA = l.dS = l.AS = l.AtS = l.SdA = l.dZp = l.dAp = l.cs = o;
    if (bwd) {
        l.G = o; o += N * NL;
        l.dA = o; o += N * NL;
        l.dS = o; o += N * ML;
        l.AS = o; o += N * ML;
        l.AtS = o; o += N * ML;
        l.SdA = o; o += N * ML;
        l.dZp = o; o += N * ML;
        l.dAp = o; o += M * ML;
        l.cs = o; o += HC_MAXM;
    }
    l.total = o;
    return l;
}

int hc_geometry(const rulgnn_hiercorrpool_shape* s, const HcFront& fe, HcGeom* g) {
    if (s->batch < 0 || s->patch_size < 0 || s->num_patch < 0 || s->hidden_dim < 0 || s->embedding_dim < 0 || s->num_nodes < 0 ||
        s->encoder_conv_kernel < 0 || s->num_nodes_out < 0)
        return RULGNN_EINVAL;
    if (s->num_nodes < 2 || s->num_nodes > fe.max_nodes || s->num_nodes_out < 1 || s->num_nodes_out > HC_MAXM || s->num_patch < 2 ||
        s->num_patch > fe.max_patch || s->patch_size < 1 || s->patch_size > fe.max_patch_size || s->hidden_dim < 1 || s->embedding_dim < 1 ||
        s->encoder_conv_kernel < 1)
        return RULGNN_EUNSUPPORTED;
    g->ns = fe.ns; g->w = fe.w;
    g->B = s->batch; g->p = s->patch_size; g->P = s->num_patch; g->h = s->hidden_dim; g->e = s->embedding_dim; g->N = s->num_nodes;
    g->K = s->encoder_conv_kernel; g->M = s->num_nodes_out;
    const int64_t d64 = (int64_t)g->K * g->e, c364 = (int64_t)4 * g->h * g->N;
    if (d64 > fe.max_d || c364 > HC_MAXC3) return RULGNN_EUNSUPPORTED;
    g->d = (int)d64; g->d3 = 3 * g->d; g->e3 = 3 * g->e;
    const int N = g->N, M = g->M, d = g->d;
    const int64_t B = g->B;
    int C = fe.C0, L = g->P, o = 0, obn = 0;
    for (int l = 0; l < 3; ++l) {
        HcBlock& k = g->blk[l];
        k.Cin = C; k.Cout = (g->h * N) << l; k.Lin = L; k.Lc = L + 1; k.Lp = k.Lc / 2 + 1;
        k.o_w = o; o += k.Cout * k.Cin * HC_TAPS;
        k.o_g = o; o += k.Cout;
        k.o_b = o; o += k.Cout;
        k.o_bn = obn; obn += 2 * k.Cout;
        k.R = B * (k.Lin + 2 * HC_PAD);
        if ((k.R + 7) * (int64_t)(k.Cout > k.Cin ? k.Cout : k.Cin) >= (int64_t)1 << 31) return RULGNN_EUNSUPPORTED;   // int rows / 32-bit indices
        C = k.Cout; L = k.Lp;
    }
    g->Lq = L; g->bncount = obn;
    if ((int64_t)g->Lq * 4 * g->h != d64) return RULGNN_EUNSUPPORTED;       // L' 4h != K e: the flat reinterpretation does not exist
    g->o_tw = o; o += g->d3 * d;
    g->o_tb = o; o += g->d3;
    g->o_wd = o; o += M * d;
    g->o_bd = o; o += M;
    g->o_wm = o; o += M * (N + M);
    g->o_bm = o; o += M;
    g->o_f0w = o; o += g->e3 * g->d3 * M;
    g->o_f0b = o; o += g->e3;
    g->o_f1w = o; o += g->e3;
    g->o_f1b = o; o += 1;
    g->pcount = o;
    g->CW = M * d + M + M * (N + M);
    g->lds_fwd = sizeof(float) * (size_t)hc_graph_lds(N, M, d, false).total;
    g->lds_bwd = sizeof(float) * (size_t)hc_graph_lds(N, M, d, true).total;
    if (g->lds_fwd > MAX_LDS_BYTES || g->lds_bwd > MAX_LDS_BYTES) return RULGNN_EUNSUPPORTED;
    WsCarver c;
    auto take = [&c](int64_t nfl) { return (int64_t)(c.take<float>((size_t)(nfl > 0 ? nfl : 1)) / sizeof(float)); };
    g->split_floats = 1024;
    for (int l = 0; l < 3; ++l) {
        HcBlock& k = g->blk[l];
        k.w_in = take(k.R * k.Cin);
        k.w_z = take(k.R * k.Cout);
        k.w_dz = take((k.R + 7) * k.Cout);
        k.w_din = l > 0 ? take(k.R * k.Cin) : 0;
        k.w_wp = take((int64_t)k.Cout * HC_TAPS * k.Cin);
        k.w_wt = l > 0 ? take((int64_t)k.Cin * HC_TAPS * k.Cout) : 0;
        k.w_dwp = take((int64_t)k.Cout * HC_TAPS * k.Cin);
        k.w_coef = take(4 * k.Cout);
        k.w_bcoef = take(2 * k.Cout);
        k.w_part = take((int64_t)2 * HC_SLICES * 2 * k.Cout);        // HC_SLICES x 2 x Cout doubles
        if (B > 0) {
            const size_t need[3] = {sgemm_splitk_need_floats(k.Cout, HC_TAPS * k.Cin, (int)(k.R - 7)),
                                    sgemm_splitk_need_floats((int)(k.R - 7), k.Cout, HC_TAPS * k.Cin),
                                    l > 0 ? sgemm_splitk_need_floats((int)k.R, k.Cin, HC_TAPS * k.Cout) : 0};
            for (size_t v : need) g->split_floats = v > g->split_floats ? v : g->split_floats;
        }
    }
    if (B > 0) {
        const size_t need[2] = {sgemm_splitk_need_floats(g->d3, d, (int)(B * M)), sgemm_splitk_need_floats((int)B, g->e3, M * g->d3)};
        for (size_t v : need) g->split_floats = v > g->split_floats ? v : g->split_floats;
    }
    // the graph stage's HBM traffic: the encoder output (X itself), X', A', A' X' and their gradients -- no N x N or N x d intermediate
    g->w_enc = take(B * N * d);
    g->w_xp = take(B * M * d);
    g->w_ap = take(B * M * M);
    g->w_axp = take(B * M * d);
    g->w_H = take(B * M * g->d3);
    g->w_pre0 = take(B * g->e3);
    g->w_pre1 = take(B);
    g->w_sq = take(B); g->w_dpred = take(B);
    g->w_prod = take(B * (g->e3 + 1));
    g->w_dpre0 = take(B * g->e3);
    g->w_dH = take(B * M * g->d3);
    g->w_dq = take(B * M * d);
    g->w_dxp = take(B * M * d);
    g->w_denc = take(B * N * d);
    g->w_contrib = take(B * g->CW);
    g->w_split = take((int64_t)g->split_floats);
    g->total_bytes = c.total();
    return RULGNN_OK;
}

// HierCorrPool's gate: the packed window in front, the limits of include/rulgnn.h's HierCorrPool section
int hc_geometry(const rulgnn_hiercorrpool_shape* s, HcGeom* g) {
    if (!s) return RULGNN_EINVAL;
    const HcFront fe{0, s->patch_size, s->num_nodes * s->patch_size, HC_MAXN, HC_MAXP, HC_MAXP, HC_MAXD};
    return hc_geometry(s, fe, g);
}

// HierCorrPool_bearing's gate: the STFT's shape (even nperseg, more than nperseg / 2 points to reflect), kwargs that describe it, then the
// shared geometry under RULGNN_HCPB_MAX_*
int hcpb_geometry(const rulgnn_hcpb_shape* s, HcGeom* g) {
    if (!s) return RULGNN_EINVAL;
    if (s->input_dim < 0 || s->nperseg < 0 || s->patch_size < 0 || s->num_nodes < 0) return RULGNN_EINVAL;
    const int ns = s->nperseg;
    if (ns < 2 || (ns & 1) || ns > RULGNN_HCPB_MAX_NPERSEG || s->patch_size <= ns / 2) return RULGNN_EUNSUPPORTED;
    if (s->num_nodes != ns / 2 + 1 || s->input_dim != 1 + s->patch_size / ns || s->input_dim > RULGNN_HCPB_MAX_INPUT_DIM)
        return RULGNN_EUNSUPPORTED;
    const rulgnn_hiercorrpool_shape core{s->batch, s->patch_size, s->num_patch, s->hidden_dim, s->embedding_dim, s->num_nodes,
                                         s->encoder_conv_kernel, s->num_nodes_out};
    // (patch_size < (max_input_dim + 1) nperseg follows from input_dim's limit: the staged patch stays under 5 KB of LDS)
    const HcFront fe{ns, s->input_dim, s->num_nodes * s->input_dim, RULGNN_HCPB_MAX_NODES, RULGNN_HCPB_MAX_NUM_PATCH,
                     (RULGNN_HCPB_MAX_INPUT_DIM + 1) * RULGNN_HCPB_MAX_NPERSEG, RULGNN_HCPB_MAX_D};
    return hc_geometry(&core, fe, g);
}

__device__ __forceinline__ float hc_lrelu(float v) { return v > 0.f ? v : HC_SLOPE * v; }
__device__ __forceinline__ float hc_dlrelu(float v) { return v > 0.f ? 1.f : HC_SLOPE; }

// C[M][N] = sum_k a(m, k) b(k, n) by the whole workgroup on v_mfma_f32_16x16x4_f32: wavefront w takes the (16-row, NB x 16-column) tasks
// w, w + 4, ...; lane (kq, li) = (lane / 16, lane % 16) feeds A[m = li][k = 4 s + kq] and B[k = 4 s + kq][n = li] and receives
// C[m = 4 kq + r][n = li].  a, b are called for in-range indices only (the rest is fed as zeros), c(m, n, value) once for every in-range
// output, always by the same lane for one (M, N, NB).  No barrier inside.
template <int NB, class FA, class FB, class FC>
__device__ __forceinline__ void hc_mm(int M, int N, int K, FA a, FB b, FC c) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, kq = lane >> 4;
    const int mt = (M + 15) >> 4, ng = (N + 16 * NB - 1) / (16 * NB);
    for (int t = wave; t < mt * ng; t += HC_WAVES) {
        const int i = t / ng, j0 = (t - i * ng) * NB;
        f32x4t acc[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) acc[j] = (f32x4t){0.f, 0.f, 0.f, 0.f};
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
        for (int k0 = 0; k0 < K; k0 += 4) {
            const int k = k0 + kq, kc = k < K ? k : K - 1;
            const bool kin = k < K;
            const float a0 = a(mc, kc), av = (m_in && kin) ? a0 : 0.f;
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const float b0 = b(kc, nc[j]);
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, (nin[j] && kin) ? b0 : 0.f, acc[j], 0, 0, 0);
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

inline unsigned hc_grid(int64_t n, int64_t cap) { return (unsigned)(n < 1 ? 1 : (n > cap ? cap : n)); }
inline unsigned hc_blocks(int64_t elems, int64_t cap = 1 << 16) { return hc_grid((elems + HC_GB - 1) / HC_GB, cap); }

// ---- encoder: layout kernels ------------------------------------------------------------------------------------------------------------
// in [b][P + 8][C0], in[b][4 + t][n p + j] = x[b][n][t p + j], zero rows around
__global__ void hc_pack_input_kernel(int64_t B, int N, int P, int p, const float* __restrict__ x, float* __restrict__ in) {
    const int C0 = N * p, rows = P + 2 * HC_PAD;
    const int64_t tot = B * rows * C0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < tot; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C0), r = (int)((i / C0) % rows);
        const int64_t b = i / ((int64_t)C0 * rows);
        const int t = r - HC_PAD;
        float v = 0.f;
        if (t >= 0 && t < P) { const int n = c / p, j = c - n * p; v = x[(b * N + n) * (int64_t)(P * p) + t * p + j]; }
        in[i] = v;
    }
}

// HierCorrPool_bearing's block-1 input, written directly in the layout the convolutions read: in [b][P + 8][C0 = N f],
// in[b][4 + t][n f + j] = |STFT(patch t of sample b)|[bin n][frame j] (torch.stft with n_fft = hop = win = ns, periodic Hann,
// reflect-centred: stft_device.hpp's arithmetic), zero rows around.  THE SPECTROGRAM EXISTS IN NO OTHER LAYOUT AND IN NO OTHER BUFFER:
// this kernel reads the raw window x [b][P p] and its only output is `in`, which the block-1 products read as it stands.
// Work mapping.  The kernel moves 4 (P p + (P + 8) C0) bytes per sample and does ns multiply-adds per output (at most 32): it is bound by
// its stores, so the mapping is chosen for them.  An item is one ROW of the output, (sample, r) with r over the P + 8 rows of a sample: a
// pad row is C0 zeros, any other row is one (sample, patch) -- its reflect-padded patch (p + ns floats; with the tables p + 4 ns, 2.5 KB
// at the widest reference row) is staged in LDS once, the workgroup's threads take the row's N f outputs (at most 289 at the reference's
// rows: one or two passes of 256), and consecutive threads store consecutive floats, so every row is written contiguously and exactly
// once.  Workgroups walk the items in a grid-stride loop and build the twiddle and window tables once each, not once per patch.  With
// the pad rows as items of the same loop the kernel writes every float of `in`: nothing depends on what the workspace held.  No atomics,
// one writer per element: two runs give the same bits.  The STFT is not differentiated (the input has no gradient).
__global__ __launch_bounds__(SB) void hcpb_stft_input_kernel(int64_t B, int N, int f, int P, int p, int ns, const float* __restrict__ x,
                                                             float* __restrict__ in) {
    extern __shared__ float hcpb_sm[];
    const StftLds l = stft_carve(hcpb_sm, p, ns);
    const int tid = threadIdx.x, C0 = N * f, rows = P + 2 * HC_PAD;
    stft_tables(l, ns, tid);
    const int64_t items = B * rows;
    for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
        const int64_t b = it / rows;
        const int t = (int)(it - b * rows) - HC_PAD;
        float* row = in + it * C0;
        if (t < 0 || t >= P) {                             // (the same for every thread of the workgroup)
            for (int c = tid; c < C0; c += SB) row[c] = 0.f;
            continue;
        }
        __syncthreads();                                   // the tables are written; the previous patch has been read
        stft_load_patch(l, x + (b * P + t) * (int64_t)p, p, ns, tid);
        __syncthreads();
        for (int c = tid; c < C0; c += SB) {
            const int n = c / f;
            row[c] = stft_magnitude(l, ns, n, c - n * f);
        }
    }
}

// the three convolution weights W [out][c][tap] as Wp [out][tap][c] and, for blocks 2 and 3, Wt [c][7 - tap][out]; UNPACK: d Wp -> d W
struct HcPack {
    const float* W[3];
    float* Wp[3];
    float* Wt[3];
    int Cin[3], Cout[3];
};
template <bool UNPACK>
__global__ void hc_pack_weights_kernel(HcPack k) {
    for (int l = 0; l < 3; ++l) {
        const int Cin = k.Cin[l], Cout = k.Cout[l];
        const int64_t tot = (int64_t)Cout * Cin * HC_TAPS;
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < tot; i += (int64_t)gridDim.x * blockDim.x) {
            // i indexes Wp: [o][tap][c]
            const int c = (int)(i % Cin), tap = (int)((i / Cin) % HC_TAPS), o = (int)(i / ((int64_t)Cin * HC_TAPS));
            const int64_t wi = ((int64_t)o * Cin + c) * HC_TAPS + tap;
            if (UNPACK) {
                k.Wp[l][wi] = k.W[l][i];                 // (W = the packed gradient, Wp = the parameter-layout gradient)
            } else {
                const float v = k.W[l][wi];
                k.Wp[l][i] = v;
                if (k.Wt[l]) k.Wt[l][((int64_t)c * HC_TAPS + (HC_TAPS - 1 - tap)) * Cout + o] = v;
            }
        }
    }
}

// ---- encoder: BatchNorm / ReLU / max-pool / dropout epilogue ------------------------------------------------------------------------------
struct HcEpi {
    int64_t B;
    int C, Lin, Lc, Lp;
    const float* z;            // [B (Lin + 8)][C]: row b (Lin + 8) + t holds step t < Lc
    const float* coef;         // [4][C]: mean, 1 / sigma, scale, shift
    const float* bcoef;        // [2][C]: mean(dy), mean(dy xhat)       (backward)
    float* out;                // forward: pooled output, row (b orow + ooff + j)
    int orow, ooff;
    const float* dout;         // backward: its gradient, row (b srow + soff + j)
    int srow, soff;
    float* dz;                 // [7 + B (Lin + 8)][C], zero wherever z holds no step
    uint32_t drop_key, drop_thr;
    float drop_scale;          // 0: no dropout here
    int64_t sample_offset;
};

__device__ __forceinline__ float hc_keep(const HcEpi& q, int64_t b, int c, int j) {
    if (q.drop_scale == 0.f) return 1.f;
    const uint32_t ctr = (uint32_t)((((uint64_t)(q.sample_offset + b) * (uint64_t)q.C + (uint64_t)c) * (uint64_t)q.Lp + (uint64_t)j) & 0xFFFFFFFFull);
    return lowbias32(ctr ^ q.drop_key) >= q.drop_thr ? q.drop_scale : 0.f;
}

// d loss / d y (the BatchNorm output) at step t: through the ReLU and to the pool window's winner only (the first index on ties)
__device__ __forceinline__ float hc_dy(const HcEpi& q, int64_t b, int t, int c, float* xhat) {
    const float* zr = q.z + (b * (q.Lin + 2 * HC_PAD)) * q.C + c;
    const float zv = zr[(int64_t)t * q.C], sc = q.coef[2 * q.C + c], sh = q.coef[3 * q.C + c];
    *xhat = (zv - q.coef[c]) * q.coef[q.C + c];
    const float y = zv * sc + sh;
    if (!(y > 0.f)) return 0.f;
    const bool first = (t & 1) != 0;                   // window j = (t + 1) / 2 holds steps 2 j - 1, 2 j
    const int tp = first ? t + 1 : t - 1;
    if (tp >= 0 && tp < q.Lc) {
        const float yp = fmaxf(zr[(int64_t)tp * q.C] * sc + sh, 0.f);
        if (first ? !(y >= yp) : !(y > yp)) return 0.f;
    }
    const int j = (t + 1) >> 1;
    return q.dout[((b * q.srow + q.soff + j)) * q.C + c] * hc_keep(q, b, c, j);
}

// per-channel fp64 partial sums over a slice of the B Lc steps: forward (z, z^2), backward (dy, dy xhat).  grid (C / 64, slices), 256
// threads = 64 channels x 4 step lanes; part [slice][2][C]
template <bool BWD>
__global__ __launch_bounds__(HC_GB) void hc_stats_kernel(HcEpi q, double* __restrict__ part) {
    __shared__ double red[2][4][64];
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6, c = blockIdx.x * 64 + cl;
    const int64_t V = q.B * q.Lc;
    double s0 = 0.0, s1 = 0.0;
    if (c < q.C)
        for (int64_t v = (int64_t)blockIdx.y * 4 + rl; v < V; v += (int64_t)gridDim.y * 4) {
            const int64_t b = v / q.Lc;
            const int t = (int)(v - b * q.Lc);
            if (BWD) {
                float xh;
                const float dy = hc_dy(q, b, t, c, &xh);
                s0 += (double)dy; s1 += (double)dy * (double)xh;
            } else {
                const float zv = q.z[(b * (q.Lin + 2 * HC_PAD) + t) * q.C + c];
                s0 += (double)zv; s1 += (double)zv * (double)zv;
            }
        }
    red[0][rl][cl] = s0; red[1][rl][cl] = s1;
    __syncthreads();
    if (rl == 0 && c < q.C) {
        part[((int64_t)blockIdx.y * 2 + 0) * q.C + c] = (red[0][0][cl] + red[0][1][cl]) + (red[0][2][cl] + red[0][3][cl]);
        part[((int64_t)blockIdx.y * 2 + 1) * q.C + c] = (red[1][0][cl] + red[1][1][cl]) + (red[1][2][cl] + red[1][3][cl]);
    }
}

// forward: the slices in order -> batch moments -> coefficients (eval: from the running statistics) and the running-statistics update;
// backward: -> mean(dy), mean(dy xhat) and the BatchNorm weight / bias gradients
template <bool BWD>
__global__ void hc_stats_finish_kernel(int C, int slices, double count, const double* __restrict__ part, const float* __restrict__ gamma,
                                       const float* __restrict__ beta, float* __restrict__ coef, float* __restrict__ bcoef, float* running,
                                       int training, int update, float* __restrict__ ggamma, float* __restrict__ gbeta) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double s0 = 0.0, s1 = 0.0;
    if (BWD || training)
        for (int s = 0; s < slices; ++s) { s0 += part[((int64_t)s * 2 + 0) * C + c]; s1 += part[((int64_t)s * 2 + 1) * C + c]; }
    if (BWD) {
        bcoef[c] = (float)(s0 / count);
        bcoef[C + c] = (float)(s1 / count);
        gbeta[c] = (float)s0;
        ggamma[c] = (float)s1;
        return;
    }
    BnMoments m;
    if (training) {
        m = bn_moments(s0, s1, count);
        if (update) bn_running_blend(running + c, running + C + c, m.mean, m.var, count, HC_MOMENTUM, 0, 1);
    } else {
        m.mean = running[c]; m.var = running[C + c];
    }
    const BnCoef k = bn_coef(m, gamma[c], beta[c], HC_EPS);
    coef[c] = k.mean; coef[C + c] = k.inv; coef[2 * C + c] = k.sc; coef[3 * C + c] = k.sh;
}

// BN -> ReLU -> max-pool -> dropout, one pass over the output rows (the zero rows of the next block's padded input included)
__global__ void hc_epilogue_fwd_kernel(HcEpi q) {
    const int64_t tot = q.B * q.orow * q.C;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < tot; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % q.C), r = (int)((i / q.C) % q.orow);
        const int64_t b = i / ((int64_t)q.C * q.orow);
        const int j = r - q.ooff;
        float v = 0.f;
        if (j >= 0 && j < q.Lp) {
            const float* zr = q.z + (b * (q.Lin + 2 * HC_PAD)) * q.C + c;
            const float sc = q.coef[2 * q.C + c], sh = q.coef[3 * q.C + c];
            const int t0 = 2 * j - 1, t1 = 2 * j;
            if (t0 >= 0 && t0 < q.Lc) v = fmaxf(zr[(int64_t)t0 * q.C] * sc + sh, 0.f);
            if (t1 < q.Lc) v = fmaxf(v, fmaxf(zr[(int64_t)t1 * q.C] * sc + sh, 0.f));
            v *= hc_keep(q, b, c, j);
        }
        q.out[i] = v;
    }
}

// dz = gamma / sigma (dy - mean(dy) - xhat mean(dy xhat)) on the rows that hold a step, zero on the seven leading rows and between samples
__global__ void hc_dz_kernel(HcEpi q, const float* __restrict__ gamma) {
    const int rows = q.Lin + 2 * HC_PAD;
    const int64_t tot = (q.B * rows + 7) * q.C;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < tot; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % q.C);
        const int64_t r = i / q.C - 7;
        float v = 0.f;
        if (r >= 0) {
            const int64_t b = r / rows;
            const int t = (int)(r - b * rows);
            if (t < q.Lc) {
                float xh;
                const float dy = hc_dy(q, b, t, c, &xh);
                v = gamma[c] * q.coef[q.C + c] * (dy - q.bcoef[c] - xh * q.bcoef[q.C + c]);
            }
        }
        q.dz[i] = v;
    }
}

// ---- graph stage ------------------------------------------------------------------------------------------------------------------------
struct HcGraphBufs {
    const float* enc;          // [B][L'][C3] = X through the flat reinterpretation
    float *xp, *ap, *axp;      // X' [B][M][d], A' [B][M][M], A' X' [B][M][d]: all of the stage that reaches HBM
    const float* dq;           // backward: d (A' X') [B][M][d]
    float* dxp;                // backward scratch: d X' [B][M][d]
    float* denc;               // backward: d enc
    float* contrib;            // backward: [B][CW] per-sample [d Wd | d bd | d Wm]
};

// X, G, A, AX, Z, S of sample b into LDS (what both directions start from)
template <bool BWD>
__device__ __forceinline__ void hc_graph_common(const HcGeom& g, const HcGraphLds& l, float* lds, const float* __restrict__ prm, const float* F) {
    const int N = g.N, M = g.M, d = g.d, e = g.e, LD = d + 1, NL = N + 1, ML = M + 1, tid = threadIdx.x;
    float* X = lds + l.X; float* AX = lds + l.AX; float* A = lds + l.A; float* Z = lds + l.Z; float* S = lds + l.S; float* G = lds + l.G;
    const float* Wd = prm + g.o_wd; const float* bd = prm + g.o_bd; const float* Wm = prm + g.o_wm; const float* bm = prm + g.o_bm;
    for (int i = tid; i < N * d; i += HC_GB) {
        const int q = i % e, n = (i / e) % N, k = i / (e * N);
        X[n * LD + k * e + q] = F[i];
    }
    __syncthreads();
    hc_mm<2>(N, N, d, [&](int m, int k) { return X[m * LD + k]; }, [&](int k, int n) { return X[n * LD + k]; },
             [&](int m, int n, float v) { A[m * NL + n] = v; });
    __syncthreads();
    if (tid < N) {
        float* row = A + tid * NL;
        float mx = -INFINITY;
        for (int j = 0; j < N; ++j) {
            if (BWD) G[tid * NL + j] = row[j];
            if (j != tid) mx = fmaxf(mx, hc_lrelu(row[j]));
        }
        float sum = 0.f;
        for (int j = 0; j < N; ++j)
            if (j != tid) { const float ex = expf(hc_lrelu(row[j]) - mx); row[j] = ex; sum += ex; }
        const float inv = 1.0f / sum;
        for (int j = 0; j < N; ++j) row[j] = j != tid ? row[j] * inv : 1.0f;
    }
    __syncthreads();
    hc_mm<4>(N, d, N, [&](int m, int k) { return A[m * NL + k]; }, [&](int k, int n) { return X[k * LD + n]; },
             [&](int m, int n, float v) { AX[m * LD + n] = v; });
    __syncthreads();
    hc_mm<1>(N, M, d, [&](int m, int k) { return AX[m * LD + k]; }, [&](int k, int n) { return Wd[n * d + k]; },
             [&](int m, int n, float v) { Z[m * ML + n] = 1.0f / (1.0f + expf(-(v + bd[n]))); });
    __syncthreads();
    for (int i = tid; i < N * M; i += HC_GB) {
        const int n = i / M, m = i - n * M;
        const float* w = Wm + m * (N + M);
        float a = bm[m];
        for (int j = 0; j < N; ++j) a = fmaf(A[n * NL + j], w[j], a);
        for (int j = 0; j < M; ++j) a = fmaf(Z[n * ML + j], w[N + j], a);
        S[n * ML + m] = a;
    }
    __syncthreads();
    if (tid < M) {
        float mx = -INFINITY;
        for (int n = 0; n < N; ++n) mx = fmaxf(mx, S[n * ML + tid]);
        float sum = 0.f;
        for (int n = 0; n < N; ++n) { const float ex = expf(S[n * ML + tid] - mx); S[n * ML + tid] = ex; sum += ex; }
        const float inv = 1.0f / sum;
        for (int n = 0; n < N; ++n) S[n * ML + tid] *= inv;
    }
    __syncthreads();
}

__global__ __launch_bounds__(HC_GB) void hcp_graph_fwd(HcGeom g, const float* __restrict__ prm, HcGraphBufs q) {
    extern __shared__ float lds[];
    const int N = g.N, M = g.M, d = g.d, LD = d + 1, NL = N + 1, ML = M + 1, tid = threadIdx.x;
    const HcGraphLds l = hc_graph_lds(N, M, d, false);
    float* X = lds + l.X; float* R = lds + l.AX; float* A = lds + l.A; float* S = lds + l.S; float* SA = lds + l.SA; float* Ap = lds + l.Ap;
    for (int64_t b = blockIdx.x; b < g.B; b += gridDim.x) {
        __syncthreads();
        hc_graph_common<false>(g, l, lds, prm, q.enc + b * N * d);
        float* xp = q.xp + b * M * d;
        hc_mm<4>(M, d, N, [&](int m, int k) { return S[k * ML + m]; }, [&](int k, int n) { return X[k * LD + n]; },
                 [&](int m, int n, float v) { R[m * LD + n] = v; xp[m * d + n] = v; });
        for (int i = tid; i < M * N; i += HC_GB) {
            const int m = i / N, j = i - m * N;
            float a = 0.f;
            for (int n = 0; n < N; ++n) a = fmaf(S[n * ML + m], A[n * NL + j], a);
            SA[m * NL + j] = a;
        }
        __syncthreads();
        for (int i = tid; i < M * M; i += HC_GB) {
            const int m = i / M, m2 = i - m * M;
            float a = 0.f;
            for (int j = 0; j < N; ++j) a = fmaf(SA[m * NL + j], S[j * ML + m2], a);
            Ap[m * ML + m2] = a;
            q.ap[b * M * M + i] = a;
        }
        __syncthreads();
        float* axp = q.axp + b * M * d;
        hc_mm<4>(M, d, M, [&](int m, int k) { return Ap[m * ML + k]; }, [&](int k, int n) { return R[k * LD + n]; },
                 [&](int m, int n, float v) { axp[m * d + n] = v; });
    }
}

__global__ __launch_bounds__(HC_GB) void hcp_graph_bwd(HcGeom g, const float* __restrict__ prm, HcGraphBufs q) {
    extern __shared__ float lds[];
    const int N = g.N, M = g.M, d = g.d, e = g.e, LD = d + 1, NL = N + 1, ML = M + 1, tid = threadIdx.x;
    const HcGraphLds l = hc_graph_lds(N, M, d, true);
    float* X = lds + l.X; float* AX = lds + l.AX; float* A = lds + l.A; float* Z = lds + l.Z; float* S = lds + l.S; float* G = lds + l.G;
    float* dA = lds + l.dA; float* dS = lds + l.dS; float* AS = lds + l.AS; float* AtS = lds + l.AtS; float* SdA = lds + l.SdA;
    float* dZp = lds + l.dZp; float* dAp = lds + l.dAp; float* cs = lds + l.cs;
    const float* Wd = prm + g.o_wd; const float* Wm = prm + g.o_wm;
    for (int64_t b = blockIdx.x; b < g.B; b += gridDim.x) {
        __syncthreads();
        hc_graph_common<true>(g, l, lds, prm, q.enc + b * N * d);
        const float* dQ = q.dq + b * M * d;
        const float* xpg = q.xp + b * M * d;
        const float* apg = q.ap + b * M * M;
        float* dxp = q.dxp + b * M * d;
        float* part = q.contrib + b * g.CW;
        // dA' = dQ X'^T, dX' = A'^T dQ
        hc_mm<1>(M, M, d, [&](int m, int k) { return dQ[m * d + k]; }, [&](int k, int n) { return xpg[n * d + k]; },
                 [&](int m, int n, float v) { dAp[m * ML + n] = v; });
        hc_mm<4>(M, d, M, [&](int m, int k) { return apg[k * M + m]; }, [&](int k, int n) { return dQ[k * d + n]; },
                 [&](int m, int n, float v) { dxp[m * d + n] = v; });
        for (int i = tid; i < N * M; i += HC_GB) {
            const int n = i / M, m = i - n * M;
            float a = 0.f, at = 0.f;
            for (int j = 0; j < N; ++j) { a = fmaf(A[n * NL + j], S[j * ML + m], a); at = fmaf(A[j * NL + n], S[j * ML + m], at); }
            AS[n * ML + m] = a; AtS[n * ML + m] = at;
        }
        __syncthreads();                   // (dX' of this sample is read back below: same workgroup)
        // dS = X dX'^T + (A S) dA'^T + (A^T S) dA'
        hc_mm<1>(N, M, d, [&](int m, int k) { return X[m * LD + k]; }, [&](int k, int n) { return dxp[n * d + k]; },
                 [&](int m, int n, float v) {
                     for (int j = 0; j < M; ++j) v += AS[m * ML + j] * dAp[n * ML + j] + AtS[m * ML + j] * dAp[j * ML + n];
                     dS[m * ML + n] = v;
                 });
        for (int i = tid; i < N * M; i += HC_GB) {
            const int n = i / M, m = i - n * M;
            float a = 0.f;
            for (int j = 0; j < M; ++j) a = fmaf(S[n * ML + j], dAp[j * ML + m], a);
            SdA[n * ML + m] = a;
        }
        __syncthreads();
        if (tid < M) {
            float a = 0.f;
            for (int n = 0; n < N; ++n) a = fmaf(S[n * ML + tid], dS[n * ML + tid], a);
            cs[tid] = a;
        }
        __syncthreads();
        for (int i = tid; i < N * M; i += HC_GB) {          // dT over dS
            const int n = i / M, m = i - n * M;
            dS[n * ML + m] = S[n * ML + m] * (dS[n * ML + m] - cs[m]);
        }
        __syncthreads();
        // d Wm = dT^T [A | Z]
        for (int i = tid; i < M * (N + M); i += HC_GB) {
            const int m = i / (N + M), j = i - m * (N + M);
            float a = 0.f;
            if (j < N) for (int n = 0; n < N; ++n) a = fmaf(dS[n * ML + m], A[n * NL + j], a);
            else for (int n = 0; n < N; ++n) a = fmaf(dS[n * ML + m], Z[n * ML + j - N], a);
            part[M * d + M + i] = a;
        }
        // dA = S dA' S^T + dT Wa;  dZp = (dT Wz) Z (1 - Z)
        for (int i = tid; i < N * N; i += HC_GB) {
            const int r = i / N, j = i - r * N;
            float a = 0.f;
            for (int m = 0; m < M; ++m) a += SdA[r * ML + m] * S[j * ML + m] + dS[r * ML + m] * Wm[m * (N + M) + j];
            dA[r * NL + j] = a;
        }
        for (int i = tid; i < N * M; i += HC_GB) {
            const int n = i / M, j = i - n * M;
            float a = 0.f;
            for (int m = 0; m < M; ++m) a = fmaf(dS[n * ML + m], Wm[m * (N + M) + N + j], a);
            const float z = Z[n * ML + j];
            dZp[n * ML + j] = a * z * (1.f - z);
        }
        __syncthreads();
        if (tid < M) {
            float a = 0.f;
            for (int n = 0; n < N; ++n) a += dZp[n * ML + tid];
            part[M * d + tid] = a;
        }
        hc_mm<4>(M, d, N, [&](int m, int k) { return dZp[k * ML + m]; }, [&](int k, int n) { return AX[k * LD + n]; },
                 [&](int m, int n, float v) { part[m * d + n] = v; });
        __syncthreads();
        hc_mm<4>(N, d, M, [&](int m, int k) { return dZp[m * ML + k]; }, [&](int k, int n) { return Wd[k * d + n]; },
                 [&](int m, int n, float v) { AX[m * LD + n] = v; });          // d(AX) over AX
        __syncthreads();
        hc_mm<2>(N, N, d, [&](int m, int k) { return AX[m * LD + k]; }, [&](int k, int n) { return X[n * LD + k]; },
                 [&](int m, int n, float v) { dA[m * NL + n] += v; });
        __syncthreads();
        if (tid < N) {                       // through the row softmax and the leaky ReLU: dG over dA, nothing on the diagonal
            float* row = dA + tid * NL;
            const float* pr = A + tid * NL;
            float s = 0.f;
            for (int j = 0; j < N; ++j)
                if (j != tid) s = fmaf(pr[j], row[j], s);
            for (int j = 0; j < N; ++j) row[j] = j != tid ? pr[j] * (row[j] - s) * hc_dlrelu(G[tid * NL + j]) : 0.f;
        }
        __syncthreads();
        // dX = S dX' + A^T d(AX) + (dG + dG^T) X, one product over k = M + N + N, written through the flat reinterpretation
        float* de = q.denc + b * N * d;
        hc_mm<4>(N, d, M + 2 * N,
                 [&](int m, int k) {
                     if (k < M) return S[m * ML + k];
                     if (k < M + N) return A[(k - M) * NL + m];
                     return dA[m * NL + k - M - N] + dA[(k - M - N) * NL + m];
                 },
                 [&](int k, int n) {
                     if (k < M) return dxp[k * d + n];
                     if (k < M + N) return AX[(k - M) * LD + n];
                     return X[(k - M - N) * LD + n];
                 },
                 [&](int m, int n, float v) { de[((n / e) * N + m) * e + n % e] = v; });
    }
}

// ---- head -------------------------------------------------------------------------------------------------------------------------------
// v[r][c] = leaky(v[r][c] + bias[c]); BWD: v = dH * leaky'(H)
template <bool BWD>
__global__ void hc_bias_leaky_kernel(int64_t rows, int C, float* __restrict__ v, const float* __restrict__ bias, const float* __restrict__ H) {
    const int64_t tot = rows * C;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < tot; i += (int64_t)gridDim.x * blockDim.x)
        v[i] = BWD ? v[i] * hc_dlrelu(H[i]) : hc_lrelu(v[i] + bias[i % C]);
}

// a0 = leaky(pre0 + b0) in place, pre1 = a0 . w1 + b1, pred = leaky(pre1); with y the squared-error share and d loss / d pred
__global__ void hc_head_kernel(HcGeom g, const float* __restrict__ prm, float* __restrict__ pre0, float* __restrict__ pre1, const float* __restrict__ y,
                               float* __restrict__ pred, float* __restrict__ sq, float* __restrict__ dpred, float inv_gb) {
    const int E = g.e3;
    for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < g.B; b += (int64_t)gridDim.x * blockDim.x) {
        float a = prm[g.o_f1b];
        for (int i = 0; i < E; ++i) {
            const float v = hc_lrelu(pre0[b * E + i] + prm[g.o_f0b + i]);
            pre0[b * E + i] = v;
            a = fmaf(v, prm[g.o_f1w + i], a);
        }
        pre1[b] = a;
        const float pv = hc_lrelu(a);
        pred[b] = pv;
        if (y) {
            const float df = pv - y[b];
            sq[b] = df * df * inv_gb;
            dpred[b] = 2.f * df * inv_gb;
        }
    }
}

// d1 = dpred leaky'(pre1); dpre0 = d1 w1 leaky'(a0); prod [B][3e + 1] = [d1 a0 | d1], whose column sums are g fc_1.weight | g fc_1.bias;
// g matrix.bias = 0 exactly (the bias is constant along the softmax axis)
__global__ void hc_head_bwd_kernel(HcGeom g, const float* __restrict__ prm, const float* __restrict__ a0, const float* __restrict__ pre1,
                                   const float* __restrict__ dpred, float* __restrict__ prod, float* __restrict__ dpre0, float* __restrict__ gr) {
    const int E = g.e3;
    for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < g.B; b += (int64_t)gridDim.x * blockDim.x) {
        const float v = dpred[b] * hc_dlrelu(pre1[b]);
        prod[b * (E + 1) + E] = v;
        for (int i = 0; i < E; ++i) {
            const float av = a0[b * E + i];
            prod[b * (E + 1) + i] = v * av;
            dpre0[b * E + i] = v * prm[g.o_f1w + i] * hc_dlrelu(av);
        }
    }
    if (blockIdx.x == 0 && (int)threadIdx.x < g.M) gr[g.o_bm + threadIdx.x] = 0.f;
}

HcEpi hc_epi(const HcGeom& g, int l, float* ws, const rulgnn_hiercorrpool_args* a) {
    const HcBlock& k = g.blk[l];
    HcEpi q{};
    q.B = g.B; q.C = k.Cout; q.Lin = k.Lin; q.Lc = k.Lc; q.Lp = k.Lp;
    q.z = ws + k.w_z; q.coef = ws + k.w_coef; q.bcoef = ws + k.w_bcoef; q.dz = ws + k.w_dz;
    if (l < 2) {
        q.out = ws + g.blk[l + 1].w_in; q.orow = k.Lp + 2 * HC_PAD; q.ooff = HC_PAD;
        q.dout = ws + g.blk[l + 1].w_din; q.srow = k.Lp + 2 * HC_PAD; q.soff = HC_PAD;
    } else {
        q.out = ws + g.w_enc; q.orow = k.Lp; q.ooff = 0;
        q.dout = ws + g.w_denc; q.srow = k.Lp; q.soff = 0;
    }
    q.sample_offset = a->sample_offset;
    if (l == 0 && a->training && a->dropout_p > 0.f) {
        const DropoutConst dc = dropout_const(a->dropout_p);
        q.drop_key = dropout_layer_key(a->seed, a->step, 0); q.drop_thr = dc.thr; q.drop_scale = dc.scale;
    }
    return q;
}

// The chain of both families; the front end (g.ns) decides the first launch and nothing else.
// mode bit 0: forward, bit 1: backward (after a forward with the same args / workspace)
int hc_run(const HcGeom& g, const rulgnn_hiercorrpool_args* a, int mode, hipStream_t st) {
    if (a->workspace_bytes < g.total_bytes) return RULGNN_EWORKSPACE;
    if (g.B == 0) return RULGNN_OK;
    float* ws = static_cast<float*>(a->workspace);
    const float* prm = a->params;
    const int64_t gb = a->global_batch > 0 ? a->global_batch : g.B;
    const int64_t B = g.B;
    const int N = g.N, M = g.M, d = g.d, d3 = g.d3, e3 = g.e3, BM = (int)(B * M);
    HcGraphBufs gq{ws + g.w_enc, ws + g.w_xp, ws + g.w_ap, ws + g.w_axp, ws + g.w_dq, ws + g.w_dxp, ws + g.w_denc, ws + g.w_contrib};
    const float* dpred = a->dpred ? a->dpred : ws + g.w_dpred;
    if (mode & 1) {
        if (g.ns)
            RULGNN_TRY(launch_checked(hcpb_stft_input_kernel, dim3(hc_grid(g.blk[0].R, HCPB_GRID)), dim3(SB), sizeof(float) * stft_lds_floats(g.p, g.ns), st,
                                      B, N, g.w, g.P, g.p, g.ns, a->x, ws + g.blk[0].w_in));
        else
            RULGNN_TRY(launch_checked(hc_pack_input_kernel, dim3(hc_blocks(g.blk[0].R * g.blk[0].Cin)), dim3(HC_GB), 0, st, B, N, g.P, g.p, a->x, ws + g.blk[0].w_in));
        HcPack pk{};
        for (int l = 0; l < 3; ++l) {
            const HcBlock& k = g.blk[l];
            pk.W[l] = prm + k.o_w; pk.Wp[l] = ws + k.w_wp; pk.Wt[l] = l > 0 ? ws + k.w_wt : nullptr; pk.Cin[l] = k.Cin; pk.Cout[l] = k.Cout;
        }
        RULGNN_TRY(launch_checked(hc_pack_weights_kernel<false>, dim3(hc_blocks((int64_t)g.blk[2].Cout * g.blk[2].Cin * HC_TAPS, 4096)), dim3(HC_GB), 0, st, pk));
        for (int l = 0; l < 3; ++l) {
            const HcBlock& k = g.blk[l];
            // z [R - 7][Cout] = (overlapping-row view of the padded input) [R - 7][8 Cin] . Wp^T
            // (split-K in fixed slices: at the reference's batch the output is a few dozen tiles over k = 8 Cin)
            RULGNN_TRY(sgemm_splitk(ws + k.w_in, k.Cin, 1, ws + k.w_wp, (int64_t)HC_TAPS * k.Cin, 1, ws + k.w_z, k.Cout, (int)(k.R - 7), k.Cout,
                                    HC_TAPS * k.Cin, false, ws + g.w_split, st));
            const HcEpi q = hc_epi(g, l, ws, a);
            double* part = reinterpret_cast<double*>(ws + k.w_part);
            const int slices = (int)hc_grid((B * k.Lc + 31) / 32, HC_SLICES);
            if (a->training) RULGNN_TRY(launch_checked(hc_stats_kernel<false>, dim3((k.Cout + 63) / 64, slices), dim3(HC_GB), 0, st, q, part));
            RULGNN_TRY(launch_checked(hc_stats_finish_kernel<false>, dim3((k.Cout + 63) / 64), dim3(64), 0, st, k.Cout, slices, (double)(B * k.Lc),
                                      (const double*)part, prm + k.o_g, prm + k.o_b, ws + k.w_coef, ws + k.w_bcoef, a->bn_state + k.o_bn,
                                      a->training ? 1 : 0, (a->training && a->update_running_stats) ? 1 : 0, (float*)nullptr, (float*)nullptr));
            RULGNN_TRY(launch_checked(hc_epilogue_fwd_kernel, dim3(hc_blocks(B * q.orow * k.Cout)), dim3(HC_GB), 0, st, q));
        }
        RULGNN_TRY(allow_dynamic_lds(hcp_graph_fwd, g.lds_fwd));
        RULGNN_TRY(launch_checked(hcp_graph_fwd, dim3(hc_grid(B, 8192)), dim3(HC_GB), g.lds_fwd, st, g, prm, gq));
        // H = leaky((A' X') Wt^T + bt); pre0 = H.flat fc_0^T
        RULGNN_TRY(sgemm(ws + g.w_axp, d, 1, prm + g.o_tw, d, 1, ws + g.w_H, d3, BM, d3, d, false, st));
        RULGNN_TRY(launch_checked(hc_bias_leaky_kernel<false>, dim3(hc_blocks((int64_t)BM * d3)), dim3(HC_GB), 0, st, (int64_t)BM, d3, ws + g.w_H, prm + g.o_tb,
                                  (const float*)nullptr));
        RULGNN_TRY(sgemm_splitk(ws + g.w_H, (int64_t)M * d3, 1, prm + g.o_f0w, (int64_t)M * d3, 1, ws + g.w_pre0, e3, (int)B, e3, M * d3, false,
                                ws + g.w_split, st));
        RULGNN_TRY(launch_checked(hc_head_kernel, dim3(hc_blocks(B, 4096)), dim3(HC_GB), 0, st, g, prm, ws + g.w_pre0, ws + g.w_pre1, a->y, a->pred, ws + g.w_sq,
                                  ws + g.w_dpred, 1.0f / (float)gb));
        if (a->y && a->loss) RULGNN_TRY(block_sum((const float*)(ws + g.w_sq), B, a->loss, st));
    }
    if (mode & 2) {
        if (!a->grads) return RULGNN_EINVAL;
        float* gr = a->grads;
        RULGNN_TRY(launch_checked(hc_head_bwd_kernel, dim3(hc_blocks(B, 4096)), dim3(HC_GB), 0, st, g, prm, (const float*)(ws + g.w_pre0), (const float*)(ws + g.w_pre1),
                                  dpred, ws + g.w_prod, ws + g.w_dpre0, gr));
        // g fc_0.weight [3e][3dM] = dpre0^T H.flat (k = the batch, one fixed-order product); dH = dpre0 fc_0
        RULGNN_TRY(sgemm(ws + g.w_dpre0, 1, e3, ws + g.w_H, 1, (int64_t)M * d3, gr + g.o_f0w, (int64_t)M * d3, e3, M * d3, (int)B, false, st));
        RULGNN_TRY(sgemm(ws + g.w_dpre0, e3, 1, prm + g.o_f0w, 1, (int64_t)M * d3, ws + g.w_dH, (int64_t)M * d3, (int)B, M * d3, e3, false, st));
        RULGNN_TRY(launch_checked(hc_bias_leaky_kernel<true>, dim3(hc_blocks((int64_t)BM * d3)), dim3(HC_GB), 0, st, (int64_t)BM, d3, ws + g.w_dH,
                                  (const float*)nullptr, (const float*)(ws + g.w_H)));
        {   // [g fc_1.weight | g fc_1.bias], g fc_0.bias and g theta.bias: three fixed-order column sums in one launch
            const float* const part[3] = {ws + g.w_prod, ws + g.w_dpre0, ws + g.w_dH};
            float* const out[3] = {gr + g.o_f1w, gr + g.o_f0b, gr + g.o_tb};
            const int rows[3] = {(int)B, (int)B, BM}, n[3] = {e3 + 1, e3, d3};
            const int64_t ld[3] = {e3 + 1, e3, d3};
            RULGNN_TRY(rows_sum_three(part, out, rows, ld, n, st));
        }
        // g theta.weight [3d][d] = dHpre^T (A' X') over all B M rows; d(A' X') = dHpre Wt
        RULGNN_TRY(sgemm_splitk(ws + g.w_dH, 1, d3, ws + g.w_axp, 1, d, gr + g.o_tw, d, d3, d, BM, false, ws + g.w_split, st));
        RULGNN_TRY(sgemm(ws + g.w_dH, d3, 1, prm + g.o_tw, 1, d, ws + g.w_dq, d, BM, d, d3, false, st));
        RULGNN_TRY(allow_dynamic_lds(hcp_graph_bwd, g.lds_bwd));
        RULGNN_TRY(launch_checked(hcp_graph_bwd, dim3(hc_grid(B, 8192)), dim3(HC_GB), g.lds_bwd, st, g, prm, gq));
        // [g Wd | g bd | g Wm] = the samples' contributions in order (contiguous in the parameter layout)
        RULGNN_TRY(rows_sum(ws + g.w_contrib, (int)B, g.CW, g.CW, gr + g.o_wd, st));
        HcPack up{};
        for (int l = 2; l >= 0; --l) {
            const HcBlock& k = g.blk[l];
            const HcEpi q = hc_epi(g, l, ws, a);
            double* part = reinterpret_cast<double*>(ws + k.w_part);
            const int slices = (int)hc_grid((B * k.Lc + 31) / 32, HC_SLICES);
            RULGNN_TRY(launch_checked(hc_stats_kernel<true>, dim3((k.Cout + 63) / 64, slices), dim3(HC_GB), 0, st, q, part));
            RULGNN_TRY(launch_checked(hc_stats_finish_kernel<true>, dim3((k.Cout + 63) / 64), dim3(64), 0, st, k.Cout, slices, (double)(B * k.Lc),
                                      (const double*)part, prm + k.o_g, prm + k.o_b, ws + k.w_coef, ws + k.w_bcoef, (float*)nullptr, 1, 0, gr + k.o_g, gr + k.o_b));
            RULGNN_TRY(launch_checked(hc_dz_kernel, dim3(hc_blocks((k.R + 7) * k.Cout)), dim3(HC_GB), 0, st, q, prm + k.o_g));
            const float* dz = ws + k.w_dz + (int64_t)7 * k.Cout;           // row r of z's numbering
            // d Wp [Cout][8 Cin] = dz^T . view, k = the R - 7 rows in fixed slices
            RULGNN_TRY(sgemm_splitk(dz, 1, k.Cout, ws + k.w_in, 1, k.Cin, ws + k.w_dwp, (int64_t)HC_TAPS * k.Cin, k.Cout, HC_TAPS * k.Cin, (int)(k.R - 7),
                                    false, ws + g.w_split, st));
            // d input [R][Cin] = (overlapping-row view of dz from its leading zero rows) [R][8 Cout] . Wt^T
            if (l > 0)
                RULGNN_TRY(sgemm_splitk(ws + k.w_dz, k.Cout, 1, ws + k.w_wt, (int64_t)HC_TAPS * k.Cout, 1, ws + k.w_din, k.Cin, (int)k.R, k.Cin,
                                        HC_TAPS * k.Cout, false, ws + g.w_split, st));
            up.W[l] = ws + k.w_dwp; up.Wp[l] = gr + k.o_w; up.Wt[l] = nullptr; up.Cin[l] = k.Cin; up.Cout[l] = k.Cout;
        }
        RULGNN_TRY(launch_checked(hc_pack_weights_kernel<true>, dim3(hc_blocks((int64_t)g.blk[2].Cout * g.blk[2].Cin * HC_TAPS, 4096)), dim3(HC_GB), 0, st, up));
    }
    return RULGNN_OK;
}

// workspace taps of both families, float offsets (4, 5: the block-1 input and block 1's convolution output, which follows it)
int64_t hc_tap(const HcGeom& g, int which, bool bearing) {
    switch (which) {
        case 0: return g.w_enc;
        case 1: return g.w_xp;
        case 2: return g.w_ap;
        case 3: return g.w_H;
        case 4: return bearing ? g.blk[0].w_in : -1;
        case 5: return bearing ? g.blk[0].w_z : -1;
        default: return -1;
    }
}

}  // namespace

// RULGNN_OK, or the code every entry returns for a refused shape: hc_geometry's own.
int Hiercorrpool::shape_status(const Shape* s) {
    HcGeom g;
    return hc_geometry(s, &g);
}

int64_t Hiercorrpool::param_count(const Shape* s) {
    HcGeom g;
    return hc_geometry(s, &g) == RULGNN_OK ? g.pcount : -1;
}

int64_t Hiercorrpool::bn_state_count(const Shape* s) {
    HcGeom g;
    return hc_geometry(s, &g) == RULGNN_OK ? g.bncount : -1;
}

size_t Hiercorrpool::workspace_bytes(const Shape* s) {
    HcGeom g;
    return hc_geometry(s, &g) == RULGNN_OK ? g.total_bytes : 0;
}

int64_t Hiercorrpool::tap_offset(const Shape* s, int which) {
    HcGeom g;
    return hc_geometry(s, &g) == RULGNN_OK ? hc_tap(g, which, false) : -1;
}

int Hiercorrpool::run(const Shape* s, const Args* a, int mode, hipStream_t st) {
    HcGeom g;
    RULGNN_TRY(hc_geometry(s, &g));
    return hc_run(g, a, mode, st);
}

// ---- HierCorrPool_bearing: the same chain behind hcpb_geometry -----------------------------------------------------------------------------
int Hcpb::shape_status(const Shape* s) {
    HcGeom g;
    return hcpb_geometry(s, &g);
}

int64_t Hcpb::param_count(const Shape* s) {
    HcGeom g;
    return hcpb_geometry(s, &g) == RULGNN_OK ? g.pcount : -1;
}

int64_t Hcpb::bn_state_count(const Shape* s) {
    HcGeom g;
    return hcpb_geometry(s, &g) == RULGNN_OK ? g.bncount : -1;
}

size_t Hcpb::workspace_bytes(const Shape* s) {
    HcGeom g;
    return hcpb_geometry(s, &g) == RULGNN_OK ? g.total_bytes : 0;
}

int64_t Hcpb::tap_offset(const Shape* s, int which) {
    HcGeom g;
    return hcpb_geometry(s, &g) == RULGNN_OK ? hc_tap(g, which, true) : -1;
}

int Hcpb::run(const Shape* s, const Args* a, int mode, hipStream_t st) {
    HcGeom g;
    RULGNN_TRY(hcpb_geometry(s, &g));
    return hc_run(g, a, mode, st);
}

}  // namespace rulgnn
