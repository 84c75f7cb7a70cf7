// What the STFT families (STNet: stnet.hip, GDAGDL: gdagdl.hip) share on the device: the STFT magnitude of one (sample, patch) in LDS,
// and the small element-wise / reduction kernels of their common back end (auto-encoder, reconstruction term, head).  Each translation
// unit that includes this gets its own copies of the kernels (anonymous namespace); the arithmetic is stated here once.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rulgnn {

namespace {

constexpr int SB = 256;

// ---- STFT magnitude (n_fft = hop = win = ns, periodic Hann, reflect-centred: torch.stft's defaults), one workgroup per patch -------
// LDS floats in front of the magnitude tile: the reflect-padded patch [P + ns], cos / sin [ns] each, the window [ns].
__host__ __device__ inline size_t stft_lds_floats(int P, int ns) { return (size_t)P + 4 * (size_t)ns; }

struct StftLds {
    float *xp, *cs, *sn, *win, *end;
};
__device__ __forceinline__ StftLds stft_carve(float* sm, int P, int ns) {
    StftLds l;
    l.xp = sm;                        // [P + ns] reflect-padded patch
    l.cs = l.xp + P + ns;             // [ns] cos(2 pi j / ns)
    l.sn = l.cs + ns;                 // [ns] sin
    l.win = l.sn + ns;                // [ns] periodic Hann
    l.end = l.win + ns;
    return l;
}
__device__ __forceinline__ void stft_tables(const StftLds& l, int ns, int tid) {
    for (int j = tid; j < ns; j += SB) {
        const float a = 6.283185307179586f * (float)j / (float)ns;
        l.cs[j] = cosf(a);
        l.sn[j] = sinf(a);
        l.win[j] = 0.5f - 0.5f * cosf(a);
    }
}
__device__ __forceinline__ void stft_load_patch(const StftLds& l, const float* __restrict__ px, int P, int ns, int tid) {
    const int half = ns / 2;
    for (int i = tid; i < P + ns; i += SB) {
        int q = i - half;                                   // reflect without repeating the edge sample (torch 'reflect')
        if (q < 0) q = -q;
        if (q >= P) q = 2 * (P - 1) - q;
        l.xp[i] = px[q];
    }
}
// |STFT| of frequency bin k, frame t
__device__ __forceinline__ float stft_magnitude(const StftLds& l, int ns, int k, int t) {
    float re = 0.f, im = 0.f;
    for (int m = 0; m < ns; ++m) {
        const float v = l.xp[t * ns + m] * l.win[m];
        const int j = (k * m) % ns;
        re = fmaf(v, l.cs[j], re);
        im = fmaf(-v, l.sn[j], im);
    }
    return sqrtf(re * re + im * im);
}

// ---- back end ---------------------------------------------------------------------------------------------------------------------
__global__ void sn_bias_act_kernel(float* __restrict__ z, const float* __restrict__ bias, int64_t rows, int C, int relu) {
    const int64_t n = rows * C;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float v = z[i] + bias[i % C];
        z[i] = relu ? fmaxf(v, 0.f) : v;
    }
}

__global__ void sn_relu_bwd_kernel(float* __restrict__ d, const float* __restrict__ h, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        d[i] = h[i] > 0.f ? d[i] : 0.f;
}

// a *= w[0], b *= w[0]: the reconstruction term's gradients under a weight other than 1 (autograd path)
__global__ void sn_scale2_kernel(float* __restrict__ a, float* __restrict__ b, int64_t n, const float* __restrict__ w) {
    const float s = w[0];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        a[i] *= s;
        b[i] *= s;
    }
}
__global__ void sn_add_kernel(float* __restrict__ a, const float* __restrict__ b, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) a[i] += b[i];
}

// reconstruction error: partial sums of (Yo - Yp)^2 (one per workgroup, fixed assignment), d Yp = -2 s (Yo - Yp), d Yo = +2 s (Yo - Yp)
__global__ __launch_bounds__(SB) void sn_recon_kernel(const float* __restrict__ yo, const float* __restrict__ yp, int64_t n, float scale,
                                                      float* __restrict__ dyp, float* __restrict__ dyo, float* __restrict__ part) {
    __shared__ float red[SB];
    float a = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * SB + threadIdx.x; i < n; i += (int64_t)gridDim.x * SB) {
        const float d = yo[i] - yp[i];
        a = fmaf(d, d, a);
        if (dyp) { dyp[i] = -2.f * scale * d; dyo[i] = 2.f * scale * d; }
    }
    red[threadIdx.x] = a;
    __syncthreads();
    for (int m = SB / 2; m > 0; m >>= 1) {
        if ((int)threadIdx.x < m) red[threadIdx.x] += red[threadIdx.x + m];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0] * scale;
}

// head: pred = hseq_flat . w + b; squared error and d loss / d pred.  G: the family's geometry (B, E, T, o_lw, o_lb, w_sq, w_dpred)
template <typename G>
__global__ __launch_bounds__(SB) void sn_head_kernel(G g, const float* __restrict__ hseq, const float* __restrict__ prm, const float* __restrict__ y,
                                                     float* __restrict__ pred, float* __restrict__ ws, float inv_gb) {
    __shared__ float red[SB];
    const int n = g.E * g.T;
    for (int64_t b = blockIdx.x; b < g.B; b += gridDim.x) {
        float a = 0.f;
        for (int i = threadIdx.x; i < n; i += SB) a = fmaf(hseq[b * n + i], prm[g.o_lw + i], a);
        red[threadIdx.x] = a;
        __syncthreads();
        for (int m = SB / 2; m > 0; m >>= 1) {
            if ((int)threadIdx.x < m) red[threadIdx.x] += red[threadIdx.x + m];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            const float pr = red[0] + prm[g.o_lb];
            pred[b] = pr;
            if (y) {
                const float d = pr - y[b];
                ws[g.w_sq + b] = d * d * inv_gb;
                ws[g.w_dpred + b] = 2.f * d * inv_gb;
            }
        }
        __syncthreads();
    }
}

// d hseq[b][i] = dpred[b] w[i]
template <typename G>
__global__ void sn_head_bwd_kernel(G g, const float* __restrict__ dpred, const float* __restrict__ prm, float* __restrict__ dhs) {
    const int n = g.E * g.T;
    const int64_t tot = g.B * n;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < tot; i += (int64_t)gridDim.x * blockDim.x)
        dhs[i] = dpred[i / n] * prm[g.o_lw + i % n];
}

__global__ void sn_loss_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ loss) {
    if (threadIdx.x == 0 && blockIdx.x == 0) loss[0] = a[0] + b[0];
}

inline unsigned sn_grid(int64_t n) {
    int64_t b = (n + SB - 1) / SB;
    return (unsigned)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

}  // namespace

}  // namespace rulgnn
