// Probe for profiles/r28_logo_bearing.md: the STFT magnitude at LOGO_bearing's two geometries (batch 100 and 1024) as (a) a separate pass,
// one workgroup per (sample, patch), magnitude to HBM, and (b) the setup of lg_graph_fwd<true> / lg_graph_bwd<true> alone, one workgroup per
// sample walking its T patches into the LDS window.  Both on stft_device.hpp's functions; one JSON line per case.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/probe_stft_setup.hip -o tools/probe_stft_setup.bin && tools/probe_stft_setup.bin
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../gnn_rul_benchmarking_amd/csrc/stft_device.hpp"
using namespace rulgnn;
#define CK(e) do { hipError_t r_ = (e); if (r_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(r_), __LINE__); return 1; } } while (0)

__global__ __launch_bounds__(256) void sep_kernel(const float* __restrict__ x, float* __restrict__ mag, long G, int P, int ns, int N, int f) {
    extern __shared__ float sm[];
    const StftLds l = stft_carve(sm, P, ns);
    stft_tables(l, ns, threadIdx.x);
    for (long gi = blockIdx.x; gi < G; gi += gridDim.x) {
        __syncthreads();
        stft_load_patch(l, x + gi * P, P, ns, threadIdx.x);
        __syncthreads();
        for (int i = threadIdx.x; i < N * f; i += 256) mag[gi * N * f + i] = stft_magnitude(l, ns, i / f, i % f);
    }
}

__global__ __launch_bounds__(256) void fused_kernel(const float* __restrict__ x, float* __restrict__ out, long B, int T, int P, int ns, int N, int f) {
    extern __shared__ float sm[];
    const int L = T * f, XL = L + 1, tid = threadIdx.x;
    float* X = sm;
    const StftLds l = stft_carve(sm + N * XL, P, ns);
    stft_tables(l, ns, tid);
    for (long b = blockIdx.x; b < B; b += gridDim.x) {
        __syncthreads();
        for (int t = 0; t < T; ++t) {
            stft_load_patch(l, x + (b * T + t) * P, P, ns, tid);
            __syncthreads();
            for (int i = tid; i < N * f; i += 256) { const int n = i / f, j = i - n * f; X[n * XL + t * f + j] = stft_magnitude(l, ns, n, j); }
            __syncthreads();
        }
        float s = 0.f;
        for (int i = tid; i < N * L; i += 256) s += X[(i / L) * XL + i % L];
        out[b * 256 + tid] = s;
    }
}

static int run(long B, int T, int P, int ns) {
    const int N = ns / 2 + 1, f = 1 + P / ns;
    const long G = B * T;
    std::vector<float> hx((size_t)G * P);
    for (size_t i = 0; i < hx.size(); ++i) hx[i] = (float)((i * 2654435761u) % 1000) / 500.f - 1.f;
    float *x, *mag, *out;
    CK(hipMalloc(&x, hx.size() * 4)); CK(hipMalloc(&mag, (size_t)G * N * f * 4)); CK(hipMalloc(&out, (size_t)B * 256 * 4));
    CK(hipMemcpy(x, hx.data(), hx.size() * 4, hipMemcpyHostToDevice));
    const size_t lds_a = (size_t)(P + 4 * ns) * 4, lds_b = (size_t)(N * (T * f + 1) + P + 4 * ns) * 4;
    if (lds_b > 160 * 1024) { printf("does not fit\n"); return 1; }
    CK(hipFuncSetAttribute((const void*)fused_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_b));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const unsigned ga = (unsigned)(G > 65536 ? 65536 : G), gb = (unsigned)(B > 8192 ? 8192 : B);
    float ms_a = 0, ms_b = 0;
    const int reps = 20;
    for (int w = 0; w < 2; ++w) {
        CK(hipEventRecord(e0));
        for (int r = 0; r < reps; ++r) hipLaunchKernelGGL(sep_kernel, dim3(ga), dim3(256), lds_a, 0, x, mag, G, P, ns, N, f);
        CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); CK(hipEventElapsedTime(&ms_a, e0, e1));
        CK(hipEventRecord(e0));
        for (int r = 0; r < reps; ++r) hipLaunchKernelGGL(fused_kernel, dim3(gb), dim3(256), lds_b, 0, x, out, B, T, P, ns, N, f);
        CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); CK(hipEventElapsedTime(&ms_b, e0, e1));
        CK(hipGetLastError());
    }
    // the two forms computed the same magnitudes: per-sample sums agree
    std::vector<float> hm((size_t)N * f * T), ho(256);
    CK(hipMemcpy(hm.data(), mag, hm.size() * 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(ho.data(), out, 256 * 4, hipMemcpyDeviceToHost));
    double sa = 0, sb = 0; for (float v : hm) sa += v; for (float v : ho) sb += v;
    printf("{\"B\": %ld, \"T\": %d, \"P\": %d, \"nperseg\": %d, \"separate_pass_us\": %.1f, \"fused_setup_us\": %.1f, \"sum_sep\": %.4f, \"sum_fused\": %.4f}\n",
           B, T, P, ns, ms_a * 1000 / reps, ms_b * 1000 / reps, sa, sb);
    CK(hipFree(x)); CK(hipFree(mag)); CK(hipFree(out));
    return 0;
}

int main() {
    for (long B : {100L, 1024L}) { if (run(B, 40, 64, 8)) return 1; if (run(B, 32, 1024, 32)) return 1; }
    return 0;
}
