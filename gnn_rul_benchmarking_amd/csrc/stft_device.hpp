// The STFT magnitude of one (sample, patch) in LDS: what the STFT front ends (STNet: stnet.hip, GDAGDL: gdagdl.hip, LOGO_bearing:
// logo.hip) share on the device.  Device-inline functions only; the arithmetic is stated here once.
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

}  // namespace

}  // namespace rulgnn
