// The fp64 BatchNorm reduction cells every BatchNorm family shares, and what is computed from them.
//
// A kernel that reduces over the batch adds its per-workgroup (sum, sum of squares) -- or (sum dy, sum dy xhat) in backward -- with one
// atomic per channel.  With one workgroup per sample thousands of them hit the same addresses and serialise (~10 ns each), so the cells
// exist CELL_REP times: workgroup b adds into replica b % CELL_REP and every reader sums the replicas in ONE fixed order (replica_sum).
//
// The invariant synchronised BatchNorm rests on: sync_cells (families_host.hpp) sums the replicas of one reduction pair into replica 0
// in that same order and zeroes the others, so every reader's replica_sum is what it was before (v + 0.0 + ... + 0.0 is exact), and the
// caller's all-reduce on replica 0 turns it into the global batch's sum on every rank.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/rulgnn.h"

namespace rulgnn {

constexpr int CELL_REP = 16;

// one cell over its replicas, `stride_doubles` apart, replica 0 first
__device__ inline double replica_sum(const double* first, int stride_doubles) {
    double v = 0.0;
#pragma unroll
    for (int r = 0; r < CELL_REP; ++r) v += first[r * stride_doubles];
    return v;
}

// train mode: mean and biased variance of `count` values in fp64 from their (sum, sum of squares), clamped at 0, rounded to fp32 once each
struct BnMoments {
    float mean, var;
};
__device__ inline BnMoments bn_moments(double sum, double sumsq, double count) {
    const double m = sum / count;
    double v = sumsq / count - m * m;
    if (v < 0.0) v = 0.0;
    return {(float)m, (float)v};
}
// BatchNorm of one channel as scale / shift: y = z * sc + sh; xhat = (z - mean) * inv -- from bn_moments() in train mode, from the running
// statistics in eval mode.  (One coefficient function behind the choice of moments, not one per mode: a caller that loads gamma and beta
// itself then loads them once, behind the branch, as the kernels always did -- profiles/r14_bn_cells.md, section 1.)
struct BnCoef {
    float mean, inv, sc, sh;
};
__device__ inline BnCoef bn_coef(BnMoments s, float gamma, float beta, float eps) {
    BnCoef r;
    r.mean = s.mean;
    r.inv = 1.0f / sqrtf(s.var + eps);
    r.sc = gamma * r.inv;
    r.sh = beta - r.mean * r.sc;
    return r;
}

// batch statistics for the caller: (mean, biased var), or weight * (E z, E z^2) where ranks average their moments (weight > 0)
__device__ inline void bn_batch_out(double sum, double sumsq, double count, float weight, float* mean, float* var) {
    const double m = sum / count, q = sumsq / count;
    if (weight > 0.f) {
        *mean = (float)(weight * m);
        *var = (float)(weight * q);
    } else {
        const double v = q - m * m;
        *mean = (float)m;
        *var = (float)(v < 0.0 ? 0.0 : v);
    }
}

// nn.BatchNorm1d's running statistics from one batch's (mean, biased var) -- or (E z, E z^2) with `from_moments` -- of `count` values:
// the variance unbiased by a double-precision count / (count - 1), the momentum blend applied `times` times (ST_Conv runs every
// BatchNorm module twice per training forward)
__device__ inline void bn_running_blend(float* rm, float* rv, float mean, float var, double count, float momentum, int from_moments,
                                        int times) {
    if (from_moments) {
        var = var - mean * mean;
        if (var < 0.f) var = 0.f;
    }
    const float unbiased = count > 1.0 ? (float)(var * (count / (count - 1.0))) : var;
    float m = *rm, v = *rv;
    for (int k = 0; k < times; ++k) {
        m = (1.0f - momentum) * m + momentum * mean;
        v = (1.0f - momentum) * v + momentum * unbiased;
    }
    *rm = m;
    *rv = v;
}

// Synchronised BatchNorm hook of the *_fwdbwd_syncbn_* entries (include/rulgnn.h): behind every launch that completes a reduction pair,
// sync_cells collapses the pair and hands replica 0 to `fn` (the caller's all-reduce, in stream order).  `bn_param_grad_scale`: the
// cells then hold GLOBAL sums on every rank, and only that share of the BatchNorm gamma / beta gradients may enter the all-reduced bucket.
struct SyncHook {
    rulgnn_allreduce_f64_fn fn;
    void* user;
    float bn_param_grad_scale;
};

}  // namespace rulgnn
