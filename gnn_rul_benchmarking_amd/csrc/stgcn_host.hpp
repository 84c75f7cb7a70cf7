// Host-side launch geometry shared by the forward and training translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rulgnn.h"
#include "bn_cells.hpp"
#include "host_util.hpp"
#include "stgcn_device.hpp"

namespace rulgnn {

struct TileGeom {
    int RW;             // lanes per sample row: 16, 32 or 64
    int SPW;            // samples per wavefront
    int Ppad;           // LDS patch stride (floats): keeps per-lane patch reads bank-conflict free
    int vec4;           // tile copy may use 16-byte loads (given a 16-byte aligned x)
    int stage_floats;   // LDS staging floats per wavefront (multiple of 4)
    uint32_t magicP;    // ceil(2^32 / P) for fastdiv
    int64_t ntiles;     // wavefront tiles = ceil(batch / SPW)
};

[[nodiscard]] inline int validate_shape(const rulgnn_stgcn_shape* s) {
    if (!s) return RULGNN_EINVAL;
    if (s->batch < 0 || s->num_patch < 2 || s->patch_size < 2 || s->num_layers < 1) return RULGNN_EINVAL;
    if (s->mpnn_k < 1) return RULGNN_EINVAL;
    // MPNN order (Model.py:74-90): every wiring of the reference leaves the constructor default 1; 2 and 3 run on the row-mapped fp32
    // kernels (num_patch <= 64), not on the matrix-core or tiled ones
    if (s->mpnn_k > MAX_MPNN_ORDER || (s->mpnn_k > 1 && s->num_patch > 64)) return RULGNN_EUNSUPPORTED;
    if (s->num_patch > 4096 || s->num_layers > 8 || s->patch_size > 4096) return RULGNN_EUNSUPPORTED;
    if (s->batch > (int64_t)400000000 / ((int64_t)F * s->num_patch)) return RULGNN_EUNSUPPORTED;  // 32-bit dropout counter
    return RULGNN_OK;
}

[[nodiscard]] inline int tile_geometry(const rulgnn_stgcn_shape* s, TileGeom* g) {
    const int rc = validate_shape(s);
    if (rc != RULGNN_OK) return rc;
    const int N = s->num_patch, P = s->patch_size;
    if (N > 64) return RULGNN_EUNSUPPORTED;                 // fused row-mapped kernels; larger num_patch -> tiled path
    g->RW = N <= 16 ? 16 : (N <= 32 ? 32 : 64);
    g->SPW = 64 / g->RW;
    // even P: patches are read with ds_read_b64, conflict-free iff (stride/2) is odd.
    // odd P: ds_read_b32, conflict-free as stride is odd.
    g->Ppad = (P % 2 == 0 && (P / 2) % 2 == 0) ? P + 2 : P;
    g->vec4 = (g->Ppad == P) && (((int64_t)N * P) % 4 == 0);
    const int raw = g->SPW * N * g->Ppad;
    g->stage_floats = (raw + 3) & ~3;
    if (g->RW == 16 && g->stage_floats < PT_FLOATS) g->stage_floats = PT_FLOATS;   // the staging area doubles as the Pearson transpose tile
    if ((size_t)g->stage_floats * sizeof(float) > 36 * 1024) return RULGNN_EUNSUPPORTED;
    g->magicP = (uint32_t)((((uint64_t)1 << 32) + (uint64_t)P - 1) / (uint64_t)P);
    g->ntiles = (s->batch + g->SPW - 1) / g->SPW;
    return RULGNN_OK;
}

// Device-resident step state (include/rulgnn.h, RULGNN_STEP_STATE_BYTES): counters advanced on the device, plus what the
// compute kernels derive from them, so that a captured hipGraph replays with fresh dropout keys / Adam bias corrections.
struct StepState {
    uint64_t dropout_step;
    int64_t adam_step;
    float lr_over_bc1, inv_sqrt_bc2;
    uint32_t drop_key[8];
    uint32_t pad[2];
};
static_assert(sizeof(StepState) == RULGNN_STEP_STATE_BYTES, "step state layout");

// (seed, step, layer) -> 32-bit dropout key; bit-identical to oracle/stgcn_oracle.py::dropout_layer_key
__host__ __device__ inline uint64_t splitmix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__host__ __device__ inline uint32_t dropout_layer_key(uint64_t seed, uint64_t step, int layer) {
    return (uint32_t)(splitmix64(seed ^ splitmix64(step * 64 + (uint64_t)layer + 1)) & 0xFFFFFFFFull);
}

// Persistent grid: exactly as many workgroups as are co-resident (occupancy API x CU count), never
// more than there are tiles; workgroups grid-stride over wavefront tiles.  A grid larger than
// the resident set would run a second, mostly empty round (measured: 1024 blocks on 768 slots
// cost 1.5x).
// `oversub`: launch that many times the resident set so that the hardware dispatcher balances the tail
// (measured on the fused forward at 1M samples: x4 -> -10 %; it hurts the short training phases).
template <typename K>
inline int persistent_grid(K kernel, int64_t ntiles, size_t lds_bytes, int oversub = 1) {
    const Residency r = residency(kernel, BLOCK, lds_bytes);
    int64_t want = (ntiles + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    int64_t cap = (int64_t)r.cus * r.per_cu;
    if (oversub > 1 && want >= cap * oversub * 2) cap *= oversub;    // only when every wavefront still gets >= 8 tiles
    if (want > cap) want = cap;
    if (want < 1) want = 1;
    return (int)want;
}

// Eval-forward path selection (include/rulgnn.h: RULGNN_EVAL_*): AUTO = matrix-core kernel when the shape qualifies.
enum { STGCN_EVAL_AUTO = RULGNN_EVAL_AUTO, STGCN_EVAL_EXACT = RULGNN_EVAL_EXACT, STGCN_EVAL_MX = RULGNN_EVAL_MX };
[[nodiscard]] int stgcn_forward_eval(const rulgnn_stgcn_shape* s, const float* x, const float* prm, const float* bn, float* out,
                       hipStream_t stream, int path = STGCN_EVAL_AUTO);
// Matrix-core kernel (stgcn_forward_mx.hip); RULGNN_EUNSUPPORTED when the shape does not qualify (nothing launched).
// `taps`: optional debug buffer, MX_TAP_FLOATS floats (raw register dumps of the first tile, see the kernel).
[[nodiscard]] int stgcn_forward_eval_mx(const rulgnn_stgcn_shape* s, const float* x, const float* prm, const float* bn, float* out,
                          hipStream_t stream, float* taps = nullptr);
int stgcn_forward_mx_tap_floats();
// The matrix-core eval forward for 16 <= num_patch <= 47 (stgcn_forward_mx.hip) and the scanning launch that follows it: every
// non-finite prediction is recomputed by the exact row-mapped routine (stgcn_forward.hip).
[[nodiscard]] int stgcn_forward_eval_mxw(const rulgnn_stgcn_shape* s, const float* x, const float* prm, const float* bn, float* out, hipStream_t stream);
[[nodiscard]] int stgcn_forward_fixup(const rulgnn_stgcn_shape* s, const float* x, const float* prm, const float* bn, float* out, hipStream_t stream);
// Training phase F_0 on the matrix cores (stgcn_forward_mx.hip); RULGNN_EUNSUPPORTED when the shape is outside its rules
[[nodiscard]] int stgcn_train_f0_mx(const rulgnn_stgcn_shape* s, const float* x, const float* prm, float* cacheX, float* cacheA, float* H0, float* Z1,
                      double* cells_bn0, int cell_stride_doubles, int replicas, hipStream_t stream);
size_t stgcn_tiled_forward_workspace_bytes(const rulgnn_stgcn_shape* s);
[[nodiscard]] int stgcn_tiled_forward_eval(const rulgnn_stgcn_shape* s, const float* x, const float* prm, const float* bn, float* pred,
                             void* workspace, size_t workspace_bytes, hipStream_t stream);
size_t stgcn_tiled_train_workspace_bytes(const rulgnn_stgcn_shape* s);
// optional "these gradients are final" callback of the tiled training step (include/rulgnn.h: rulgnn_grad_ready_fn)
struct GradReadyHook {
    rulgnn_grad_ready_fn fn;
    void* user;
};
// (`sync` != nullptr, synchronised BatchNorm -- SyncHook, bn_cells.hpp: whole steps only, mode 2; the reduction pairs are 2 F doubles)
[[nodiscard]] int stgcn_tiled_train(const rulgnn_stgcn_shape* s, const rulgnn_stgcn_train_args* a, int mode, hipStream_t stream,
                      const GradReadyHook* ready = nullptr, const SyncHook* sync = nullptr);
size_t stgcn_train_workspace_bytes(const rulgnn_stgcn_shape* s);
// The LDS bytes a launch form of the fused row-mapped kernels requests at this shape (and MPNN order): the exact eval kernel, the scan
// behind the wide matrix-core eval kernel (order 1), the largest phase of the fp32 training chain; 0 where the row-mapped geometry does
// not apply.  Each is the `total` of the layout the kernels carve from and the launchers size their launches with (EvalWeightsLds,
// train_lds); the C-ABI gates (rulgnn_api.hip) compare them with MAX_LDS_BYTES (launch.hpp), so a shape the gates accept cannot fail a
// launcher's LDS check after an earlier launch of the same call has run.
size_t stgcn_forward_exact_lds_bytes(const rulgnn_stgcn_shape* s);
size_t stgcn_forward_fixup_lds_bytes(const rulgnn_stgcn_shape* s);
size_t stgcn_train_chain_lds_bytes(const rulgnn_stgcn_shape* s);
[[nodiscard]] int stgcn_train_forward(const rulgnn_stgcn_shape* s, const rulgnn_stgcn_train_args* a, hipStream_t stream);
[[nodiscard]] int stgcn_train_backward(const rulgnn_stgcn_shape* s, const rulgnn_stgcn_train_args* a, hipStream_t stream);
[[nodiscard]] int stgcn_train_fwdbwd(const rulgnn_stgcn_shape* s, const rulgnn_stgcn_train_args* a, hipStream_t stream);
[[nodiscard]] int stgcn_train_step(const rulgnn_stgcn_shape* s, const rulgnn_stgcn_train_args* a, const rulgnn_adam_args* opt,
                     hipStream_t stream, int path = RULGNN_STEP_AUTO);     // opt == nullptr: forward + backward only
[[nodiscard]] int stgcn_train_phase(const rulgnn_stgcn_shape* s, const rulgnn_stgcn_train_args* a, int phase, hipStream_t stream,
                      int path = RULGNN_STEP_AUTO);
[[nodiscard]] int stgcn_train_fwdbwd_syncbn(const rulgnn_stgcn_shape* s, const rulgnn_stgcn_train_args* a, const SyncHook* hook, hipStream_t stream,
                              int path = RULGNN_STEP_CHAIN);
int stgcn_train_mx_kind(const rulgnn_stgcn_shape* s, const float* x);        // 0 fp32 phases, 1 matrix-core chain, 2 wide matrix-core chain
int64_t stgcn_train_guard_counter_offset(const rulgnn_stgcn_shape* s);

}  // namespace rulgnn
