// extern "C" surface of librulgnn.so (declared in include/rulgnn.h).
#include <initializer_list>

#include "sgemm_mfma.hpp"
#include "families_host.hpp"
#include "adam_device.hpp"
#include "stgcn_train_mx.hpp"

using namespace rulgnn;

namespace rulgnn {
int& sgemm_big_mode() {
    static int mode = RULGNN_GEMM_BF16X3;
    return mode;
}
}  // namespace rulgnn

extern "C" {

int rulgnn_version(void) { return 100; }   // 0.1.0

const char* rulgnn_strerror(int code) {
    switch (code) {
        case RULGNN_OK: return "ok";
        case RULGNN_EINVAL: return "invalid argument (shape, null pointer or hyper-parameter)";
        case RULGNN_EUNSUPPORTED: return "shape not covered by the fused gfx950 kernels";
        case RULGNN_EWORKSPACE: return "workspace too small";
        case RULGNN_EHIP: return "HIP runtime error";
        case RULGNN_EALIGN: return "pointer not 4-byte aligned";
        case RULGNN_ECALLBACK: return "caller-supplied callback failed";
        default: return "unknown rulgnn error";
    }
}

int64_t rulgnn_stgcn_param_count(int32_t num_patch, int32_t num_layers) {
    if (num_patch < 1 || num_layers < 1) return -1;
    return param_count(num_patch, num_layers);
}
int64_t rulgnn_stgcn_param_count_order(int32_t num_patch, int32_t num_layers, int32_t mpnn_k) {
    if (num_patch < 1 || num_layers < 1 || mpnn_k < 1) return -1;
    return param_count(num_patch, num_layers, mpnn_k);
}

static int check_ptrs(std::initializer_list<const void*> ps) {
    for (const void* p : ps) {
        if (!p) return RULGNN_EINVAL;
        if (reinterpret_cast<uintptr_t>(p) & 3) return RULGNN_EALIGN;
    }
    return RULGNN_OK;
}

// An optional pointer: null, or 4-byte aligned.
static bool opt_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

// The pointer checks the plain families' steps end in, in two halves (a family with tests of its own between them calls the halves):
// parameters and workspace always, x and pred with a batch; for a backward the gradients and, with a batch, d pred or the targets.
// `a` is any family's args struct: the fields have the same names in all of them.
extern "C++" {
template <typename A>
static int check_fwd_ptrs(const A* a, int64_t batch) {
    RULGNN_TRY(check_ptrs({a->params, a->workspace}));
    return batch > 0 ? check_ptrs({a->x, a->pred}) : RULGNN_OK;
}
template <typename A>
static int check_bwd_ptrs(const A* a, int64_t batch) {
    RULGNN_TRY(check_ptrs({a->grads}));
    return !a->dpred && !a->y && batch > 0 ? RULGNN_EINVAL : RULGNN_OK;
}
template <typename A>
static int check_step_ptrs(const A* a, int64_t batch, bool bwd) {
    RULGNN_TRY(check_fwd_ptrs(a, batch));
    return bwd ? check_bwd_ptrs(a, batch) : RULGNN_OK;
}
}  // extern "C++"

// The optimizer block of a family's fused step (rulgnn_<family>_fwdbwd_f32): a step count or a device step state, the step's own
// parameter buffer, then the Adam pointers.
static int check_adam(const rulgnn_adam_args* opt, const float* params) {
    if ((opt->step < 1 && !opt->step_state) || opt->params != params) return RULGNN_EINVAL;
    return check_ptrs({opt->params, opt->exp_avg, opt->exp_avg_sq});
}

// Plain Adam over the flat floats [first, first + n) behind a family's step kernels.
static int adam_tail(const rulgnn_adam_args* opt, const float* grads, int64_t first, int64_t n, hipStream_t st) {
    return adam_step(opt->params + first, grads + first, opt->exp_avg + first, opt->exp_avg_sq + first, n, opt->step, opt->lr, opt->beta1,
                     opt->beta2, opt->eps, opt->weight_decay, 1.0f, st, opt->step_state);
}

// ---- the entries of a step family (families_host.hpp: StepFamily) -------------------------------------------------------------------
// Every rulgnn_<family>_{forward,backward,fwdbwd}_f32 is one of these on the family's description F: null structs are refused, then
// whatever F::check_args refuses (its shape_status first), then F::run is enqueued in mode 1, 2 or 3.
extern "C++" {
template <typename F>
static int step_check(const typename F::Shape* shape, const typename F::Args* args, bool fwd, bool bwd) {
    if (!shape || !args) return RULGNN_EINVAL;
    return F::check_args(shape, args, fwd, bwd);
}
template <typename F>
static int step_forward(const typename F::Shape* shape, const typename F::Args* args, void* stream) {
    RULGNN_TRY(step_check<F>(shape, args, true, false));
    return F::run(shape, args, 1, static_cast<hipStream_t>(stream));
}
template <typename F>
static int step_backward(const typename F::Shape* shape, const typename F::Args* args, void* stream) {
    RULGNN_TRY(step_check<F>(shape, args, false, true));
    return F::run(shape, args, 2, static_cast<hipStream_t>(stream));
}
// The fused call is the MSE step: d pred is refused, and so is a batch without targets.  With an optimizer block, plain Adam over the
// flat floats the family's description leaves live follows the step.
template <typename F>
static int step_fwdbwd(const typename F::Shape* shape, const typename F::Args* args, const rulgnn_adam_args* opt, void* stream) {
    RULGNN_TRY(step_check<F>(shape, args, true, true));
    if (args->dpred || (!args->y && shape->batch > 0)) return RULGNN_EINVAL;
    if (opt) RULGNN_TRY(check_adam(opt, args->params));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = F::run(shape, args, 3, st);
    if (rc != RULGNN_OK || !opt) return rc;
    const int64_t first = F::adam_first(shape);
    return adam_tail(opt, args->grads, first, F::param_count(shape) - first - F::adam_frozen_tail(shape), st);
}
// The fused call of `n` runs of one shape (rulgnn_<family>_fwdbwd_group_f32): groups[i] is run i's args, opts null or one block per run.
// Every group passes what step_fwdbwd checks and the workspace size run() would check, and no two groups may write the same buffers,
// all before F::run_group's first launch; Adam follows run by run.
template <typename F>
static int step_fwdbwd_group(const typename F::Shape* shape, const typename F::Args* groups, const rulgnn_adam_args* opts, int32_t n,
                             void* stream) {
    if (!shape || !groups || n < 1) return RULGNN_EINVAL;
    if (n > STEP_MAX_GROUPS) return RULGNN_EUNSUPPORTED;
    for (int32_t i = 0; i < n; ++i) {
        const typename F::Args* a = &groups[i];
        RULGNN_TRY(step_check<F>(shape, a, true, true));
        if (a->dpred || (!a->y && shape->batch > 0)) return RULGNN_EINVAL;
        if (a->workspace_bytes < F::workspace_bytes(shape)) return RULGNN_EWORKSPACE;
        if (opts) RULGNN_TRY(check_adam(&opts[i], a->params));
        for (int32_t j = 0; j < i; ++j)
            if (groups[j].workspace == a->workspace || groups[j].grads == a->grads || groups[j].params == a->params) return RULGNN_EINVAL;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    RULGNN_TRY(F::run_group(shape, groups, n, st));
    if (!opts) return RULGNN_OK;
    const int64_t first = F::adam_first(shape), count = F::param_count(shape) - first - F::adam_frozen_tail(shape);
    for (int32_t i = 0; i < n; ++i) RULGNN_TRY(adam_tail(&opts[i], groups[i].grads, first, count, st));
    return RULGNN_OK;
}
}  // extern "C++"

// The extern "C" entries of step family F under the prefix rulgnn_<name>_ (include/rulgnn.h declares each): the two queries and the
// three step calls, the fused one on the template `fwdbwd` (the BatchNorm families have their own below); _TAPS adds tap_offset.
#define STEP_FAMILY_ENTRIES_ON(name, F, fwdbwd)                                                                                             \
    int64_t rulgnn_##name##_param_count(const F::Shape* shape) { return F::param_count(shape); }                                            \
    size_t rulgnn_##name##_workspace_bytes(const F::Shape* shape) { return F::workspace_bytes(shape); }                                     \
    int rulgnn_##name##_forward_f32(const F::Shape* shape, const F::Args* args, void* stream) { return step_forward<F>(shape, args, stream); } \
    int rulgnn_##name##_backward_f32(const F::Shape* shape, const F::Args* args, void* stream) { return step_backward<F>(shape, args, stream); } \
    int rulgnn_##name##_fwdbwd_f32(const F::Shape* shape, const F::Args* args, const rulgnn_adam_args* opt, void* stream) {                 \
        return fwdbwd<F>(shape, args, opt, stream);                                                                                         \
    }
#define STEP_FAMILY_ENTRIES(name, F) STEP_FAMILY_ENTRIES_ON(name, F, step_fwdbwd)
#define STEP_FAMILY_ENTRIES_TAPS(name, F) \
    STEP_FAMILY_ENTRIES(name, F)          \
    int64_t rulgnn_##name##_tap_offset(const F::Shape* shape, int32_t which) { return F::tap_offset(shape, which); }
// The grouped fused step of a family whose description has run_group.
#define STEP_FAMILY_GROUP_ENTRY(name, F)                                                                                                    \
    int rulgnn_##name##_fwdbwd_group_f32(const F::Shape* shape, const F::Args* groups, const rulgnn_adam_args* opts, int32_t num_groups,    \
                                         void* stream) {                                                                                    \
        return step_fwdbwd_group<F>(shape, groups, opts, num_groups, stream);                                                               \
    }
int32_t rulgnn_step_max_groups(void) { return STEP_MAX_GROUPS; }

// Path selection.  The fused row-mapped kernels cover num_patch <= 64 as long as one wavefront's input tile fits its LDS staging area,
// every launch form a call may reach fits the 160 KB of LDS a workgroup can have (stgcn_host.hpp: the *_lds_bytes functions the
// launchers size their launches with) and, for training, num_layers <= 3 / <= 2; everything else valid goes to the tiled path, which has
// no such limits.  Deciding it here, before anything is launched, is what makes a refusal (RULGNN_EUNSUPPORTED) leave every buffer as
// it was.
static bool tiled_eval(const rulgnn_stgcn_shape* shape) {
    TileGeom g;
    return tile_geometry(shape, &g) != RULGNN_OK || stgcn_forward_exact_lds_bytes(shape) > MAX_LDS_BYTES;
}
static bool tiled(const rulgnn_stgcn_shape* shape) { return stgcn_train_workspace_bytes(shape) == 0; }

// MPNN order k > 1 exists on the fused row-mapped kernels only: a shape they cannot hold (a window beyond a wavefront's LDS staging area,
// weights + tiles beyond the workgroup's LDS, more layers than the phase chain is instantiated for) must NOT fall through to the tiled
// kernels, which read the order-1 layout: it is refused up front.
static bool order_needs_tiled(const rulgnn_stgcn_shape* shape, bool train) {
    return shape->mpnn_k != 1 && (train ? tiled(shape) : tiled_eval(shape));
}

size_t rulgnn_stgcn_forward_workspace_bytes(const rulgnn_stgcn_shape* shape) {
    if (validate_shape(shape) != RULGNN_OK || order_needs_tiled(shape, false)) return 0;
    return tiled_eval(shape) ? stgcn_tiled_forward_workspace_bytes(shape) : 0;
}

int rulgnn_stgcn_forward_path_f32(const rulgnn_stgcn_shape* shape, const float* x, const float* params,
                                  const float* bn_stats, float* pred, void* workspace, size_t workspace_bytes,
                                  int path, void* stream) {
    int rc = validate_shape(shape);
    if (rc != RULGNN_OK) return rc;
    if (path != RULGNN_EVAL_AUTO && path != RULGNN_EVAL_EXACT && path != RULGNN_EVAL_MX) return RULGNN_EINVAL;
    if (order_needs_tiled(shape, false)) return RULGNN_EUNSUPPORTED;
    if (shape->batch == 0) return RULGNN_OK;
    rc = check_ptrs({x, params, bn_stats, pred});
    if (rc != RULGNN_OK) return rc;
    if (tiled_eval(shape))
        return stgcn_tiled_forward_eval(shape, x, params, bn_stats, pred, workspace, workspace_bytes,
                                        static_cast<hipStream_t>(stream));
    return stgcn_forward_eval(shape, x, params, bn_stats, pred, static_cast<hipStream_t>(stream), path);
}

int rulgnn_stgcn_forward_f32(const rulgnn_stgcn_shape* shape, const float* x, const float* params,
                             const float* bn_stats, float* pred, void* workspace, size_t workspace_bytes,
                             void* stream) {
    return rulgnn_stgcn_forward_path_f32(shape, x, params, bn_stats, pred, workspace, workspace_bytes, RULGNN_EVAL_AUTO, stream);
}

int rulgnn_stgcn_forward_mx_tap_floats(void) { return stgcn_forward_mx_tap_floats(); }

int rulgnn_stgcn_forward_mx_taps_f32(const rulgnn_stgcn_shape* shape, const float* x, const float* params,
                                     const float* bn_stats, float* pred, float* taps, void* stream) {
    int rc = validate_shape(shape);
    if (rc != RULGNN_OK) return rc;
    rc = check_ptrs({x, params, bn_stats, pred, taps});
    if (rc != RULGNN_OK) return rc;
    return stgcn_forward_eval_mx(shape, x, params, bn_stats, pred, static_cast<hipStream_t>(stream), taps);
}

static size_t train_ws_bytes(const rulgnn_stgcn_shape* shape) {
    if (order_needs_tiled(shape, true)) return 0;
    return tiled(shape) ? stgcn_tiled_train_workspace_bytes(shape) : stgcn_train_workspace_bytes(shape);
}

size_t rulgnn_stgcn_train_workspace_bytes(const rulgnn_stgcn_shape* shape) {
    if (validate_shape(shape) != RULGNN_OK) return 0;
    return train_ws_bytes(shape);
}

static int check_train(const rulgnn_stgcn_shape* shape, const rulgnn_stgcn_train_args* a, bool need_grads) {
    int rc = validate_shape(shape);
    if (rc != RULGNN_OK) return rc;
    if (!a) return RULGNN_EINVAL;
    if (shape->batch < 1) return RULGNN_EINVAL;                 // BatchNorm needs a batch
    if (a->global_batch < shape->batch || a->sample_offset < 0) return RULGNN_EINVAL;
    if (!(a->dropout_p >= 0.f && a->dropout_p < 1.f)) return RULGNN_EINVAL;
    if (!(a->bn_moment_weight >= 0.f)) return RULGNN_EINVAL;
    rc = check_ptrs({a->x, a->params, a->pred, a->bn_batch, a->workspace});
    if (rc != RULGNN_OK) return rc;
    if (need_grads) {
        rc = check_ptrs({a->grads});
        if (rc != RULGNN_OK) return rc;
        if (!a->dpred) {
            rc = check_ptrs({a->y, a->loss});
            if (rc != RULGNN_OK) return rc;
        } else if (!opt_aligned(a->dpred)) {
            return RULGNN_EALIGN;
        }
    }
    const size_t need = train_ws_bytes(shape);
    if (need == 0) return RULGNN_EUNSUPPORTED;
    if (a->workspace_bytes < need) return RULGNN_EWORKSPACE;
    return RULGNN_OK;
}

int rulgnn_stgcn_train_forward_f32(const rulgnn_stgcn_shape* shape, const rulgnn_stgcn_train_args* args, void* stream) {
    const int rc = check_train(shape, args, false);
    if (rc != RULGNN_OK) return rc;
    if (tiled(shape)) return stgcn_tiled_train(shape, args, 0, static_cast<hipStream_t>(stream));
    return stgcn_train_forward(shape, args, static_cast<hipStream_t>(stream));
}

int rulgnn_stgcn_train_backward_f32(const rulgnn_stgcn_shape* shape, const rulgnn_stgcn_train_args* args, void* stream) {
    const int rc = check_train(shape, args, true);
    if (rc != RULGNN_OK) return rc;
    if (tiled(shape)) return stgcn_tiled_train(shape, args, 1, static_cast<hipStream_t>(stream));
    return stgcn_train_backward(shape, args, static_cast<hipStream_t>(stream));
}

int rulgnn_stgcn_train_fwdbwd_f32(const rulgnn_stgcn_shape* shape, const rulgnn_stgcn_train_args* args, void* stream) {
    const int rc = check_train(shape, args, true);
    if (rc != RULGNN_OK) return rc;
    if (tiled(shape)) return stgcn_tiled_train(shape, args, 2, static_cast<hipStream_t>(stream));
    return stgcn_train_fwdbwd(shape, args, static_cast<hipStream_t>(stream));
}

int rulgnn_stgcn_train_fwdbwd_ready_f32(const rulgnn_stgcn_shape* shape, const rulgnn_stgcn_train_args* args, rulgnn_grad_ready_fn ready,
                                        void* user, void* stream) {
    const int rc = check_train(shape, args, true);
    if (rc != RULGNN_OK) return rc;
    if (!ready) return RULGNN_EINVAL;
    if (tiled(shape)) {
        const GradReadyHook hook = {ready, user};
        return stgcn_tiled_train(shape, args, 2, static_cast<hipStream_t>(stream), &hook);
    }
    return stgcn_train_fwdbwd(shape, args, static_cast<hipStream_t>(stream));     // buckets of a few KB: nothing to overlap
}

// What every synchronised-BatchNorm entry refuses in its own arguments: a share of the BatchNorm parameter gradients outside [0, 1], no
// all-reduce, averaged moments (the cells hold the global batch's sums already).  (ASTGCNN and FC_STGNN leave the moment weight to their
// drivers, which refuse it behind their geometry check.)
static int check_sync(float bn_param_grad_scale, rulgnn_allreduce_f64_fn allreduce, float bn_moment_weight = 0.f) {
    if (!(bn_param_grad_scale >= 0.f && bn_param_grad_scale <= 1.f) || !allreduce || bn_moment_weight != 0.f) return RULGNN_EINVAL;
    return RULGNN_OK;
}

// the ST_GCN step under `sync` on the launch form the shape takes
static int stgcn_sync_step(const rulgnn_stgcn_shape* shape, const rulgnn_stgcn_train_args* args, const SyncHook& sync, const GradReadyHook* ready,
                           int path, void* stream) {
    if (tiled(shape)) return stgcn_tiled_train(shape, args, 2, static_cast<hipStream_t>(stream), ready, &sync);
    return stgcn_train_fwdbwd_syncbn(shape, args, &sync, static_cast<hipStream_t>(stream), path);
}

int rulgnn_stgcn_train_fwdbwd_syncbn_f32(const rulgnn_stgcn_shape* shape, const rulgnn_stgcn_train_args* args,
                                         float bn_param_grad_scale, rulgnn_allreduce_f64_fn allreduce, void* user, void* stream) {
    const int rc = check_train(shape, args, true);
    if (rc != RULGNN_OK) return rc;
    RULGNN_TRY(check_sync(bn_param_grad_scale, allreduce, args->bn_moment_weight));
    return stgcn_sync_step(shape, args, {allreduce, user, bn_param_grad_scale}, nullptr, RULGNN_STEP_CHAIN, stream);
}

int rulgnn_stgcn_train_fwdbwd_syncbn_ready_f32(const rulgnn_stgcn_shape* shape, const rulgnn_stgcn_train_args* args,
                                               float bn_param_grad_scale, rulgnn_allreduce_f64_fn allreduce, void* user,
                                               rulgnn_grad_ready_fn ready, void* ready_user, void* stream) {
    const int rc = check_train(shape, args, true);
    if (rc != RULGNN_OK) return rc;
    RULGNN_TRY(check_sync(bn_param_grad_scale, allreduce, args->bn_moment_weight));
    if (!ready) return RULGNN_EINVAL;
    // (num_patch <= 64, buckets of a few KB: nothing to overlap, no region is reported -- as rulgnn_stgcn_train_fwdbwd_ready_f32 there)
    const GradReadyHook hook = {ready, ready_user};
    return stgcn_sync_step(shape, args, {allreduce, user, bn_param_grad_scale}, &hook, RULGNN_STEP_CHAIN, stream);
}

int rulgnn_stgcn_train_fwdbwd_syncbn_path_f32(const rulgnn_stgcn_shape* shape, const rulgnn_stgcn_train_args* args,
                                              float bn_param_grad_scale, rulgnn_allreduce_f64_fn allreduce, void* user, int32_t path,
                                              void* stream) {
    const int rc = check_train(shape, args, true);
    if (rc != RULGNN_OK) return rc;
    RULGNN_TRY(check_sync(bn_param_grad_scale, allreduce, args->bn_moment_weight));
    if (path != RULGNN_STEP_AUTO && path != RULGNN_STEP_CHAIN && path != RULGNN_STEP_MX) return RULGNN_EINVAL;
    // (num_patch > 64 has one launch form: `path` is ignored there, as by rulgnn_stgcn_train_step_path_f32)
    return stgcn_sync_step(shape, args, {allreduce, user, bn_param_grad_scale}, nullptr, path, stream);
}

int64_t rulgnn_stgcn_train_guard_counter_offset(const rulgnn_stgcn_shape* shape) {
    if (validate_shape(shape) != RULGNN_OK) return -1;
    return tiled(shape) ? -1 : stgcn_train_guard_counter_offset(shape);
}

size_t rulgnn_stgcn_train_args_size(void) { return sizeof(rulgnn_stgcn_train_args); }

size_t rulgnn_struct_size(int32_t which) {
    switch (which) {
    case RULGNN_STRUCT_STGCN_SHAPE: return sizeof(rulgnn_stgcn_shape);
    case RULGNN_STRUCT_STGCN_TRAIN_ARGS: return sizeof(rulgnn_stgcn_train_args);
    case RULGNN_STRUCT_ADAM_ARGS: return sizeof(rulgnn_adam_args);
    case RULGNN_STRUCT_STMSGCN_SHAPE: return sizeof(rulgnn_stmsgcn_shape);
    case RULGNN_STRUCT_STMSGCN_ARGS: return sizeof(rulgnn_stmsgcn_args);
    case RULGNN_STRUCT_ASTGCNN_SHAPE: return sizeof(rulgnn_astgcnn_shape);
    case RULGNN_STRUCT_ASTGCNN_ARGS: return sizeof(rulgnn_astgcnn_args);
    case RULGNN_STRUCT_FCSTGNN_SHAPE: return sizeof(rulgnn_fcstgnn_shape);
    case RULGNN_STRUCT_FCSTGNN_ARGS: return sizeof(rulgnn_fcstgnn_args);
    case RULGNN_STRUCT_RGCNU_SHAPE: return sizeof(rulgnn_rgcnu_shape);
    case RULGNN_STRUCT_RGCNU_ARGS: return sizeof(rulgnn_rgcnu_args);
    case RULGNN_STRUCT_STNET_SHAPE: return sizeof(rulgnn_stnet_shape);
    case RULGNN_STRUCT_STNET_ARGS: return sizeof(rulgnn_stnet_args);
    case RULGNN_STRUCT_SAGCN_SHAPE: return sizeof(rulgnn_sagcn_shape);
    case RULGNN_STRUCT_SAGCN_ARGS: return sizeof(rulgnn_sagcn_args);
    case RULGNN_STRUCT_STAGNN_SHAPE: return sizeof(rulgnn_stagnn_shape);
    case RULGNN_STRUCT_STAGNN_ARGS: return sizeof(rulgnn_stagnn_args);
    case RULGNN_STRUCT_HAGCN_SHAPE: return sizeof(rulgnn_hagcn_shape);
    case RULGNN_STRUCT_HAGCN_ARGS: return sizeof(rulgnn_hagcn_args);
    case RULGNN_STRUCT_BILSTM_SHAPE: return sizeof(rulgnn_bilstm_shape);
    case RULGNN_STRUCT_BILSTM_ARGS: return sizeof(rulgnn_bilstm_args);
    case RULGNN_STRUCT_STCONV_SHAPE: return sizeof(rulgnn_stconv_shape);
    case RULGNN_STRUCT_STGNN_SHAPE: return sizeof(rulgnn_stgnn_shape);
    case RULGNN_STRUCT_GRU_SHAPE: return sizeof(rulgnn_gru_shape);
    case RULGNN_STRUCT_GRU_ARGS: return sizeof(rulgnn_gru_args);
    case RULGNN_STRUCT_GRUCM_SHAPE: return sizeof(rulgnn_grucm_shape);
    case RULGNN_STRUCT_GRUCM_ARGS: return sizeof(rulgnn_grucm_args);
    case RULGNN_STRUCT_AGCNTF_SHAPE: return sizeof(rulgnn_agcntf_shape);
    case RULGNN_STRUCT_AGCNTF_ARGS: return sizeof(rulgnn_agcntf_args);
    case RULGNN_STRUCT_HIERCORRPOOL_SHAPE: return sizeof(rulgnn_hiercorrpool_shape);
    case RULGNN_STRUCT_HIERCORRPOOL_ARGS: return sizeof(rulgnn_hiercorrpool_args);
    case RULGNN_STRUCT_LOGO_SHAPE: return sizeof(rulgnn_logo_shape);
    case RULGNN_STRUCT_LOGO_ARGS: return sizeof(rulgnn_logo_args);
    case RULGNN_STRUCT_DVGTFORMER_SHAPE: return sizeof(rulgnn_dvgtformer_shape);
    case RULGNN_STRUCT_DVGTFORMER_ARGS: return sizeof(rulgnn_dvgtformer_args);
    case RULGNN_STRUCT_GDAGDL_SHAPE: return sizeof(rulgnn_gdagdl_shape);
    case RULGNN_STRUCT_GDAGDL_ARGS: return sizeof(rulgnn_gdagdl_args);
    case RULGNN_STRUCT_GATLSTM_SHAPE: return sizeof(rulgnn_gatlstm_shape);
    case RULGNN_STRUCT_GATLSTM_ARGS: return sizeof(rulgnn_gatlstm_args);
    case RULGNN_STRUCT_LOGOB_SHAPE: return sizeof(rulgnn_logob_shape);
    case RULGNN_STRUCT_HCPB_SHAPE: return sizeof(rulgnn_hcpb_shape);
    case RULGNN_STRUCT_STFA_SHAPE: return sizeof(rulgnn_stfa_shape);
    case RULGNN_STRUCT_STFA_ARGS: return sizeof(rulgnn_stfa_args);
    default: return 0;
    }
}

int rulgnn_stgcn_train_step_f32(const rulgnn_stgcn_shape* shape, const rulgnn_stgcn_train_args* args,
                                const rulgnn_adam_args* opt, void* stream) {
    if (!opt) return RULGNN_EINVAL;
    return rulgnn_stgcn_train_step_path_f32(shape, args, opt, RULGNN_STEP_AUTO, stream);
}

int rulgnn_stgcn_train_step_path_f32(const rulgnn_stgcn_shape* shape, const rulgnn_stgcn_train_args* args,
                                     const rulgnn_adam_args* opt, int32_t path, void* stream) {
    int rc = check_train(shape, args, true);
    if (rc != RULGNN_OK) return rc;
    if (path != RULGNN_STEP_AUTO && path != RULGNN_STEP_CHAIN && path != RULGNN_STEP_COOP && path != RULGNN_STEP_MX && path != RULGNN_STEP_MX_PERSIST)
        return RULGNN_EINVAL;
    if (!opt) {                                            // forward + backward only
        if (tiled(shape)) return stgcn_tiled_train(shape, args, 2, static_cast<hipStream_t>(stream));
        return stgcn_train_step(shape, args, nullptr, static_cast<hipStream_t>(stream), path);
    }
    if (args->dpred) return RULGNN_EINVAL;
    rc = check_adam(opt, args->params);
    if (rc != RULGNN_OK) return rc;
    if (!opt_aligned(opt->bn_stats)) return RULGNN_EALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (tiled(shape)) {                                    // tiled path: same call, optimizer (+ running statistics) as one more kernel
        rc = stgcn_tiled_train(shape, args, 2, st);
        if (rc != RULGNN_OK) return rc;
        if (opt->bn_stats && !opt->step_state)
            return adam_bn_step(opt->params, args->grads, opt->exp_avg, opt->exp_avg_sq, param_count(shape->num_patch, shape->num_layers),
                                opt->step, opt->lr, opt->beta1, opt->beta2, opt->eps, opt->weight_decay, 1.0f, opt->bn_stats, args->bn_batch,
                                shape->num_layers, shape->batch * (int64_t)shape->num_patch, opt->bn_momentum,
                                args->bn_moment_weight > 0.f ? 1 : 0, nullptr, st);
        rc = adam_step(opt->params, args->grads, opt->exp_avg, opt->exp_avg_sq,
                       param_count(shape->num_patch, shape->num_layers), opt->step, opt->lr, opt->beta1, opt->beta2, opt->eps,
                       opt->weight_decay, 1.0f, st, opt->step_state);
        if (rc != RULGNN_OK || !opt->bn_stats) return rc;
        return bn_running_update(opt->bn_stats, args->bn_batch, shape->num_layers, shape->batch * (int64_t)shape->num_patch,
                                 opt->bn_momentum, args->bn_moment_weight > 0.f ? 1 : 0, st);
    }
    return stgcn_train_step(shape, args, opt, st, path);
}

int rulgnn_stgcn_train_step_resolve(const rulgnn_stgcn_shape* shape, const float* x, int32_t path) {
    const int rc = validate_shape(shape);
    if (rc != RULGNN_OK) return rc;
    if (tiled(shape)) return RULGNN_EUNSUPPORTED;
    if (path == RULGNN_STEP_COOP && shape->mpnn_k != 1) return RULGNN_EUNSUPPORTED;      // the single launch is built for order 1
    if (path == RULGNN_STEP_CHAIN || path == RULGNN_STEP_COOP) return path;
    if (path != RULGNN_STEP_AUTO && path != RULGNN_STEP_MX && path != RULGNN_STEP_MX_PERSIST) return RULGNN_EINVAL;
    const int kind = stgcn_train_mx_kind(shape, x);
    if (path == RULGNN_STEP_MX_PERSIST)          // the small-batch single launch: the 4-sample-tile chain, two layers, a workgroup per CU
        return kind == 1 && stgcn_train_mx_persistent_grid(shape->batch, shape->num_layers, 2048) > 0 ? RULGNN_STEP_MX : RULGNN_EUNSUPPORTED;
    if (kind != 0) return RULGNN_STEP_MX;
    return path != RULGNN_STEP_AUTO ? RULGNN_EUNSUPPORTED : RULGNN_STEP_CHAIN;
}

int rulgnn_stgcn_train_phase_count(int32_t num_layers) { return num_layers >= 1 ? 4 * num_layers + 1 : -1; }

int rulgnn_stgcn_train_phase_f32(const rulgnn_stgcn_shape* shape, const rulgnn_stgcn_train_args* args, int32_t phase,
                                 void* stream) {
    const int rc = check_train(shape, args, true);
    if (rc != RULGNN_OK) return rc;
    if (tiled(shape)) return RULGNN_EUNSUPPORTED;          // the tiled path is not a phase chain
    return stgcn_train_phase(shape, args, phase, static_cast<hipStream_t>(stream));
}

int rulgnn_adam_step_f32(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, int64_t step,
                         float lr, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                         void* stream) {
    if (n < 0 || step < 1) return RULGNN_EINVAL;
    const int rc = check_ptrs({params, grads, exp_avg, exp_avg_sq});
    if (rc != RULGNN_OK) return rc;
    return adam_step(params, grads, exp_avg, exp_avg_sq, n, step, lr, beta1, beta2, eps, weight_decay, grad_scale,
                     static_cast<hipStream_t>(stream));
}

int rulgnn_adam_step_guarded_f32(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, int64_t step,
                                 float lr, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                                 const float* guard, void* stream) {
    if (n < 0 || step < 1) return RULGNN_EINVAL;
    const int rc = check_ptrs({params, grads, exp_avg, exp_avg_sq, guard});
    if (rc != RULGNN_OK) return rc;
    return adam_step(params, grads, exp_avg, exp_avg_sq, n, step, lr, beta1, beta2, eps, weight_decay, grad_scale,
                     static_cast<hipStream_t>(stream), nullptr, guard);
}

int rulgnn_bn_running_update_guarded_f32(float* bn_stats, const float* bn_batch, int32_t num_layers, int64_t count,
                                         float momentum, int32_t from_moments, const float* guard, void* stream) {
    if (num_layers < 1 || num_layers > 8 || count < 1) return RULGNN_EINVAL;
    const int rc = check_ptrs({bn_stats, bn_batch, guard});
    if (rc != RULGNN_OK) return rc;
    return bn_running_update(bn_stats, bn_batch, num_layers, count, momentum, from_moments, static_cast<hipStream_t>(stream), guard);
}

int rulgnn_adam_bn_step_f32(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, int64_t step, float lr,
                            float beta1, float beta2, float eps, float weight_decay, float grad_scale, float* bn_stats,
                            const float* bn_batch, int32_t num_layers, int64_t count, float momentum, int32_t from_moments,
                            const float* guard, void* stream) {
    if (n < 0 || step < 1 || num_layers < 1 || num_layers > 8 || count < 1) return RULGNN_EINVAL;
    const int rc = check_ptrs({params, grads, exp_avg, exp_avg_sq, bn_stats, bn_batch});
    if (rc != RULGNN_OK) return rc;
    return adam_bn_step(params, grads, exp_avg, exp_avg_sq, n, step, lr, beta1, beta2, eps, weight_decay, grad_scale, bn_stats,
                        bn_batch, num_layers, count, momentum, from_moments, guard, static_cast<hipStream_t>(stream));
}

int rulgnn_bn_running_update_f32(float* bn_stats, const float* bn_batch, int32_t num_layers, int64_t count,
                                 float momentum, int32_t from_moments, void* stream) {
    if (num_layers < 1 || num_layers > 8 || count < 1) return RULGNN_EINVAL;
    const int rc = check_ptrs({bn_stats, bn_batch});
    if (rc != RULGNN_OK) return rc;
    return bn_running_update(bn_stats, bn_batch, num_layers, count, momentum, from_moments, static_cast<hipStream_t>(stream));
}


// ---- STMSGCN ------------------------------------------------------------------------------------------
int rulgnn_stmsgcn_features_f32(const rulgnn_stmsgcn_shape* shape, const float* x, const float* params, float* features,
                                void* stream) {
    if (!shape) return RULGNN_EINVAL;
    if (Stmsgcn::param_count(shape) >= 0 && shape->batch == 0) return RULGNN_OK;
    const int rc = check_ptrs({x, params, features});
    if (rc != RULGNN_OK) return rc;
    return stmsgcn_features(shape, x, params, features, static_cast<hipStream_t>(stream));
}

// (the shape is judged by run(), behind this)
int Stmsgcn::check_args(const Shape* shape, const Args* a, bool, bool bwd) {
    if (shape->batch < 1 || a->global_batch < shape->batch) return RULGNN_EINVAL;
    RULGNN_TRY(check_ptrs({a->x, a->params, a->pred, a->workspace}));
    if (!opt_aligned(a->y)) return RULGNN_EALIGN;
    if (!bwd) return RULGNN_OK;
    RULGNN_TRY(check_ptrs({a->grads}));
    if (a->dpred) return opt_aligned(a->dpred) ? RULGNN_OK : RULGNN_EALIGN;
    return check_ptrs({a->y, a->loss});
}

STEP_FAMILY_ENTRIES(stmsgcn, Stmsgcn)

// ---- the BatchNorm families: ASTGCNN, FC_STGNN, ST_Conv ---------------------------------------------------------------------------------
// Their shared argument check (the args structs have these fields under the same names).  The shape is judged by run(), behind it.
extern "C++" {
template <typename A>
static int check_bn_args(int64_t batch, const A* a, bool fwd, bool bwd) {
    if (batch < 1 || a->global_batch < batch) return RULGNN_EINVAL;          // BatchNorm needs a batch
    if (!(a->bn_moment_weight >= 0.f)) return RULGNN_EINVAL;
    RULGNN_TRY(check_ptrs({a->x, a->params, a->pred, a->workspace}));
    if (fwd && !a->training) RULGNN_TRY(check_ptrs({a->bn_stats}));
    for (const void* p : {(const void*)a->y, (const void*)a->dpred, (const void*)a->bn_batch, (const void*)a->loss})
        if (!opt_aligned(p)) return RULGNN_EALIGN;
    if (!bwd) return RULGNN_OK;
    if (!a->training) return RULGNN_EINVAL;            // the backward is the train-mode (batch-statistics) one
    RULGNN_TRY(check_ptrs({a->grads}));
    return a->dpred ? RULGNN_OK : check_ptrs({a->y, a->loss});
}

// Their fused MSE step.  With an optimizer block, Adam and the running-statistics update follow the step -- inside it where the
// family's run() takes them (F::run_takes_optimizer), as launches behind it otherwise.
template <typename F>
static int bn_step_fwdbwd(const typename F::Shape* shape, const typename F::Args* args, const rulgnn_adam_args* opt, void* stream) {
    RULGNN_TRY(step_check<F>(shape, args, true, true));
    if (args->dpred) return RULGNN_EINVAL;
    if (opt) RULGNN_TRY(check_adam(opt, args->params));
    if (opt && opt->bn_stats && (!args->bn_batch || !opt_aligned(opt->bn_stats))) return RULGNN_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    bool bn_in_step = false, adam_in_step = false;
    int rc;
    if constexpr (F::run_takes_optimizer) {
        // (plain batch statistics: the running-statistics update rides in the step)
        bn_in_step = opt && opt->bn_stats && args->training && args->bn_moment_weight == 0.f;
        // (host-side step count: the step's last kernel may apply the optimizer itself -- adam_device.hpp; a device step state keeps the
        // launch.  run() leaves fuse.gbase set where it did.)
        AdamFuse fuse{};
        const bool try_fuse = opt && !opt->step_state;
        if (try_fuse)
            adam_fuse_args(&fuse, opt->params, opt->exp_avg, opt->exp_avg_sq, args->grads, opt->step, opt->lr, opt->beta1, opt->beta2, opt->eps,
                           opt->weight_decay);
        rc = F::run(shape, args, 3, st, nullptr, bn_in_step ? opt->bn_stats : nullptr, bn_in_step ? opt->bn_momentum : 0.f, try_fuse ? &fuse : nullptr);
        adam_in_step = try_fuse && fuse.gbase;
    } else {
        rc = F::run(shape, args, 3, st);
    }
    if (rc != RULGNN_OK || !opt) return rc;
    if (!adam_in_step) rc = adam_tail(opt, args->grads, 0, F::param_count(shape), st);
    if (rc != RULGNN_OK || !opt->bn_stats || bn_in_step) return rc;
    return F::step_bn_update(shape, opt->bn_stats, args->bn_batch, opt->bn_momentum, args->bn_moment_weight > 0.f ? 1 : 0, st);
}

// The same step under synchronised BatchNorm (rulgnn_<family>_fwdbwd_syncbn_f32).
template <typename F>
static int bn_step_syncbn(const typename F::Shape* shape, const typename F::Args* args, float bn_param_grad_scale, rulgnn_allreduce_f64_fn allreduce,
                          void* user, void* stream) {
    RULGNN_TRY(step_check<F>(shape, args, true, true));
    if (args->dpred) return RULGNN_EINVAL;
    RULGNN_TRY(check_sync(bn_param_grad_scale, allreduce));
    const SyncHook hook = {allreduce, user, bn_param_grad_scale};
    return F::run(shape, args, 3, static_cast<hipStream_t>(stream), &hook);
}
}  // extern "C++"

// What the rulgnn_<family>_bn_running_update_f32 entries refuse (FC_STGNN's has no count: its shape holds it).
static int check_bn_update(const void* shape, const float* bn_stats, const float* bn_batch, int64_t count = 1) {
    if (!shape || count < 1) return RULGNN_EINVAL;
    return check_ptrs({bn_stats, bn_batch});
}

// ---- ASTGCNN ------------------------------------------------------------------------------------------
int Astgcnn::check_args(const Shape* shape, const Args* a, bool fwd, bool bwd) { return check_bn_args(shape->batch, a, fwd, bwd); }

STEP_FAMILY_ENTRIES_ON(astgcnn, Astgcnn, bn_step_fwdbwd)
int rulgnn_astgcnn_fwdbwd_syncbn_f32(const rulgnn_astgcnn_shape* shape, const rulgnn_astgcnn_args* args, float bn_param_grad_scale,
                                     rulgnn_allreduce_f64_fn allreduce, void* user, void* stream) {
    return bn_step_syncbn<Astgcnn>(shape, args, bn_param_grad_scale, allreduce, user, stream);
}
int rulgnn_astgcnn_bn_running_update_f32(const rulgnn_astgcnn_shape* shape, float* bn_stats, const float* bn_batch, int64_t count,
                                         float momentum, int32_t from_moments, void* stream) {
    RULGNN_TRY(check_bn_update(shape, bn_stats, bn_batch, count));
    return Astgcnn::bn_running_update(shape, bn_stats, bn_batch, count, momentum, from_moments, static_cast<hipStream_t>(stream));
}

// ---- FC_STGNN -----------------------------------------------------------------------------------------
int64_t rulgnn_fcstgnn_bn_count(const rulgnn_fcstgnn_shape* shape) { return Fcstgnn::bn_count(shape); }

int Fcstgnn::check_args(const Shape* shape, const Args* a, bool fwd, bool bwd) {
    if (a->sample_offset < 0 || !(a->dropout_p >= 0.f && a->dropout_p < 1.f)) return RULGNN_EINVAL;
    return check_bn_args(shape->batch, a, fwd, bwd);
}

STEP_FAMILY_ENTRIES_ON(fcstgnn, Fcstgnn, bn_step_fwdbwd)
int rulgnn_fcstgnn_fwdbwd_syncbn_f32(const rulgnn_fcstgnn_shape* shape, const rulgnn_fcstgnn_args* args, float bn_param_grad_scale,
                                     rulgnn_allreduce_f64_fn allreduce, void* user, void* stream) {
    return bn_step_syncbn<Fcstgnn>(shape, args, bn_param_grad_scale, allreduce, user, stream);
}
int rulgnn_fcstgnn_bn_running_update_f32(const rulgnn_fcstgnn_shape* shape, float* bn_stats, const float* bn_batch, float momentum,
                                         int32_t from_moments, void* stream) {
    RULGNN_TRY(check_bn_update(shape, bn_stats, bn_batch));
    return Fcstgnn::bn_running_update(shape, bn_stats, bn_batch, momentum, from_moments, static_cast<hipStream_t>(stream));
}

// ---- ST_Conv ------------------------------------------------------------------------------------------
int Stconv::check_args(const Shape* shape, const Args* a, bool fwd, bool bwd) { return check_bn_args(shape->batch, a, fwd, bwd); }

STEP_FAMILY_ENTRIES_ON(stconv, Stconv, bn_step_fwdbwd)
int rulgnn_stconv_bn_running_update_f32(const rulgnn_stconv_shape* shape, float* bn_stats, const float* bn_batch, int64_t count,
                                        float momentum, int32_t from_moments, void* stream) {
    RULGNN_TRY(check_bn_update(shape, bn_stats, bn_batch, count));
    return Stconv::bn_running_update(shape, bn_stats, bn_batch, count, momentum, from_moments, static_cast<hipStream_t>(stream));
}

// ---- device step state (hipGraph-capturable training steps) -----------------------------------------------
int rulgnn_step_state_set(void* step_state, uint64_t dropout_step, int64_t adam_step, void* stream) {
    if (!step_state || adam_step < 0) return RULGNN_EINVAL;
    if (reinterpret_cast<uintptr_t>(step_state) & 7) return RULGNN_EALIGN;
    return step_state_set(step_state, dropout_step, adam_step, static_cast<hipStream_t>(stream));
}

int rulgnn_adam_step_dev_f32(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, void* step_state,
                             float lr, float beta1, float beta2, float eps, float weight_decay, float grad_scale, void* stream) {
    if (n < 0 || !step_state) return RULGNN_EINVAL;
    const int rc = check_ptrs({params, grads, exp_avg, exp_avg_sq});
    if (rc != RULGNN_OK) return rc;
    return adam_step(params, grads, exp_avg, exp_avg_sq, n, 1, lr, beta1, beta2, eps, weight_decay, grad_scale,
                     static_cast<hipStream_t>(stream), step_state);
}


// ---- HAGCN graph stack ----------------------------------------------------------------------------------
int64_t rulgnn_hagcn_graph_param_count(const rulgnn_hagcn_shape* shape) { return hagcn_graph_param_count(shape); }
size_t rulgnn_hagcn_workspace_bytes(const rulgnn_hagcn_shape* shape) { return hagcn_workspace_bytes(shape); }

int rulgnn_hagcn_graph_forward_f32(const rulgnn_hagcn_shape* shape, const rulgnn_hagcn_args* a, void* stream) {
    if (!shape || !a || shape->graphs < 1) return RULGNN_EINVAL;
    const int rc = check_ptrs({a->nodes, a->params, a->feats, a->kl, a->workspace});
    if (rc != RULGNN_OK) return rc;
    for (const void* p : {(const void*)a->topk, (const void*)a->forced_topk})
        if (!opt_aligned(p)) return RULGNN_EALIGN;
    return hagcn_graph_forward(shape, a, static_cast<hipStream_t>(stream));
}

int rulgnn_hagcn_graph_backward_f32(const rulgnn_hagcn_shape* shape, const rulgnn_hagcn_args* a, void* stream) {
    if (!shape || !a || shape->graphs < 1) return RULGNN_EINVAL;
    const int rc = check_ptrs({a->params, a->dfeats, a->dkl, a->dnodes, a->grads, a->workspace});
    if (rc != RULGNN_OK) return rc;
    return hagcn_graph_backward(shape, a, static_cast<hipStream_t>(stream));
}


// ---- bidirectional LSTM layer (HAGCN encoder) ---------------------------------------------------------------
size_t rulgnn_bilstm_workspace_bytes(const rulgnn_bilstm_shape* shape) { return bilstm_workspace_bytes(shape); }

int rulgnn_bilstm_forward_f32(const rulgnn_bilstm_shape* shape, const rulgnn_bilstm_args* a, void* stream) {
    if (!shape || !a) return RULGNN_EINVAL;
    const int rc = check_ptrs({a->x, a->w_ih[0], a->w_ih[1], a->w_hh[0], a->w_hh[1], a->b_ih[0], a->b_ih[1], a->b_hh[0], a->b_hh[1],
                               a->out, a->workspace});
    if (rc != RULGNN_OK) return rc;
    return bilstm_forward(shape, a, static_cast<hipStream_t>(stream));
}

int rulgnn_bilstm_backward_f32(const rulgnn_bilstm_shape* shape, const rulgnn_bilstm_args* a, void* stream) {
    if (!shape || !a) return RULGNN_EINVAL;
    const int rc = check_ptrs({a->x, a->w_ih[0], a->w_ih[1], a->w_hh[0], a->w_hh[1], a->dout, a->dw_ih[0], a->dw_ih[1], a->dw_hh[0],
                               a->dw_hh[1], a->db_ih[0], a->db_ih[1], a->db_hh[0], a->db_hh[1], a->workspace});
    if (rc != RULGNN_OK) return rc;
    if (!opt_aligned(a->dx)) return RULGNN_EALIGN;
    return bilstm_backward(shape, a, static_cast<hipStream_t>(stream));
}

// grouped forms: the group count first, then every group's pointers like the single entries', all before the first launch
int32_t rulgnn_bilstm_max_groups(void) { return bilstm_max_groups(); }

static int check_bilstm_group_count(const rulgnn_bilstm_shape* shape, const rulgnn_bilstm_args* groups, int32_t num_groups) {
    if (!shape || !groups || num_groups < 1) return RULGNN_EINVAL;
    return num_groups > bilstm_max_groups() ? RULGNN_EUNSUPPORTED : RULGNN_OK;
}

int rulgnn_bilstm_forward_group_f32(const rulgnn_bilstm_shape* shape, const rulgnn_bilstm_args* groups, int32_t num_groups, void* stream) {
    RULGNN_TRY(check_bilstm_group_count(shape, groups, num_groups));
    for (int32_t i = 0; i < num_groups; ++i) {
        const rulgnn_bilstm_args* a = &groups[i];
        RULGNN_TRY(check_ptrs({a->x, a->w_ih[0], a->w_ih[1], a->w_hh[0], a->w_hh[1], a->b_ih[0], a->b_ih[1], a->b_hh[0], a->b_hh[1], a->out,
                               a->workspace}));
    }
    return bilstm_forward_group(shape, groups, num_groups, static_cast<hipStream_t>(stream));
}

int rulgnn_bilstm_backward_group_f32(const rulgnn_bilstm_shape* shape, const rulgnn_bilstm_args* groups, int32_t num_groups, void* stream) {
    RULGNN_TRY(check_bilstm_group_count(shape, groups, num_groups));
    for (int32_t i = 0; i < num_groups; ++i) {
        const rulgnn_bilstm_args* a = &groups[i];
        RULGNN_TRY(check_ptrs({a->x, a->w_ih[0], a->w_ih[1], a->w_hh[0], a->w_hh[1], a->dout, a->dw_ih[0], a->dw_ih[1], a->dw_hh[0],
                               a->dw_hh[1], a->db_ih[0], a->db_ih[1], a->db_hh[0], a->db_hh[1], a->workspace}));
        if (!opt_aligned(a->dx)) return RULGNN_EALIGN;
    }
    return bilstm_backward_group(shape, groups, num_groups, static_cast<hipStream_t>(stream));
}


size_t rulgnn_stgnn_workspace_bytes(const rulgnn_stgnn_shape* shape) { return stgnn_workspace_bytes(shape); }

int rulgnn_stgnn_terms_f32(const rulgnn_stgnn_shape* shape, const float* x, float* terms, float* adj, void* stream) {
    if (!shape) return RULGNN_EINVAL;
    if (shape->batch > 0) {
        const int rc = check_ptrs({x, terms});
        if (rc != RULGNN_OK) return rc;
    }
    return stgnn_terms(shape, x, terms, adj, static_cast<hipStream_t>(stream));
}

int rulgnn_stgnn_cheb_forward_f32(const rulgnn_stgnn_shape* shape, const float* terms, const float* filters, float* out,
                                  void* stream) {
    if (!shape) return RULGNN_EINVAL;
    if (shape->batch > 0) {
        const int rc = check_ptrs({terms, filters, out});
        if (rc != RULGNN_OK) return rc;
    }
    return stgnn_cheb_forward(shape, terms, filters, out, static_cast<hipStream_t>(stream));
}

int rulgnn_stgnn_cheb_backward_f32(const rulgnn_stgnn_shape* shape, const float* terms, const float* dout, float* dfilters,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    if (!shape) return RULGNN_EINVAL;
    int rc = check_ptrs({dfilters, workspace});
    if (rc != RULGNN_OK) return rc;
    if (shape->batch > 0) {
        rc = check_ptrs({terms, dout});
        if (rc != RULGNN_OK) return rc;
    }
    return stgnn_cheb_backward(shape, terms, dout, dfilters, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

int64_t rulgnn_stgnn_param_count(const rulgnn_stgnn_shape* shape) { return Stgnn::param_count(shape); }
size_t rulgnn_stgnn_step_workspace_bytes(const rulgnn_stgnn_shape* shape) { return Stgnn::workspace_bytes(shape); }

int Stgnn::check_args(const Shape* shape, const Args* a, bool fwd, bool bwd) {
    RULGNN_TRY(shape_status(shape));
    RULGNN_TRY(check_ptrs({a->params, a->workspace}));
    if (shape->batch > 0) {
        RULGNN_TRY(check_ptrs({a->x}));
        if (fwd) RULGNN_TRY(check_ptrs({a->pred}));
    }
    if (!bwd) return RULGNN_OK;
    RULGNN_TRY(check_ptrs({a->grads}));
    return shape->batch > 0 && !a->dpred && !(fwd && a->y) ? RULGNN_EINVAL : RULGNN_OK;     // needs d pred, or targets with a forward
}

int rulgnn_stgnn_forward_f32(const rulgnn_stgnn_shape* shape, const rulgnn_stmsgcn_args* args, void* stream) {
    return step_forward<Stgnn>(shape, args, stream);
}
int rulgnn_stgnn_backward_f32(const rulgnn_stgnn_shape* shape, const rulgnn_stmsgcn_args* args, void* stream) {
    return step_backward<Stgnn>(shape, args, stream);
}
int rulgnn_stgnn_fwdbwd_f32(const rulgnn_stgnn_shape* shape, const rulgnn_stmsgcn_args* args, const rulgnn_adam_args* opt, void* stream) {
    return step_fwdbwd<Stgnn>(shape, args, opt, stream);
}

// ---- STNet ------------------------------------------------------------------------------------------
int Stnet::check_args(const Shape* shape, const Args* a, bool, bool bwd) {
    RULGNN_TRY(shape_status(shape));
    return check_step_ptrs(a, shape->batch, bwd);
}

STEP_FAMILY_ENTRIES(stnet, Stnet)

// ---- SAGCN ------------------------------------------------------------------------------------------
int Sagcn::check_args(const Shape* shape, const Args* a, bool, bool bwd) {
    RULGNN_TRY(shape_status(shape));
    return check_step_ptrs(a, shape->batch, bwd);
}

STEP_FAMILY_ENTRIES_TAPS(sagcn, Sagcn)

// ---- AGCN_TF ------------------------------------------------------------------------------------------
int Agcntf::check_args(const Shape* shape, const Args* a, bool, bool bwd) {
    RULGNN_TRY(shape_status(shape));
    return check_step_ptrs(a, shape->batch, bwd);
}

STEP_FAMILY_ENTRIES_TAPS(agcntf, Agcntf)

int rulgnn_sgemm_mode(int32_t mode) {
    const int prev = sgemm_big_mode();
    if (mode == RULGNN_GEMM_F32 || mode == RULGNN_GEMM_BF16X3 || mode == RULGNN_GEMM_BF16X3_ONLY) sgemm_big_mode() = mode;
    return prev;
}

// ---- STAGNN ------------------------------------------------------------------------------------------
int64_t rulgnn_stagnn_bn_state_count(const rulgnn_stagnn_shape* shape) { return Stagnn::bn_state_count(shape); }

int Stagnn::check_args(const Shape* shape, const Args* a, bool, bool bwd) {
    RULGNN_TRY(shape_status(shape));
    RULGNN_TRY(check_ptrs({a->params, a->workspace, a->bn_state}));         // (bn_state ahead of x and pred)
    RULGNN_TRY(check_step_ptrs(a, shape->batch, bwd));
    return bwd && !a->training ? RULGNN_EINVAL : RULGNN_OK;                // (the same code as a batch without d pred or targets)
}

STEP_FAMILY_ENTRIES_TAPS(stagnn, Stagnn)

// ---- plain GEMM -------------------------------------------------------------------------------------------------------------------
int rulgnn_sgemm_f32(const float* A, int64_t sAm, int64_t sAk, const float* B, int64_t sBn, int64_t sBk, float* C, int64_t ldc, int32_t M,
                     int32_t N, int32_t K, int32_t accumulate, void* stream) {
    if (M < 0 || N < 0 || K < 0 || ldc < N) return RULGNN_EINVAL;
    if (M == 0 || N == 0) return RULGNN_OK;
    if (!A || !B || !C) return RULGNN_EINVAL;
    return sgemm(A, sAm, sAk, B, sBn, sBk, C, ldc, M, N, K, accumulate != 0, static_cast<hipStream_t>(stream));
}

int rulgnn_absmax_partials_f32(const float* x, int64_t n, float* partials, int32_t nparts, void* stream) {
    if (n < 0 || nparts <= 0 || nparts > 65535 || !partials || (n > 0 && !x)) return RULGNN_EINVAL;
    return absmax_partials(x, n, partials, nparts, static_cast<hipStream_t>(stream));
}
int rulgnn_sgemm_scaled_f32(const float* A, int64_t sAm, int64_t sAk, const float* B, int64_t sBn, int64_t sBk, float* C, int64_t ldc, int32_t M,
                            int32_t N, int32_t K, int32_t accumulate, const float* amax_a, int32_t amax_na, const float* amax_b, int32_t amax_nb,
                            void* stream) {
    if (M < 0 || N < 0 || K < 0 || ldc < N) return RULGNN_EINVAL;
    if (M == 0 || N == 0) return RULGNN_OK;
    if (!A || !B || !C || !amax_a || !amax_b || amax_na <= 0 || amax_nb <= 0) return RULGNN_EINVAL;
    return sgemm(A, sAm, sAk, B, sBn, sBk, C, ldc, M, N, K, accumulate != 0, static_cast<hipStream_t>(stream), 0, amax_a, amax_na, amax_b, amax_nb);
}

static size_t scaled_plane_bytes(int32_t M, int32_t N, int32_t K) { return ws_align(sgemm_planes_ws_bytes(M, N, K)); }
size_t rulgnn_sgemm_scaled_workspace_bytes(int32_t M, int32_t N, int32_t K, int32_t split_k) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    return scaled_plane_bytes(M, N, K) + (split_k ? sgemm_splitk_need_floats(M, N, K) * sizeof(float) : 0);
}
int rulgnn_sgemm_scaled_ws_f32(const float* A, int64_t sAm, int64_t sAk, const float* B, int64_t sBn, int64_t sBk, float* C, int64_t ldc, int32_t M,
                               int32_t N, int32_t K, int32_t accumulate, const float* amax_a, int32_t amax_na, const float* amax_b, int32_t amax_nb,
                               int32_t split_k, void* workspace, size_t workspace_bytes, int32_t* used_planes, void* stream) {
    if (M < 0 || N < 0 || K < 0 || ldc < N) return RULGNN_EINVAL;
    if (used_planes) *used_planes = 0;
    if (M == 0 || N == 0) return RULGNN_OK;
    if (!A || !B || !C || !amax_a || !amax_b || amax_na <= 0 || amax_nb <= 0 || !workspace) return RULGNN_EINVAL;
    if (workspace_bytes < rulgnn_sgemm_scaled_workspace_bytes(M, N, K, split_k)) return RULGNN_EWORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t pb = scaled_plane_bytes(M, N, K);
    if (used_planes) {
        const int s = sgemm_planes_slices(M, N, K, split_k != 0);
        const bool split_ok = !split_k || (s >= 2 && s <= sgemm_splitk_slices(M, N, K));
        *used_planes = (sgemm_big_mode() == 1 && s >= 1 && split_ok && sgemm_planes_ok(A, sAm, sAk, B, sBn, sBk, M, N, K, s)) ? 1 : 0;
    }
    if (split_k)
        return sgemm_splitk(A, sAm, sAk, B, sBn, sBk, C, ldc, M, N, K, accumulate != 0, reinterpret_cast<float*>(static_cast<unsigned char*>(workspace) + pb),
                            st, amax_a, amax_na, amax_b, amax_nb, workspace, pb);
    return sgemm(A, sAm, sAk, B, sBn, sBk, C, ldc, M, N, K, accumulate != 0, st, 0, amax_a, amax_na, amax_b, amax_nb, workspace, pb);
}

static size_t splitk_part_floats(int32_t M, int32_t N, int32_t K) {
    const size_t a = sgemm_splitk_need_floats(M, N, K), b = sgemm_splitk_need_floats(M, N + 1, K), c = sgemm_splitk_need_floats(M, 1, K);
    const size_t v = a > b ? a : b;
    return ((v > c ? v : c) + 63) & ~(size_t)63;
}
size_t rulgnn_sgemm_splitk_workspace_bytes(int32_t M, int32_t N, int32_t K) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    return (splitk_part_floats(M, N, K) + (size_t)K) * sizeof(float);
}
__global__ void splitk_ones_kernel(float* p, int n) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) p[i] = 1.f;
}
int rulgnn_sgemm_splitk_f32(const float* A, int64_t sAm, int64_t sAk, const float* B, int64_t sBn, int64_t sBk, float* C, int64_t ldc, int32_t M,
                            int32_t N, int32_t K, float* colsum, void* workspace, size_t workspace_bytes, void* stream) {
    if (M < 0 || N < 0 || K < 1 || ldc < N) return RULGNN_EINVAL;
    if (M == 0 || N == 0) return RULGNN_OK;
    if (!A || !B || !C || !workspace) return RULGNN_EINVAL;
    if (workspace_bytes < rulgnn_sgemm_splitk_workspace_bytes(M, N, K)) return RULGNN_EWORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    float* part = static_cast<float*>(workspace);
    if (!colsum) return sgemm_splitk(A, sAm, sAk, B, sBn, sBk, C, ldc, M, N, K, false, part, st);
    float* ones = part + splitk_part_floats(M, N, K);
    RULGNN_TRY(launch_checked(splitk_ones_kernel, dim3(64), dim3(256), 0, st, ones, K));
    return sgemm_splitk_colsum(A, sAm, sAk, B, sBn, sBk, C, ldc, M, N, K, colsum, ones, part, st);
}

// ---- RGCNU ------------------------------------------------------------------------------------------
int Rgcnu::check_args(const Shape* shape, const Args* a, bool, bool bwd) {
    RULGNN_TRY(shape_status(shape));
    if (!(a->dropout_p >= 0.f && a->dropout_p < 1.f)) return RULGNN_EINVAL;
    return check_step_ptrs(a, shape->batch, bwd);
}

STEP_FAMILY_ENTRIES(rgcnu, Rgcnu)

static int check_gru_fwd(const rulgnn_gru_shape* shape, const rulgnn_gru_args* a) {
    if (!shape || !a) return RULGNN_EINVAL;
    RULGNN_TRY(check_ptrs({a->w_ih, a->w_hh, a->b_ih, a->b_hh, a->workspace}));
    return shape->num_seq > 0 ? check_ptrs({a->x, a->out}) : RULGNN_OK;
}
static int check_gru_bwd(const rulgnn_gru_shape* shape, const rulgnn_gru_args* a) {
    if (!shape || !a) return RULGNN_EINVAL;
    RULGNN_TRY(check_ptrs({a->w_ih, a->w_hh, a->b_ih, a->b_hh, a->workspace, a->dw_ih, a->dw_hh, a->db_ih, a->db_hh}));
    return shape->num_seq > 0 ? check_ptrs({a->x, a->dout}) : RULGNN_OK;
}

size_t rulgnn_gru_workspace_bytes(const rulgnn_gru_shape* shape) { return gru_workspace_bytes(shape); }

int rulgnn_gru_forward_f32(const rulgnn_gru_shape* shape, const rulgnn_gru_args* args, void* stream) {
    RULGNN_TRY(check_gru_fwd(shape, args));
    return gru_forward(shape, args, static_cast<hipStream_t>(stream));
}

int rulgnn_gru_backward_f32(const rulgnn_gru_shape* shape, const rulgnn_gru_args* args, void* stream) {
    RULGNN_TRY(check_gru_bwd(shape, args));
    return gru_backward(shape, args, static_cast<hipStream_t>(stream));
}

size_t rulgnn_gru_persistent_workspace_bytes(const rulgnn_gru_shape* shape) { return gru_persistent_workspace_bytes(shape); }

int rulgnn_gru_persistent_forward_f32(const rulgnn_gru_shape* shape, const rulgnn_gru_args* args, void* stream) {
    RULGNN_TRY(check_gru_fwd(shape, args));
    return gru_persistent_forward(shape, args, static_cast<hipStream_t>(stream));
}

int rulgnn_gru_persistent_backward_f32(const rulgnn_gru_shape* shape, const rulgnn_gru_args* args, void* stream) {
    RULGNN_TRY(check_gru_bwd(shape, args));
    if (!opt_aligned(args->dx)) return RULGNN_EALIGN;
    return gru_persistent_backward(shape, args, static_cast<hipStream_t>(stream));
}

// ---- GRU_CM ------------------------------------------------------------------------------------------
int Grucm::check_args(const Shape* shape, const Args* a, bool, bool bwd) {
    RULGNN_TRY(shape_status(shape));
    if (a->global_batch < shape->batch || a->sample_offset < 0) return RULGNN_EINVAL;
    for (int site = 0; site < 3; ++site)
        if (!(a->dropout_p[site] >= 0.f && a->dropout_p[site] < 1.f)) return RULGNN_EINVAL;
    if (a->gru_path != RULGNN_GRUCM_GRU_AUTO && a->gru_path != RULGNN_GRUCM_GRU_STEP_LOOP && a->gru_path != RULGNN_GRUCM_GRU_PERSISTENT)
        return RULGNN_EINVAL;
    RULGNN_TRY(check_fwd_ptrs(a, shape->batch));
    for (const void* p : {(const void*)a->y, (const void*)a->dpred, (const void*)a->loss})
        if (!opt_aligned(p)) return RULGNN_EALIGN;
    return bwd ? check_bwd_ptrs(a, shape->batch) : RULGNN_OK;
}

STEP_FAMILY_ENTRIES(grucm, Grucm)

// ---- HierCorrPool ------------------------------------------------------------------------------------------
int64_t rulgnn_hiercorrpool_bn_state_count(const rulgnn_hiercorrpool_shape* shape) { return Hiercorrpool::bn_state_count(shape); }

// (HierCorrPool_bearing takes the same argument struct)
static int check_hiercorrpool_args(const rulgnn_hiercorrpool_args* a, int64_t batch, bool bwd) {
    if (a->global_batch < batch || a->sample_offset < 0) return RULGNN_EINVAL;
    if (!(a->dropout_p >= 0.f && a->dropout_p < 1.f)) return RULGNN_EINVAL;
    RULGNN_TRY(check_ptrs({a->params, a->workspace, a->bn_state}));
    RULGNN_TRY(check_step_ptrs(a, batch, bwd));
    return bwd && !a->training ? RULGNN_EINVAL : RULGNN_OK;
}

int Hiercorrpool::check_args(const Shape* shape, const Args* a, bool, bool bwd) {
    RULGNN_TRY(shape_status(shape));
    return check_hiercorrpool_args(a, shape->batch, bwd);
}

STEP_FAMILY_ENTRIES_TAPS(hiercorrpool, Hiercorrpool)

// ---- HierCorrPool_bearing --------------------------------------------------------------------------
int64_t rulgnn_hcpb_bn_state_count(const rulgnn_hcpb_shape* shape) { return Hcpb::bn_state_count(shape); }

int Hcpb::check_args(const Shape* shape, const Args* a, bool, bool bwd) {
    RULGNN_TRY(shape_status(shape));
    return check_hiercorrpool_args(a, shape->batch, bwd);
}

STEP_FAMILY_ENTRIES_TAPS(hcpb, Hcpb)

// ---- LOGO ------------------------------------------------------------------------------------------
// (LOGO_bearing takes the same argument struct)
static int check_logo_args(const rulgnn_logo_args* a, int64_t batch, bool bwd) {
    if (a->global_batch < batch) return RULGNN_EINVAL;
    if (!(a->dropout_p >= 0.f && a->dropout_p < 1.f)) return RULGNN_EINVAL;
    if (!opt_aligned(a->loss) || !opt_aligned(a->loss_gl)) return RULGNN_EALIGN;
    return check_step_ptrs(a, batch, bwd);
}

int Logo::check_args(const Shape* shape, const Args* a, bool, bool bwd) {
    RULGNN_TRY(shape_status(shape));
    return check_logo_args(a, shape->batch, bwd);
}

STEP_FAMILY_ENTRIES_TAPS(logo, Logo)
STEP_FAMILY_GROUP_ENTRY(logo, Logo)

// ---- LOGO_bearing ----------------------------------------------------------------------------------
int Logob::check_args(const Shape* shape, const Args* a, bool, bool bwd) {
    RULGNN_TRY(shape_status(shape));
    return check_logo_args(a, shape->batch, bwd);
}

STEP_FAMILY_ENTRIES_TAPS(logob, Logob)

// ---- DVGTformer, GDAGDL, GAT_LSTM, STFA: dropout drawn by sample index in the global batch ---------------------------------------------
// What their entries refuse behind shape_status, in this order: a global batch below the batch or a negative sample offset, a rate
// outside [0, 1) (EINVAL); a global batch whose last dropout counter passes 32 bits at `draws_per_sample` draws (EUNSUPPORTED; 0 draws:
// the family's counter has no such bound); a misaligned optional pointer -- y, dpred, loss and the family's `more`; then the step's
// pointers.
extern "C++" {
template <typename A>
static int check_dropout_step_args(const A* a, int64_t batch, bool bwd, double draws_per_sample, std::initializer_list<const void*> more = {}) {
    if (a->global_batch < batch || a->sample_offset < 0) return RULGNN_EINVAL;
    if (!(a->dropout_p >= 0.f && a->dropout_p < 1.f)) return RULGNN_EINVAL;
    if (((double)a->sample_offset + (double)batch) * draws_per_sample > 4294967296.0 || (double)a->global_batch * draws_per_sample > 4294967296.0)
        return RULGNN_EUNSUPPORTED;
    for (const void* p : {(const void*)a->y, (const void*)a->dpred, (const void*)a->loss})
        if (!opt_aligned(p)) return RULGNN_EALIGN;
    for (const void* p : more)
        if (!opt_aligned(p)) return RULGNN_EALIGN;
    return check_step_ptrs(a, batch, bwd);
}
}  // extern "C++"

// (one mask per temporal block: no counter bound)
int Dvgtformer::check_args(const Shape* shape, const Args* a, bool, bool bwd) {
    RULGNN_TRY(shape_status(shape));
    return check_dropout_step_args(a, shape->batch, bwd, 0.0);
}
STEP_FAMILY_ENTRIES_TAPS(dvgtformer, Dvgtformer)
STEP_FAMILY_GROUP_ENTRY(dvgtformer, Dvgtformer)

// (a draw per attention entry)
int Gdagdl::check_args(const Shape* shape, const Args* a, bool, bool bwd) {
    RULGNN_TRY(shape_status(shape));
    return check_dropout_step_args(a, shape->batch, bwd, (double)shape->num_patch * shape->num_nodes * shape->num_nodes, {a->recon, a->recon_weight});
}
STEP_FAMILY_ENTRIES_TAPS(gdagdl, Gdagdl)

// (a draw per band entry)
int Gatlstm::check_args(const Shape* shape, const Args* a, bool, bool bwd) {
    RULGNN_TRY(shape_status(shape));
    return check_dropout_step_args(a, shape->batch, bwd, 3.0 * (double)shape->num_patch);
}
STEP_FAMILY_ENTRIES_TAPS(gatlstm, Gatlstm)

// (a draw per directed edge, head and patch)
int Stfa::check_args(const Shape* shape, const Args* a, bool, bool bwd) {
    RULGNN_TRY(shape_status(shape));
    return check_dropout_step_args(a, shape->batch, bwd, 44.0 * (double)shape->num_heads * (double)shape->num_patch);
}
STEP_FAMILY_ENTRIES_TAPS(stfa, Stfa)

size_t rulgnn_rul_metrics_workspace_bytes(int64_t n) { return rul_metrics_workspace_bytes(n); }

int rulgnn_rul_metrics_f32(const float* pred, const float* real, int64_t n, float max_rul, double* out, void* workspace,
                           size_t workspace_bytes, void* stream) {
    if (n < 1) return RULGNN_EINVAL;
    const int rc = check_ptrs({pred, real, out, workspace});
    if (rc != RULGNN_OK) return rc;
    return rul_metrics(pred, real, n, max_rul, out, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

int rulgnn_rul_metric_sums_f32(const float* pred, const float* real, int64_t n, float max_rul, double* out, void* workspace,
                               size_t workspace_bytes, void* stream) {
    if (n < 1) return RULGNN_EINVAL;
    const int rc = check_ptrs({pred, real, out, workspace});
    if (rc != RULGNN_OK) return rc;
    return rul_metrics(pred, real, n, max_rul, out, workspace, workspace_bytes, static_cast<hipStream_t>(stream), 1);
}

}  // extern "C"
