// Host-side entry points of every family but ST_GCN (stgcn_host.hpp), the Adam / BatchNorm / step-state helpers and the metrics: what
// rulgnn_api.hip calls and what the family translation units define.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rulgnn.h"
#include "stgcn_host.hpp"          // StepState, dropout_layer_key, SyncHook (bn_cells.hpp), host_util.hpp

namespace rulgnn {

// ---- step families -------------------------------------------------------------------------------------------------------------------
// A step family is a model behind rulgnn_<family>_{forward,backward,fwdbwd}_f32: one shape struct, one args struct.  Its description, a
// struct derived from StepFamily<Shape, Args>, is what rulgnn_api.hip instantiates its entry templates on (step_forward, step_backward,
// step_fwdbwd); the family's translation unit defines the members declared here:
//   shape_status(s)      RULGNN_OK, or the code every entry returns for a refused shape: decided there alone, next to the geometry.
//                        (STMSGCN and the BatchNorm families have none: run() answers with its geometry's code behind the argument check.)
//   param_count(s), workspace_bytes(s)      the queries: -1 / 0 for a refused shape
//   run(s, a, mode, stream)                 mode bit 0: forward, bit 1: backward; checks the workspace size before its first launch
//   check_args(s, a, fwd, bwd)              what the entries refuse before run(): shape_status, then the args' own fields (defined in
//                                           rulgnn_api.hip on its pointer checks; s and a are not null)
//   adam_first(s), adam_frozen_tail(s)      the fused step's Adam updates the flat floats [adam_first, param_count - adam_frozen_tail)
//   run_group(s, groups, n, stream)        (the families with a rulgnn_<family>_fwdbwd_group_f32 entry) mode 3 of `n` runs of one shape in one
//                                           call, groups[i] run i's arguments: what run() enqueues for each, its dominant kernels as
//                                           grouped launches (grid y = the run); the entry has checked every group, workspaces included
// Most runs a grouped fused step advances (rulgnn_step_max_groups): their pointer tables travel by value in the kernel arguments.
constexpr int STEP_MAX_GROUPS = 8;
template <typename S, typename A>
struct StepFamily {
    using Shape = S;
    using Args = A;
    static int64_t adam_first(const S*) { return 0; }
    static int64_t adam_frozen_tail(const S*) { return 0; }
};

struct Stmsgcn : StepFamily<rulgnn_stmsgcn_shape, rulgnn_stmsgcn_args> {
    static int64_t param_count(const Shape* s);
    static size_t workspace_bytes(const Shape* s);
    [[nodiscard]] static int run(const Shape* s, const Args* a, int mode, hipStream_t st);
    [[nodiscard]] static int check_args(const Shape* s, const Args* a, bool fwd, bool bwd);
};
[[nodiscard]] int stmsgcn_features(const rulgnn_stmsgcn_shape* s, const float* x, const float* prm, float* features, hipStream_t stream);

// The BatchNorm families (ASTGCNN, FC_STGNN, ST_Conv) share their argument check and fused step (rulgnn_api.hip: check_bn_args,
// bn_step_fwdbwd).  On top of a step family's members:
//   run_takes_optimizer      run() has the trailing parameters of a whole training step -- `sync`: synchronised BatchNorm (the
//                            *_fwdbwd_syncbn_f32 entry); `bn_running_out`, plain batch statistics: the step updates the running statistics
//                            itself; `adam`: the constants of the optimizer update (adam_fuse_args) -- on return adam->gbase != nullptr says
//                            the step's last kernel applied it (adam_device.hpp), else the caller launches adam_step
//   bn_running_update(...)   the running-statistics update as a launch of its own; step_bn_update(...): the same behind a fused step
struct AdamFuse;          // adam_device.hpp
void adam_fuse_args(AdamFuse* t, float* p, float* m, float* v, const float* gbase, int64_t step, float lr, float beta1, float beta2, float eps,
                    float wd);
struct Astgcnn : StepFamily<rulgnn_astgcnn_shape, rulgnn_astgcnn_args> {
    static constexpr bool run_takes_optimizer = true;
    static int64_t param_count(const Shape* s);
    static size_t workspace_bytes(const Shape* s);
    [[nodiscard]] static int run(const Shape* s, const Args* a, int mode, hipStream_t st, const SyncHook* sync = nullptr, float* bn_running_out = nullptr,
                   float bn_momentum = 0.f, AdamFuse* adam = nullptr);
    [[nodiscard]] static int check_args(const Shape* s, const Args* a, bool fwd, bool bwd);
    [[nodiscard]] static int bn_running_update(const Shape* s, float* bn_stats, const float* bn_batch, int64_t count, float momentum, int from_moments,
                                 hipStream_t st);
    [[nodiscard]] static int step_bn_update(const Shape* s, float* bn_stats, const float* bn_batch, float momentum, int from_moments, hipStream_t st) {
        return bn_running_update(s, bn_stats, bn_batch, s->batch * (int64_t)s->time_length, momentum, from_moments, st);
    }
};
// (bn_running_out: the update rides on the side stream behind the batch-statistics kernel; adam: always applied, by the step's last launch)
struct Fcstgnn : StepFamily<rulgnn_fcstgnn_shape, rulgnn_fcstgnn_args> {
    static constexpr bool run_takes_optimizer = true;
    static int64_t param_count(const Shape* s);
    static int64_t bn_count(const Shape* s);
    static size_t workspace_bytes(const Shape* s);
    [[nodiscard]] static int run(const Shape* s, const Args* a, int mode, hipStream_t st, const SyncHook* sync = nullptr, float* bn_running_out = nullptr,
                   float bn_momentum = 0.f, const AdamFuse* adam = nullptr);
    [[nodiscard]] static int check_args(const Shape* s, const Args* a, bool fwd, bool bwd);
    [[nodiscard]] static int bn_running_update(const Shape* s, float* bn_stats, const float* bn_batch, float momentum, int from_moments, hipStream_t st);
    [[nodiscard]] static int step_bn_update(const Shape* s, float* bn_stats, const float* bn_batch, float momentum, int from_moments, hipStream_t st) {
        return bn_running_update(s, bn_stats, bn_batch, momentum, from_moments, st);          // (the element counts are the shape's)
    }
};
// (the args struct is ASTGCNN's)
struct Stconv : StepFamily<rulgnn_stconv_shape, rulgnn_astgcnn_args> {
    static constexpr bool run_takes_optimizer = false;
    static int64_t param_count(const Shape* s);
    static size_t workspace_bytes(const Shape* s);
    [[nodiscard]] static int run(const Shape* s, const Args* a, int mode, hipStream_t st);
    [[nodiscard]] static int check_args(const Shape* s, const Args* a, bool fwd, bool bwd);
    [[nodiscard]] static int bn_running_update(const Shape* s, float* bn_stats, const float* bn_batch, int64_t count, float momentum, int from_moments,
                                 hipStream_t st);
    [[nodiscard]] static int step_bn_update(const Shape* s, float* bn_stats, const float* bn_batch, float momentum, int from_moments, hipStream_t st) {
        return bn_running_update(s, bn_stats, bn_batch, s->batch * (int64_t)s->time_length, momentum, from_moments, st);
    }
};

// (the args struct is STMSGCN's; workspace_bytes is the step's -- stgnn_workspace_bytes below is that of the terms / cheb entries)
struct Stgnn : StepFamily<rulgnn_stgnn_shape, rulgnn_stmsgcn_args> {
    [[nodiscard]] static int shape_status(const Shape* s);
    static int64_t param_count(const Shape* s);
    static size_t workspace_bytes(const Shape* s);
    [[nodiscard]] static int run(const Shape* s, const Args* a, int mode, hipStream_t st);
    [[nodiscard]] static int check_args(const Shape* s, const Args* a, bool fwd, bool bwd);
};
struct Stnet : StepFamily<rulgnn_stnet_shape, rulgnn_stnet_args> {
    // cnn.{weight, bias} (the first 3 entries) have no gradient in the reference (`grad is None`): torch's Adam leaves them untouched
    static int64_t adam_first(const Shape*) { return 3; }
    [[nodiscard]] static int shape_status(const Shape* s);
    static int64_t param_count(const Shape* s);
    static size_t workspace_bytes(const Shape* s);
    [[nodiscard]] static int run(const Shape* s, const Args* a, int mode, hipStream_t st);
    [[nodiscard]] static int check_args(const Shape* s, const Args* a, bool fwd, bool bwd);
};
struct Sagcn : StepFamily<rulgnn_sagcn_shape, rulgnn_sagcn_args> {
    [[nodiscard]] static int shape_status(const Shape* s);
    static int64_t param_count(const Shape* s);
    static size_t workspace_bytes(const Shape* s);
    static int64_t tap_offset(const Shape* s, int which);
    [[nodiscard]] static int run(const Shape* s, const Args* a, int mode, hipStream_t st);
    [[nodiscard]] static int check_args(const Shape* s, const Args* a, bool fwd, bool bwd);
};
// SAGCN's parameter-free front end alone: x [B][P * n] -> raw [B * P][20] (scratch) -> features [B][P][40] (unit Frobenius norm)
[[nodiscard]] int sagcn_features(int64_t B, int P, int n, const float* x, float* raw, float* feat, hipStream_t st);
struct Agcntf : StepFamily<rulgnn_agcntf_shape, rulgnn_agcntf_args> {
    [[nodiscard]] static int shape_status(const Shape* s);
    static int64_t param_count(const Shape* s);
    static size_t workspace_bytes(const Shape* s);
    static int64_t tap_offset(const Shape* s, int which);
    [[nodiscard]] static int run(const Shape* s, const Args* a, int mode, hipStream_t st);
    [[nodiscard]] static int check_args(const Shape* s, const Args* a, bool fwd, bool bwd);
};
struct Stagnn : StepFamily<rulgnn_stagnn_shape, rulgnn_stagnn_args> {
    [[nodiscard]] static int shape_status(const Shape* s);
    static int64_t param_count(const Shape* s);
    static int64_t bn_state_count(const Shape* s);
    static size_t workspace_bytes(const Shape* s);
    static int64_t tap_offset(const Shape* s, int which);
    [[nodiscard]] static int run(const Shape* s, const Args* a, int mode, hipStream_t st);
    [[nodiscard]] static int check_args(const Shape* s, const Args* a, bool fwd, bool bwd);
};
struct Rgcnu : StepFamily<rulgnn_rgcnu_shape, rulgnn_rgcnu_args> {
    // the second head (fc2, the last E*L + 1 entries) has no gradient in the reference (`grad is None`): torch's Adam leaves it untouched
    static int64_t adam_frozen_tail(const Shape* s) { return (int64_t)s->encoder_hidden_dim * s->time_length + 1; }
    [[nodiscard]] static int shape_status(const Shape* s);
    static int64_t param_count(const Shape* s);
    static size_t workspace_bytes(const Shape* s);
    [[nodiscard]] static int run(const Shape* s, const Args* a, int mode, hipStream_t st);
    [[nodiscard]] static int check_args(const Shape* s, const Args* a, bool fwd, bool bwd);
};
struct Grucm : StepFamily<rulgnn_grucm_shape, rulgnn_grucm_args> {
    [[nodiscard]] static int shape_status(const Shape* s);
    static int64_t param_count(const Shape* s);
    static size_t workspace_bytes(const Shape* s);
    [[nodiscard]] static int run(const Shape* s, const Args* a, int mode, hipStream_t st);
    [[nodiscard]] static int check_args(const Shape* s, const Args* a, bool fwd, bool bwd);
};
struct Hiercorrpool : StepFamily<rulgnn_hiercorrpool_shape, rulgnn_hiercorrpool_args> {
    [[nodiscard]] static int shape_status(const Shape* s);
    static int64_t param_count(const Shape* s);
    static int64_t bn_state_count(const Shape* s);
    static size_t workspace_bytes(const Shape* s);
    static int64_t tap_offset(const Shape* s, int which);
    [[nodiscard]] static int run(const Shape* s, const Args* a, int mode, hipStream_t st);
    [[nodiscard]] static int check_args(const Shape* s, const Args* a, bool fwd, bool bwd);
};
// (the args struct is HierCorrPool's; x is the raw window [batch][num_patch * patch_size])
struct Hcpb : StepFamily<rulgnn_hcpb_shape, rulgnn_hiercorrpool_args> {
    [[nodiscard]] static int shape_status(const Shape* s);
    static int64_t param_count(const Shape* s);
    static int64_t bn_state_count(const Shape* s);
    static size_t workspace_bytes(const Shape* s);
    static int64_t tap_offset(const Shape* s, int which);
    [[nodiscard]] static int run(const Shape* s, const Args* a, int mode, hipStream_t st);
    [[nodiscard]] static int check_args(const Shape* s, const Args* a, bool fwd, bool bwd);
};
struct Logo : StepFamily<rulgnn_logo_shape, rulgnn_logo_args> {
    [[nodiscard]] static int shape_status(const Shape* s);
    static int64_t param_count(const Shape* s);
    static size_t workspace_bytes(const Shape* s);
    static int64_t tap_offset(const Shape* s, int which);
    [[nodiscard]] static int run(const Shape* s, const Args* a, int mode, hipStream_t st);
    [[nodiscard]] static int run_group(const Shape* s, const Args* groups, int n, hipStream_t st);
    [[nodiscard]] static int check_args(const Shape* s, const Args* a, bool fwd, bool bwd);
};
// (the args struct is LOGO's; x is the raw window [batch][num_patch * patch_size])
struct Logob : StepFamily<rulgnn_logob_shape, rulgnn_logo_args> {
    [[nodiscard]] static int shape_status(const Shape* s);
    static int64_t param_count(const Shape* s);
    static size_t workspace_bytes(const Shape* s);
    static int64_t tap_offset(const Shape* s, int which);
    [[nodiscard]] static int run(const Shape* s, const Args* a, int mode, hipStream_t st);
    [[nodiscard]] static int check_args(const Shape* s, const Args* a, bool fwd, bool bwd);
};
struct Dvgtformer : StepFamily<rulgnn_dvgtformer_shape, rulgnn_dvgtformer_args> {
    [[nodiscard]] static int shape_status(const Shape* s);
    static int64_t param_count(const Shape* s);
    static size_t workspace_bytes(const Shape* s);
    static int64_t tap_offset(const Shape* s, int which);
    [[nodiscard]] static int run(const Shape* s, const Args* a, int mode, hipStream_t st);
    [[nodiscard]] static int run_group(const Shape* s, const Args* groups, int n, hipStream_t st);
    [[nodiscard]] static int check_args(const Shape* s, const Args* a, bool fwd, bool bwd);
};
struct Gdagdl : StepFamily<rulgnn_gdagdl_shape, rulgnn_gdagdl_args> {
    // node_importance_linear.{weight, bias} (the first f + 1 entries) have no gradient in the reference: torch's Adam leaves them untouched
    static int64_t adam_first(const Shape* s);
    [[nodiscard]] static int shape_status(const Shape* s);
    static int64_t param_count(const Shape* s);
    static size_t workspace_bytes(const Shape* s);
    static int64_t tap_offset(const Shape* s, int which);
    [[nodiscard]] static int run(const Shape* s, const Args* a, int mode, hipStream_t st);
    [[nodiscard]] static int check_args(const Shape* s, const Args* a, bool fwd, bool bwd);
};
struct Gatlstm : StepFamily<rulgnn_gatlstm_shape, rulgnn_gatlstm_args> {
    [[nodiscard]] static int shape_status(const Shape* s);
    static int64_t param_count(const Shape* s);
    static size_t workspace_bytes(const Shape* s);
    static int64_t tap_offset(const Shape* s, int which);
    [[nodiscard]] static int run(const Shape* s, const Args* a, int mode, hipStream_t st);
    [[nodiscard]] static int check_args(const Shape* s, const Args* a, bool fwd, bool bwd);
};
// v.{weight, bias} stay inside Adam's range: the reference gives them zero gradients, not None, and its weight decay moves them
struct Stfa : StepFamily<rulgnn_stfa_shape, rulgnn_stfa_args> {
    [[nodiscard]] static int shape_status(const Shape* s);
    static int64_t param_count(const Shape* s);
    static size_t workspace_bytes(const Shape* s);
    static int64_t tap_offset(const Shape* s, int which);
    [[nodiscard]] static int run(const Shape* s, const Args* a, int mode, hipStream_t st);
    [[nodiscard]] static int check_args(const Shape* s, const Args* a, bool fwd, bool bwd);
};

int64_t hagcn_graph_param_count(const rulgnn_hagcn_shape* s);
size_t hagcn_workspace_bytes(const rulgnn_hagcn_shape* s);
[[nodiscard]] int hagcn_graph_forward(const rulgnn_hagcn_shape* s, const rulgnn_hagcn_args* a, hipStream_t stream);
[[nodiscard]] int hagcn_graph_backward(const rulgnn_hagcn_shape* s, const rulgnn_hagcn_args* a, hipStream_t stream);
size_t bilstm_workspace_bytes(const rulgnn_bilstm_shape* s);
[[nodiscard]] int bilstm_forward(const rulgnn_bilstm_shape* s, const rulgnn_bilstm_args* a, hipStream_t stream, int ndir = 2);
[[nodiscard]] int bilstm_backward(const rulgnn_bilstm_shape* s, const rulgnn_bilstm_args* a, hipStream_t stream, int ndir = 2);
// `n` bidirectional layers of one shape (1 <= n <= bilstm_max_groups()), their recurrences in one launch: groups[i] is layer i's arguments
int bilstm_max_groups();
[[nodiscard]] int bilstm_forward_group(const rulgnn_bilstm_shape* s, const rulgnn_bilstm_args* groups, int n, hipStream_t stream);
[[nodiscard]] int bilstm_backward_group(const rulgnn_bilstm_shape* s, const rulgnn_bilstm_args* groups, int n, hipStream_t stream);
[[nodiscard]] int adam_step(float* p, const float* g, float* m, float* v, int64_t n, int64_t step, float lr, float beta1, float beta2,
              float eps, float wd, float gscale, hipStream_t stream, void* step_state = nullptr, const float* guard = nullptr);
// Synchronised BatchNorm, the one step behind every launch that completes a reduction pair (bn_cells.hpp): the CELL_REP replicas of the
// `n` <= 128 contiguous doubles at cells + off (the replicas `replica_stride` doubles apart) are collapsed into replica 0, then
// h->fn runs on cells + off.  RULGNN_OK at once when `h` is null; RULGNN_EHIP / RULGNN_ECALLBACK.
[[nodiscard]] int sync_cells(const SyncHook* h, double* cells, int off, int n, int replica_stride, hipStream_t st);
// p[0 .. n) = v
[[nodiscard]] int fill_f32(float* p, int64_t n, float v, hipStream_t st);
[[nodiscard]] int step_state_set(void* state, uint64_t dropout_step, int64_t adam_step, hipStream_t stream);
[[nodiscard]] int step_prepare_dropout(void* state, uint64_t seed, int num_layers, hipStream_t stream);   // ++dropout_step, keys
[[nodiscard]] int step_prepare_adam(void* state, float lr, float beta1, float beta2, hipStream_t stream); // ++adam_step, bias corrections
[[nodiscard]] int bn_running_update(float* bn, const float* batch, int num_layers, int64_t count, float momentum, int from_moments,
                      hipStream_t stream, const float* guard = nullptr);
// adam_step + bn_running_update in one launch (what follows a data-parallel bucket all-reduce); `guard` may be null
[[nodiscard]] int adam_bn_step(float* p, const float* g, float* m, float* v, int64_t n, int64_t step, float lr, float beta1, float beta2, float eps,
                 float wd, float gscale, float* bn, const float* batch, int num_layers, int64_t count, float momentum, int from_moments,
                 const float* guard, hipStream_t stream);

size_t stgnn_workspace_bytes(const rulgnn_stgnn_shape* s);
[[nodiscard]] int stgnn_terms(const rulgnn_stgnn_shape* s, const float* x, float* terms, float* adj, hipStream_t st);
[[nodiscard]] int stgnn_cheb_forward(const rulgnn_stgnn_shape* s, const float* terms, const float* filters, float* out, hipStream_t st);
[[nodiscard]] int stgnn_cheb_backward(const rulgnn_stgnn_shape* s, const float* terms, const float* dout, float* dfilters, void* workspace,
                        size_t workspace_bytes, hipStream_t st);
size_t gru_workspace_bytes(const rulgnn_gru_shape* s);
[[nodiscard]] int gru_forward(const rulgnn_gru_shape* s, const rulgnn_gru_args* a, hipStream_t st);
[[nodiscard]] int gru_backward(const rulgnn_gru_shape* s, const rulgnn_gru_args* a, hipStream_t st);
// the same layer as one launch over all steps (gru_seq.hip); 0 / RULGNN_EUNSUPPORTED outside hidden_dim == 64, input_dim <= 64, seq_len <= 1024
size_t gru_persistent_workspace_bytes(const rulgnn_gru_shape* s);
[[nodiscard]] int gru_persistent_forward(const rulgnn_gru_shape* s, const rulgnn_gru_args* a, hipStream_t st);
[[nodiscard]] int gru_persistent_backward(const rulgnn_gru_shape* s, const rulgnn_gru_args* a, hipStream_t st);
size_t rul_metrics_workspace_bytes(int64_t n);
[[nodiscard]] int rul_metrics(const float* pred, const float* real, int64_t n, float max_rul, double* out, void* workspace, size_t workspace_bytes,
                hipStream_t st, int raw = 0);

}  // namespace rulgnn
