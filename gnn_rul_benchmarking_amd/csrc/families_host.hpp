// Host-side entry points of every family but ST_GCN (stgcn_host.hpp), the Adam / BatchNorm / step-state helpers and the metrics: what
// rulgnn_api.hip calls and what the family translation units define.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rulgnn.h"
#include "stgcn_host.hpp"          // StepState, dropout_layer_key, SyncHook (bn_cells.hpp), host_util.hpp

namespace rulgnn {

int64_t stmsgcn_param_count(const rulgnn_stmsgcn_shape* s);
size_t stmsgcn_workspace_bytes(const rulgnn_stmsgcn_shape* s);
int stmsgcn_features(const rulgnn_stmsgcn_shape* s, const float* x, const float* prm, float* features, hipStream_t stream);
int stmsgcn_run(const rulgnn_stmsgcn_shape* s, const rulgnn_stmsgcn_args* a, int mode, hipStream_t stream);
int64_t astgcnn_param_count(const rulgnn_astgcnn_shape* s);
size_t astgcnn_workspace_bytes(const rulgnn_astgcnn_shape* s);
struct AdamFuse;          // adam_device.hpp
// (`bn_running_out` != nullptr, whole training steps with plain batch statistics: the finalize kernel also updates the running statistics;
// `adam` != nullptr, whole training steps: the constants of the optimizer update (adam_fuse_args) -- on return adam->gbase != nullptr says
// the step's last kernel applied it, else the caller launches adam_step)
int astgcnn_run(const rulgnn_astgcnn_shape* s, const rulgnn_astgcnn_args* a, int mode, hipStream_t stream, const SyncHook* sync = nullptr,
                float* bn_running_out = nullptr, float bn_momentum = 0.f, AdamFuse* adam = nullptr);
void adam_fuse_args(AdamFuse* t, float* p, float* m, float* v, const float* gbase, int64_t step, float lr, float beta1, float beta2, float eps,
                    float wd);
int astgcnn_bn_running_update(const rulgnn_astgcnn_shape* s, float* bn_stats, const float* bn_batch, int64_t count, float momentum,
                              int from_moments, hipStream_t stream);
int64_t fcstgnn_param_count(const rulgnn_fcstgnn_shape* s);
int64_t fcstgnn_bn_count(const rulgnn_fcstgnn_shape* s);
size_t fcstgnn_workspace_bytes(const rulgnn_fcstgnn_shape* s);
// (`bn_running_out` != nullptr, whole training steps with plain batch statistics: the running-statistics update rides on the side stream
// behind the batch-statistics kernel instead of closing the step)
// (`fuse` != nullptr, whole training steps on one rank: the step's last launch -- the finalize kernel, then behind the join with the side
// stream -- applies torch.optim.Adam to every parameter: adam_device.hpp; no optimizer launch)
struct AdamFuse;
int fcstgnn_run(const rulgnn_fcstgnn_shape* s, const rulgnn_fcstgnn_args* a, int mode, hipStream_t stream, const SyncHook* sync = nullptr,
                float* bn_running_out = nullptr, float bn_momentum = 0.f, const AdamFuse* fuse = nullptr);
int fcstgnn_bn_running_update(const rulgnn_fcstgnn_shape* s, float* bn_stats, const float* bn_batch, float momentum, int from_moments,
                              hipStream_t stream);
int64_t hagcn_graph_param_count(const rulgnn_hagcn_shape* s);
size_t hagcn_workspace_bytes(const rulgnn_hagcn_shape* s);
int hagcn_graph_forward(const rulgnn_hagcn_shape* s, const rulgnn_hagcn_args* a, hipStream_t stream);
int hagcn_graph_backward(const rulgnn_hagcn_shape* s, const rulgnn_hagcn_args* a, hipStream_t stream);
size_t bilstm_workspace_bytes(const rulgnn_bilstm_shape* s);
int bilstm_forward(const rulgnn_bilstm_shape* s, const rulgnn_bilstm_args* a, hipStream_t stream, int ndir = 2);
int bilstm_backward(const rulgnn_bilstm_shape* s, const rulgnn_bilstm_args* a, hipStream_t stream, int ndir = 2);
int64_t stconv_param_count(const rulgnn_stconv_shape* s);
size_t stconv_workspace_bytes(const rulgnn_stconv_shape* s);
int stconv_run(const rulgnn_stconv_shape* s, const rulgnn_astgcnn_args* a, int mode, hipStream_t stream);
int stconv_bn_running_update(const rulgnn_stconv_shape* s, float* bn_stats, const float* bn_batch, int64_t count, float momentum,
                             int from_moments, hipStream_t stream);
int adam_step(float* p, const float* g, float* m, float* v, int64_t n, int64_t step, float lr, float beta1, float beta2,
              float eps, float wd, float gscale, hipStream_t stream, void* step_state = nullptr, const float* guard = nullptr);
// Synchronised BatchNorm, the one step behind every launch that completes a reduction pair (bn_cells.hpp): the CELL_REP replicas of the
// `n` <= 128 contiguous doubles at cells + off (the replicas `replica_stride` doubles apart) are collapsed into replica 0, then
// h->fn runs on cells + off.  RULGNN_OK at once when `h` is null; RULGNN_EHIP / RULGNN_ECALLBACK.
int sync_cells(const SyncHook* h, double* cells, int off, int n, int replica_stride, hipStream_t st);
// p[0 .. n) = v
int fill_f32(float* p, int64_t n, float v, hipStream_t st);
int step_state_set(void* state, uint64_t dropout_step, int64_t adam_step, hipStream_t stream);
int step_prepare_dropout(void* state, uint64_t seed, int num_layers, hipStream_t stream);   // ++dropout_step, keys
int step_prepare_adam(void* state, float lr, float beta1, float beta2, hipStream_t stream); // ++adam_step, bias corrections
int bn_running_update(float* bn, const float* batch, int num_layers, int64_t count, float momentum, int from_moments,
                      hipStream_t stream, const float* guard = nullptr);
// adam_step + bn_running_update in one launch (what follows a data-parallel bucket all-reduce); `guard` may be null
int adam_bn_step(float* p, const float* g, float* m, float* v, int64_t n, int64_t step, float lr, float beta1, float beta2, float eps,
                 float wd, float gscale, float* bn, const float* batch, int num_layers, int64_t count, float momentum, int from_moments,
                 const float* guard, hipStream_t stream);

size_t stgnn_workspace_bytes(const rulgnn_stgnn_shape* s);
int stgnn_terms(const rulgnn_stgnn_shape* s, const float* x, float* terms, float* adj, hipStream_t st);
int stgnn_cheb_forward(const rulgnn_stgnn_shape* s, const float* terms, const float* filters, float* out, hipStream_t st);
int stgnn_cheb_backward(const rulgnn_stgnn_shape* s, const float* terms, const float* dout, float* dfilters, void* workspace,
                        size_t workspace_bytes, hipStream_t st);
int64_t stnet_param_count(const rulgnn_stnet_shape* s);
size_t stnet_workspace_bytes(const rulgnn_stnet_shape* s);
int stnet_run(const rulgnn_stnet_shape* s, const rulgnn_stnet_args* a, int mode, hipStream_t st);
int64_t sagcn_param_count(const rulgnn_sagcn_shape* s);
size_t sagcn_workspace_bytes(const rulgnn_sagcn_shape* s);
int64_t sagcn_tap_offset(const rulgnn_sagcn_shape* s, int which);
int sagcn_run(const rulgnn_sagcn_shape* s, const rulgnn_sagcn_args* a, int mode, hipStream_t st);
// SAGCN's parameter-free front end alone: x [B][P * n] -> raw [B * P][20] (scratch) -> features [B][P][40] (unit Frobenius norm)
int sagcn_features(int64_t B, int P, int n, const float* x, float* raw, float* feat, hipStream_t st);
int64_t agcntf_param_count(const rulgnn_agcntf_shape* s);
size_t agcntf_workspace_bytes(const rulgnn_agcntf_shape* s);
int64_t agcntf_tap_offset(const rulgnn_agcntf_shape* s, int which);
int agcntf_run(const rulgnn_agcntf_shape* s, const rulgnn_agcntf_args* a, int mode, hipStream_t st);
int64_t stagnn_param_count(const rulgnn_stagnn_shape* s);
int64_t stagnn_bn_state_count(const rulgnn_stagnn_shape* s);
size_t stagnn_workspace_bytes(const rulgnn_stagnn_shape* s);
int64_t stagnn_tap_offset(const rulgnn_stagnn_shape* s, int which);
int stagnn_run(const rulgnn_stagnn_shape* s, const rulgnn_stagnn_args* a, int mode, hipStream_t st);
int64_t rgcnu_param_count(const rulgnn_rgcnu_shape* s);
size_t rgcnu_workspace_bytes(const rulgnn_rgcnu_shape* s);
int rgcnu_run(const rulgnn_rgcnu_shape* s, const rulgnn_rgcnu_args* a, int mode, hipStream_t st);
int64_t stgnn_param_count(const rulgnn_stgnn_shape* s);
size_t stgnn_step_workspace_bytes(const rulgnn_stgnn_shape* s);
int stgnn_run(const rulgnn_stgnn_shape* s, const rulgnn_stmsgcn_args* a, int mode, hipStream_t st);
size_t gru_workspace_bytes(const rulgnn_gru_shape* s);
int gru_forward(const rulgnn_gru_shape* s, const rulgnn_gru_args* a, hipStream_t st);
int gru_backward(const rulgnn_gru_shape* s, const rulgnn_gru_args* a, hipStream_t st);
// the same layer as one launch over all steps (gru_seq.hip); 0 / RULGNN_EUNSUPPORTED outside hidden_dim == 64, input_dim <= 64, seq_len <= 1024
size_t gru_persistent_workspace_bytes(const rulgnn_gru_shape* s);
int gru_persistent_forward(const rulgnn_gru_shape* s, const rulgnn_gru_args* a, hipStream_t st);
int gru_persistent_backward(const rulgnn_gru_shape* s, const rulgnn_gru_args* a, hipStream_t st);
int64_t grucm_param_count(const rulgnn_grucm_shape* s);
size_t grucm_workspace_bytes(const rulgnn_grucm_shape* s);
int grucm_run(const rulgnn_grucm_shape* s, const rulgnn_grucm_args* a, int mode, hipStream_t st);
int64_t hiercorrpool_param_count(const rulgnn_hiercorrpool_shape* s);
int64_t hiercorrpool_bn_state_count(const rulgnn_hiercorrpool_shape* s);
size_t hiercorrpool_workspace_bytes(const rulgnn_hiercorrpool_shape* s);
int64_t hiercorrpool_tap_offset(const rulgnn_hiercorrpool_shape* s, int which);
int hiercorrpool_run(const rulgnn_hiercorrpool_shape* s, const rulgnn_hiercorrpool_args* a, int mode, hipStream_t st);
int64_t logo_param_count(const rulgnn_logo_shape* s);
size_t logo_workspace_bytes(const rulgnn_logo_shape* s);
int64_t logo_tap_offset(const rulgnn_logo_shape* s, int which);
int logo_run(const rulgnn_logo_shape* s, const rulgnn_logo_args* a, int mode, hipStream_t st);
size_t rul_metrics_workspace_bytes(int64_t n);
int rul_metrics(const float* pred, const float* real, int64_t n, float max_rul, double* out, void* workspace, size_t workspace_bytes,
                hipStream_t st, int raw = 0);

}  // namespace rulgnn
