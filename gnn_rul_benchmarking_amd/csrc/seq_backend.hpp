// The back end STNet, GDAGDL, GAT_LSTM and STFA end in (csrc/seq_backend.hip): an optional 4 + 4 Linear / ReLU auto-encoder over the patch rows
// with its reconstruction term, unidirectional LSTMs over the patches (bilstm.hip, one direction), Linear(H * T, 1) -- or Linear(H, 1) over
// the last step (LstmHeadPlan::last_step) -- with the MSE.  A
// family's geometry embeds the plans and lays them out from its own running parameter (`o`) and workspace (`w`: floats, 64-float granules)
// counters; what differs between the families (which sums make the loss, which buffers the gradient walks through) stays with the caller.
#pragma once
#include "sgemm_mfma.hpp"
#include "families_host.hpp"

namespace rulgnn {

constexpr int SEQ_MAX_LSTM = 3;

// C = A B^T (strides as sgemm): a short product over a long reduction (K >= 512, fewer than 128 output tiles: [BT x 900] x [900 x 50]
// is 32 tiles walking all of K alone, 45 us) is split over k (6 us + a 6-us fixed-order sum), anything else is the plain SGEMM.  The two
// paths sum in different orders: which products come here is part of a family's bits.
[[nodiscard]] int gemm_rows(const float* A, int64_t sAm, int64_t sAk, const float* B, int64_t sBn, int64_t sBk, float* C, int64_t ldc, int M, int N, int K,
              float* split, hipStream_t st);
// `p`, or its copy at `slot` (enqueued on `st`; nullptr when that fails) when p is off a 16-byte boundary: the large-tile GEMM (16-byte
// vector loads) falls back to the 64 x 64 fp32 tiles for a misaligned operand -- 123 instead of 98 us for STNet's [18 000 x 900] x
// [900 x 200] -- and the flat parameter buffer puts most weights behind odd-sized tensors.
const float* aligned_operand(const float* p, size_t count, float* slot, hipStream_t st);
// Backward of y = h W^T + b over `rows` rows, d = dy: gw = d^T h and gb = sum_rows d (split-K, gb against `one`), then dn = d W by the
// GEMM the caller names (the choice changes the summation order).
enum DenseData { DENSE_NO_DATA, DENSE_PLAIN, DENSE_ROWS };          // no data gradient / sgemm / gemm_rows
[[nodiscard]] int dense_backward(const float* d, const float* h, const float* W, const float* one, float* gw, float* gb, DenseData data, float* dn, int rows,
                   int out, int in, float* split, hipStream_t st);
[[nodiscard]] int sum_pair(const float* a, const float* b, float* out, hipStream_t st);          // out[0] = a[0] + b[0]
// One direction of bilstm.hip over T steps of B sequences, I -> E wide, parameters at flat offsets o = {w_ih, w_hh, b_ih, b_hh} of `prm`
// (and of `grads`; null with dout and dx for a forward alone).  Slot [1] mirrors [0] (unused).
void lstm_uni_args(rulgnn_bilstm_shape* ls, rulgnn_bilstm_args* la, int T, int64_t B, int I, int E, const float* x, float* out, float* lstm_ws,
                   const float* prm, const int o[4], float* grads = nullptr, const float* dout = nullptr, float* dx = nullptr);

struct LstmHeadPlan {
    int64_t B;
    int T, nk, H[SEQ_MAX_LSTM + 1];              // nk layers, H[k] -> H[k + 1] wide; the head reads H[nk] * T values per sample
    int last_step = 0;                           // != 0: the head is Linear(H[nk], 1) over the last step alone (STFA: fc(lstm_output[:, -1, :]))
    int o_lstm[SEQ_MAX_LSTM][4], o_lw, o_lb;     // flat parameter offsets: {w_ih, w_hh, b_ih, b_hh} per layer, linear.{weight, bias}
    int64_t w_hseq[SEQ_MAX_LSTM], w_lstm[SEQ_MAX_LSTM], w_dpred, w_sq, w_one;      // workspace (floats); w_one: 64 floats, [0] = 1 in a backward
};
// B, T, nk, H are set: takes parameters and workspace regions, registers the head's split-K products; EUNSUPPORTED where bilstm.hip refuses
[[nodiscard]] int lstm_head_layout(LstmHeadPlan* p, int* o, int64_t* w, SplitKScratch* sp);
// x [B * T][H[0]] -> the layers -> pred [B]; with y, the squared-error terms / global batch in w_sq and d loss / d pred in w_dpred
[[nodiscard]] int lstm_head_forward(const LstmHeadPlan& p, const float* x, const float* prm, float* ws, const float* y, float* pred, float inv_gb, hipStream_t st);
// linear.{weight, bias} gradients, d hseq into dbuf[0] (zero before the last step under last_step), then down the layers from one buffer into the other: d x is left in dbuf[nk & 1]
[[nodiscard]] int lstm_head_backward(const LstmHeadPlan& p, const float* x, const float* prm, float* ws, const float* dpred, float* grads, float* const dbuf[2],
                       float* split, hipStream_t st);

struct AutoEncoderPlan {
    int64_t BT;                                  // patch rows
    int ein[4], eout[4], din[4], dout[4];        // Linear widths; ein[0] = dout[3] = D, ReLU behind all but the last of each half
    int o_enc_w[4], o_enc_b[4], o_dec_w[4], o_dec_b[4];
    int64_t w_enc[4], w_dec[4], w_rsq, w_dD1, w_dD2, w_dA1, w_dA2, w_dH;
    int rblocks;                                 // workgroups of the reconstruction-error kernel (= partial sums)
};
// BT and the widths are set: takes parameters and workspace regions, registers every split-K product of the two passes
void autoencoder_layout(AutoEncoderPlan* p, int* o, int64_t* w, SplitKScratch* sp);
// yo [BT][D] -> encoder (output w_enc[3]: the LSTM's input) -> decoder; recon_sum[0] = mean over the GLOBAL batch of (yo - yp)^2 (rscale =
// 1 / its element count), the term's gradients w.r.t. yp and yo in w_dD1 / w_dD2
[[nodiscard]] int autoencoder_forward(const AutoEncoderPlan& p, const float* yo, const float* prm, float* ws, float rscale, float* recon_sum, float* split,
                        hipStream_t st);
// w_dH holds the LSTM path's d (encoder output); recon_weight (device, may be null) scales the reconstruction gradients.  d yo: w_dD1.
[[nodiscard]] int autoencoder_backward(const AutoEncoderPlan& p, const float* yo, const float* prm, float* ws, float* grads, const float* one,
                         const float* recon_weight, float* split, hipStream_t st);

}  // namespace rulgnn
