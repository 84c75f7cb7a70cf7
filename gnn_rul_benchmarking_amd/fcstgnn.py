"""Drop-in ``FC_STGNN_RUL`` whose forward/backward run in the gfx950 HIP kernels (csrc/fcstgnn.hip).

Mirrors the reference class (models/FC_STGNN/Model.py:5-84): same ten constructor kwargs, same ``forward(X) -> [bs, 1]``,
the same 56 ``state_dict`` keys (seven BatchNorms with their buffers, the ``positional_encoding.pe`` table buffer
``[1, 5000, 2*hidden_dim]``) in the same order and -- because the parameter-holding sub-modules are created in the
reference's order -- the same initial weights for a torch seed.  None of the sub-modules is ever *called*: parameters are
views into one flat fp32 buffer that the kernels read directly (layout in include/rulgnn.h), the BatchNorm running
statistics views into a second one.

The positional-encoding dropout (p = 0.1 in train mode, Model.py:25) uses the package's counter-based hash stream
(seed, step, element index) instead of torch's Bernoulli stream; everything else is the reference's arithmetic.

There is no CPU path: calling the model with a non-CUDA tensor raises.
"""
from __future__ import annotations

import ctypes as C
import math
from collections import OrderedDict

import torch
import torch.nn as nn

from . import _lib, params as PL
from .flat import FlatModule, current_stream as _stream

PE_DROPOUT = 0.1


class Feature_extractor_1DCNN_RUL(nn.Module):
    """Holder of the two conv blocks (Model_Base.py:12-30)."""

    def __init__(self, input_channels, num_hidden, out_dim, kernel_size=8, stride=1, dropout=0):
        super().__init__()
        self.conv_block1 = nn.Sequential(
            nn.Conv1d(input_channels, num_hidden, kernel_size=kernel_size, stride=stride, bias=False, padding=(kernel_size // 2)),
            nn.BatchNorm1d(num_hidden), nn.ReLU(), nn.Dropout(dropout))
        self.conv_block2 = nn.Sequential(
            nn.Conv1d(num_hidden, out_dim, kernel_size=kernel_size, stride=1, bias=False, padding=1),
            nn.BatchNorm1d(out_dim), nn.ReLU())


class PositionalEncoding(nn.Module):
    """Holder of the ``pe`` buffer (Model_Base.py:111-125; base 100)."""

    def __init__(self, d_model, dropout, max_len=5000):
        super().__init__()
        self.dropout = nn.Dropout(p=dropout)
        pe = torch.zeros(max_len, d_model)
        position = torch.arange(0, max_len).unsqueeze(1)
        div_term = torch.exp(torch.arange(0, d_model, 2) * -(math.log(100.0) / d_model))
        pe[:, 0::2] = torch.sin(position * div_term)
        pe[:, 1::2] = torch.cos(position * div_term)
        self.register_buffer('pe', pe.unsqueeze(0))


class Dot_Graph_Construction_weights(nn.Module):
    def __init__(self, input_dim):
        super().__init__()
        self.mapping = nn.Linear(input_dim, input_dim)


class MPNN_mk_v2(nn.Module):
    def __init__(self, input_dimension, outpuut_dinmension, k):
        super().__init__()
        self.k = k
        self.theta = nn.ModuleList([nn.Linear(input_dimension, outpuut_dinmension) for _ in range(k)])
        self.bn1 = nn.BatchNorm1d(outpuut_dinmension)


class GraphConvpoolMPNN_block_v6(nn.Module):
    def __init__(self, input_dim, output_dim, num_sensors, time_length, time_window_size, stride, decay, pool_choice):
        super().__init__()
        self.graph_construction = Dot_Graph_Construction_weights(input_dim)
        self.BN = nn.BatchNorm1d(input_dim)
        self.MPNN = MPNN_mk_v2(input_dim, output_dim, k=1)


BN_NAMES = ("nonlin_map.conv_block1.1", "nonlin_map.conv_block2.1", "nonlin_map2.1", "MPNN1.BN", "MPNN1.MPNN.bn1", "MPNN2.BN",
            "MPNN2.MPNN.bn1")


class FC_STGNN_RUL(FlatModule):
    def __init__(self, patch_size, num_patch, encoder_time_out, encoder_hidden_dim, encoder_out_dim, encoder_conv_kernel,
                 hidden_dim, num_sequential, num_node, num_windows):
        super().__init__()
        self.cfg = dict(patch_size=int(patch_size), num_patch=int(num_patch), encoder_time_out=int(encoder_time_out),
                        encoder_hidden_dim=int(encoder_hidden_dim), encoder_out_dim=int(encoder_out_dim),
                        encoder_conv_kernel=int(encoder_conv_kernel), hidden_dim=int(hidden_dim),
                        num_sequential=int(num_sequential), num_node=int(num_node), num_windows=int(num_windows))
        self.patch_size, self.num_patch = int(patch_size), int(num_patch)
        # same construction order as the reference (Model.py:20-43) => same RNG consumption => same initial weights
        self.nonlin_map = Feature_extractor_1DCNN_RUL(1, encoder_hidden_dim, encoder_out_dim, kernel_size=encoder_conv_kernel)
        self.nonlin_map2 = nn.Sequential(nn.Linear(encoder_out_dim * encoder_time_out, 2 * hidden_dim), nn.BatchNorm1d(2 * hidden_dim))
        self.positional_encoding = PositionalEncoding(2 * hidden_dim, PE_DROPOUT, max_len=5000)
        self.MPNN1 = GraphConvpoolMPNN_block_v6(2 * hidden_dim, hidden_dim, num_node, num_sequential, 2, 1, 0.7, 'mean')
        self.MPNN2 = GraphConvpoolMPNN_block_v6(2 * hidden_dim, hidden_dim, num_node, num_sequential, 2, 2, 0.7, 'mean')
        self.fc = nn.Sequential(OrderedDict([
            ('fc1', nn.Linear(hidden_dim * num_windows * num_node, 2 * hidden_dim)), ('relu1', nn.ReLU(inplace=True)),
            ('fc2', nn.Linear(2 * hidden_dim, 2 * hidden_dim)), ('relu2', nn.ReLU(inplace=True)),
            ('fc3', nn.Linear(2 * hidden_dim, hidden_dim)), ('relu3', nn.ReLU(inplace=True)),
            ('fc4', nn.Linear(hidden_dim, 1))]))

        self.side_stream = PL.SideStream()
        self._step = 0
        self._seed = int(torch.initial_seed()) & 0xFFFFFFFFFFFFFFFF
        self.dropout_p = PE_DROPOUT
        # "f32" (default; meets the 1e-4 parity gate) or "bf16": bf16 operands on every product of the window-graph kernels (forward and
        # backward: v_mfma_f32_32x32x16_bf16) and on the row-projection GEMMs; fp32 accumulation / softmax / BatchNorm / weight gradients /
        # optimizer -- BASELINE.json's "FC_STGNN ... bf16" variant, reported separately (rulgnn.h: rulgnn_fcstgnn_args.compute_dtype)
        self.compute_dtype = "f32"
        self._track_batchnorm_counters()
        self._init_flat()                   # flat layout = named_parameters() order (the order include/rulgnn.h documents)
        lib_count = _lib.load().rulgnn_fcstgnn_param_count(C.byref(self._shape(1)))
        if lib_count >= 0 and lib_count != self._count:
            raise RuntimeError(f"flat parameter layout mismatch: module {self._count} vs kernels {lib_count}")

    # ---- flat storage ----------------------------------------------------------------------------------
    workspace_slots = 4
    bn_modules = BN_NAMES

    # ---- C-ABI calls -----------------------------------------------------------------------------------
    c_family, Args = "fcstgnn", _lib.FcstgnnArgs
    not_covered = ("FC_STGNN kernels do not cover this configuration (encoder_time_out must be the second conv's output length, "
                   "num_windows the windows of the two blocks; num_node <= 20, hidden_dim <= 32, encoder_out_dim <= 64, "
                   "encoder_hidden_dim <= 16, encoder_conv_kernel <= 4)")

    def _shape(self, batch):
        c = self.cfg
        return _lib.FcstgnnShape(batch, c["patch_size"], c["num_patch"], c["encoder_time_out"], c["encoder_hidden_dim"],
                                 c["encoder_out_dim"], c["encoder_conv_kernel"], c["hidden_dim"], c["num_sequential"], c["num_node"],
                                 c["num_windows"])

    def _check_input(self, x):
        self._require_device(x)
        c = self.cfg
        if x.dim() != 3 or x.size(1) != c["num_node"] or x.size(2) != c["num_patch"] * c["patch_size"]:
            raise RuntimeError(f"shape '[{x.size(0)}, {c['num_node']}, {c['num_patch']}, {c['patch_size']}]' is invalid for input "
                               f"of size {x.numel()}")
        return x.reshape(x.size(0), -1).contiguous().float()

    def _args(self, shp, x2d, training, step, y=None, dpred=None, global_batch=None, sample_offset=0, moments_to_bucket=False):
        a = super()._args(shp, x2d, y, dpred, global_batch)
        self._bn_args(a, x2d.size(0), moments_to_bucket)
        a.sample_offset = int(sample_offset)
        a.dropout_p = float(self.dropout_p)
        a.seed = self._seed
        a.step = int(step)
        a.training = 1 if training else 0
        a.step_state = self._step_state.data_ptr() if self._step_state is not None else None
        a.aux_stream = self.side_stream.pointer(self._flat.device, training)       # the backward's weight / bias gradient GEMMs
        if self.compute_dtype not in ("f32", "bf16"):
            raise RuntimeError(f"compute_dtype must be 'f32' or 'bf16', not {self.compute_dtype!r}")
        a.compute_dtype = _lib.DTYPE_BF16 if self.compute_dtype == "bf16" else _lib.DTYPE_F32
        return a

    def _after_train_forward(self, batch, from_bucket_moments=False, from_bucket_stats=False):
        """BatchNorm side effects of a training forward.  ``batch``: the (global) batch the statistics were taken over.
        ``from_bucket_moments``: the bucket tail holds the all-reduced (E[z], E[z^2]) (local BatchNorm); ``from_bucket_stats``: it
        holds the global (mean, var) (synchronised)."""
        src = self._bn_source(from_bucket_moments or from_bucket_stats)
        shp = self._shape(int(batch))
        _lib.check(_lib.load().rulgnn_fcstgnn_bn_running_update_f32(C.byref(shp), self._bn.data_ptr(), src, 0.1,
                                                                    1 if from_bucket_moments else 0, _stream()),
                   "rulgnn_fcstgnn_bn_running_update_f32")
        self._nbt_pending += 1

    def _forward_state(self, training):
        """(training, dropout step): a training forward draws the next step."""
        if not training:
            return False, 0
        self._step += 1
        return True, self._step

    def fused_mse_step(self, x, y, optimizer=None, global_batch=None, sample_offset=0, update_running_stats=True,
                       moments_to_bucket=False):
        """train forward + MSE + backward (+ Adam and the running statistics with ``optimizer``) in one C call."""
        return self._bn_fused_mse_step(x, y, optimizer, global_batch, update_running_stats, moments_to_bucket,
                                       sample_offset=sample_offset)

    def sync_bn_schedule(self):
        """float64 counts of the all-reduces one synchronised-BatchNorm step issues, in order (dp.py: a rank with an empty shard joins
        them with zeros)."""
        return [128] * 14

    def fused_mse_step_syncbn(self, x, y, global_batch, sample_offset, bn_param_grad_scale, allreduce):
        """See ``FlatModule._syncbn_step`` (rulgnn_fcstgnn_fwdbwd_syncbn_f32)."""
        return self._syncbn_step("rulgnn_fcstgnn_fwdbwd_syncbn_f32", x, y, global_batch, bn_param_grad_scale, allreduce,
                                 sample_offset=sample_offset)

    # ---- nn.Module surface -----------------------------------------------------------------------------
    def forward(self, X):
        return self._bn_forward(X)
