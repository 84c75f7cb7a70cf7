"""Drop-in ``ST_Conv_model`` whose forward/backward run in the gfx950 HIP kernels (csrc/stconv.hip).

Mirrors the reference class (models/ST_Conv/Model.py:173-222): same constructor kwargs ``(num_nodes, time_length,
kernel_size)``, same ``forward(x) -> [bs, 1]``, the same ``state_dict`` keys in the same order -- including the "_2" layers
and the TCN's ``net0``/``net1`` branches that the reference's forward never calls (Model.py:196-206 uses the "_1" modules for
both branches) -- and the same initial weights for a torch seed.  None of the sub-modules is ever *called*: the live
parameters are views into one flat fp32 buffer that the kernels read directly (layout in include/rulgnn.h), the three live
BatchNorms' running statistics views into a second one; like in the reference each of them advances twice per training
forward.

There is no CPU path: calling the model with a non-CUDA tensor raises.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from . import _lib
from .flat import FlatModule, current_stream as _stream
from .stgcn import MPNN_mk, TemporalConvNet

LIVE = ("theta1", "theta2", "theta3", "theta4", "gcn_layer_1.theta.0.weight", "gcn_layer_1.theta.0.bias",
        "cnn_layer_1.conv.weight", "cnn_layer_1.conv.bias", "cnn_layer_1.bn.weight", "cnn_layer_1.bn.bias",
        "tcn_layer_1.conv_block1.0.weight", "tcn_layer_1.conv_block1.2.weight", "tcn_layer_1.conv_block1.2.bias",
        "tcn_layer_1.conv_block2.0.weight", "tcn_layer_1.conv_block2.2.weight", "tcn_layer_1.conv_block2.2.bias",
        "fc.weight", "fc.bias")
BN_NAMES = ("tcn_layer_1.conv_block1.2", "tcn_layer_1.conv_block2.2", "cnn_layer_1.bn")


class CNNLayer(nn.Module):
    """Holder of ``conv`` = Conv1d(padding='same') and ``bn`` (Model.py:58-63)."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1):
        super().__init__()
        self.conv = nn.Conv1d(in_channels, out_channels, kernel_size=kernel_size, padding='same', stride=stride)
        self.bn = nn.BatchNorm1d(out_channels)


class ST_Conv_model(FlatModule):
    def __init__(self, num_nodes, time_length, kernel_size):
        super().__init__()
        self.num_nodes, self.time_length, self.kernel_size = int(num_nodes), int(time_length), int(kernel_size)
        # same construction order as the reference (Model.py:176-190) => same RNG consumption => same initial weights
        self.gcn_layer_1 = MPNN_mk(time_length, time_length, k=1)
        self.cnn_layer_1 = CNNLayer(num_nodes, num_nodes, kernel_size)
        self.tcn_layer_1 = TemporalConvNet(num_nodes, [num_nodes, num_nodes], kernel_size)
        self.gcn_layer_2 = MPNN_mk(time_length, time_length, k=1)
        self.cnn_layer_2 = CNNLayer(num_nodes, num_nodes, kernel_size)
        self.tcn_layer_2 = TemporalConvNet(num_nodes, [num_nodes, num_nodes], kernel_size)
        self.theta1 = nn.Parameter(torch.randn(1))
        self.theta2 = nn.Parameter(torch.randn(1))
        self.theta3 = nn.Parameter(torch.randn(1))
        self.theta4 = nn.Parameter(torch.randn(1))
        self.fc = nn.Linear(num_nodes * time_length, 1)

        self._track_batchnorm_counters()
        self._init_flat()

    # ---- flat storage ----------------------------------------------------------------------------------
    flat_order = LIVE                                                  # the parameters the forward uses; the rest stay ordinary tensors
    workspace_slots = 4
    bn_modules = BN_NAMES

    def _flush_nbt(self):
        if self._nbt_pending and self._nbt is not None:
            self._nbt += 2 * self._nbt_pending          # every live BatchNorm runs twice per training forward (Model.py:196-206)
            self._nbt_pending = 0

    # ---- C-ABI calls -----------------------------------------------------------------------------------
    c_family, Args = "stconv", _lib.AstgcnnArgs
    not_covered = "ST_Conv kernels do not cover this configuration (kernel_size 6, num_nodes <= 25, time_length <= 64)"

    def _shape(self, batch):
        return _lib.StconvShape(batch, self.num_nodes, self.time_length, self.kernel_size)

    def _check_input(self, x):
        self._require_device(x)
        if x.dim() != 3 or x.size(1) != self.num_nodes or x.size(2) != self.time_length:
            raise RuntimeError(f"expected input [bs, {self.num_nodes}, {self.time_length}], got {list(x.shape)}")
        return x.reshape(x.size(0), -1).contiguous().float()

    def _args(self, shp, x2d, training, y=None, dpred=None, global_batch=None, moments_to_bucket=False):
        a = super()._args(shp, x2d, y, dpred, global_batch)
        self._bn_args(a, x2d.size(0), moments_to_bucket)
        a.training = 1 if training else 0
        return a

    def _after_train_forward(self, batch, from_bucket_moments=False):
        src = self._bn_source(from_bucket_moments)
        shp = self._shape(batch)
        _lib.check(_lib.load().rulgnn_stconv_bn_running_update_f32(C.byref(shp), self._bn.data_ptr(), src, batch * self.time_length,
                                                                   0.1, 1 if from_bucket_moments else 0, _stream()),
                   "rulgnn_stconv_bn_running_update_f32")
        self._nbt_pending += 1

    def fused_mse_step(self, x, y, optimizer=None, global_batch=None, sample_offset=0, update_running_stats=True,
                       moments_to_bucket=False):
        """train forward + MSE + backward (+ Adam and the running statistics with ``optimizer``) in one C call."""
        return self._bn_fused_mse_step(x, y, optimizer, global_batch, update_running_stats, moments_to_bucket)

    # ---- nn.Module surface -----------------------------------------------------------------------------
    def forward(self, x):
        return self._bn_forward(x)
