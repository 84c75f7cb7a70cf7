"""Drop-in ``ASTGCNN_model`` whose forward/backward run in the gfx950 HIP kernels (csrc/astgcnn.hip).

Mirrors the reference class (models/ASTGCNN/Model.py:233-254): same constructor kwargs
``(num_nodes, time_length, encoder_out_dim, output_dim, K)``, same ``forward(X) -> [bs, 1]``, the same 29
``state_dict`` keys (including the never-called ``tcn.net0`` / ``tcn.net1`` branches, Model.py:86-109) and -- because the
parameter-holding sub-modules are created in the reference's order -- the same initial weights for a torch seed.  None of
the sub-modules is ever *called*: the live parameters are views into one flat fp32 buffer that the kernels read directly
(layout in include/rulgnn.h), the BatchNorm running statistics views into a second one.

There is no CPU path: calling the model with a non-CUDA tensor raises.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from . import _lib, params as PL
from .flat import FlatModule, current_stream as _stream
from .stgcn import TemporalConvNet

TCN_KERNEL = 6          # Model.py:236


class GatingMechanism(nn.Module):
    """Holder of ``theta`` = Linear(time_length, encoder_out_dim) and ``bias`` (Model.py:169-173)."""

    def __init__(self, num_channels, out_channels):
        super().__init__()
        self.theta = nn.Linear(num_channels, out_channels)
        self.bias = nn.Parameter(torch.zeros(out_channels))


class construct_graph(nn.Module):
    """Holder of ``P`` = Linear(f, f, bias=False) (Model.py:184-187)."""

    def __init__(self, num_features):
        super().__init__()
        self.P = nn.Linear(num_features, num_features, bias=False)


class ChebNet(nn.Module):
    """Holder of ``filters`` [K, in, out], xavier-uniform (Model.py:198-209)."""

    def __init__(self, in_channels, out_channels, K):
        super().__init__()
        self.filters = nn.Parameter(torch.Tensor(K, in_channels, out_channels))
        nn.init.xavier_uniform_(self.filters)


def live_layout(num_nodes, time_length, output_dim, K):
    """state_dict name (without the algorithm's ``model.`` prefix) -> (offset, shape) in the flat buffer."""
    N, T, E, O = num_nodes, time_length, time_length, output_dim
    out, off = {}, 0
    for name, shape in (("tcn.conv_block1.0.weight", (N, N, TCN_KERNEL)), ("tcn.conv_block1.2.weight", (N,)),
                        ("tcn.conv_block1.2.bias", (N,)), ("tcn.conv_block2.0.weight", (N, N, TCN_KERNEL)),
                        ("tcn.conv_block2.2.weight", (N,)), ("tcn.conv_block2.2.bias", (N,)),
                        ("gate.theta.weight", (E, T)), ("gate.theta.bias", (E,)), ("gate.bias", (E,)),
                        ("distance_module.P.weight", (E, E)), ("chebnet.filters", (K, E, O)), ("fc.weight", (1, O)),
                        ("fc.bias", (1,))):
        n = 1
        for s in shape:
            n *= s
        out[name] = (off, shape)
        off += n
    return out, off


class ASTGCNN_model(FlatModule):
    def __init__(self, num_nodes, time_length, encoder_out_dim, output_dim, K):
        super().__init__()
        self.num_nodes, self.time_length = int(num_nodes), int(time_length)
        self.encoder_out_dim, self.output_dim, self.K = int(encoder_out_dim), int(output_dim), int(K)
        # same construction order as the reference => same RNG consumption => same initial weights
        self.tcn = TemporalConvNet(self.num_nodes, [self.num_nodes, self.num_nodes], kernel_size=TCN_KERNEL)
        self.gate = GatingMechanism(self.time_length, self.encoder_out_dim)
        self.distance_module = construct_graph(self.encoder_out_dim)
        self.chebnet = ChebNet(self.encoder_out_dim, self.output_dim, self.K)
        self.fc = nn.Linear(self.output_dim, 1)

        # (off by default: with the step's five parameter-gradient products as one launch pair behind the backward chain, one stream is
        # faster -- 0.119 vs 0.122 ms per step at N-CMAPSS batch 512; ``enabled = True`` runs the pair beside the TCN backward instead)
        self.side_stream = PL.SideStream()
        self.side_stream.enabled = False
        self._track_batchnorm_counters()
        self._init_flat(*live_layout(self.num_nodes, self.time_length, self.output_dim, self.K))

    # ---- flat storage ----------------------------------------------------------------------------------
    workspace_slots = 4
    bn_modules = ("tcn.conv_block1.2", "tcn.conv_block2.2")

    # ---- C-ABI calls -----------------------------------------------------------------------------------
    c_family, Args = "astgcnn", _lib.AstgcnnArgs
    not_covered = "ASTGCNN kernels do not cover this configuration (num_nodes <= 25, time_length <= 64, output_dim <= 256, K <= 3)"

    def _shape(self, batch):
        if self.encoder_out_dim != self.time_length:
            raise RuntimeError(f"The size of tensor a ({self.encoder_out_dim}) must match the size of tensor b "
                               f"({self.time_length}) at non-singleton dimension 2")      # what the reference's gate raises
        return _lib.AstgcnnShape(batch, self.num_nodes, self.time_length, self.output_dim, self.K)

    def _check_input(self, x):
        self._require_device(x)
        if x.dim() != 3 or x.size(1) != self.num_nodes or x.size(2) != self.time_length:
            raise RuntimeError(f"expected input [bs, {self.num_nodes}, {self.time_length}], got {list(x.shape)}")
        return x.reshape(x.size(0), -1).contiguous().float()

    def _args(self, shp, x2d, training, y=None, dpred=None, global_batch=None, moments_to_bucket=False):
        a = super()._args(shp, x2d, y, dpred, global_batch)
        self._bn_args(a, x2d.size(0), moments_to_bucket)
        a.training = 1 if training else 0
        a.aux_stream = self.side_stream.pointer(self._flat.device, training)
        return a

    def _after_train_forward(self, batch, from_bucket_moments=False, from_bucket_stats=False):
        """BatchNorm side effects of a training forward (running stats, num_batches_tracked).  ``from_bucket_moments``: the bucket
        tail holds the all-reduced (E[z], E[z^2]) (local BatchNorm); ``from_bucket_stats``: the global (mean, var) (synchronised)."""
        src = self._bn_source(from_bucket_moments or from_bucket_stats)
        shp = self._shape(batch)
        _lib.check(_lib.load().rulgnn_astgcnn_bn_running_update_f32(C.byref(shp), self._bn.data_ptr(), src,
                                                                    batch * self.time_length, 0.1,
                                                                    1 if from_bucket_moments else 0, _stream()),
                   "rulgnn_astgcnn_bn_running_update_f32")
        self._nbt_pending += 1

    def fused_mse_step(self, x, y, optimizer=None, global_batch=None, sample_offset=0, update_running_stats=True,
                       moments_to_bucket=False):
        """train forward + MSE + backward (+ Adam and the running-statistics update when ``optimizer`` is a FusedAdam over
        this model) in one C call; fills ``self.bucket``; returns (pred [B], loss 0-d tensor) on the device."""
        return self._bn_fused_mse_step(x, y, optimizer, global_batch, update_running_stats, moments_to_bucket)

    def sync_bn_schedule(self):
        """float64 counts of the all-reduces one synchronised-BatchNorm step issues, in order (dp.py: a rank with an empty shard joins
        them with zeros)."""
        return [50] * 4

    def fused_mse_step_syncbn(self, x, y, global_batch, sample_offset, bn_param_grad_scale, allreduce):
        """See ``FlatModule._syncbn_step`` (rulgnn_astgcnn_fwdbwd_syncbn_f32)."""
        return self._syncbn_step("rulgnn_astgcnn_fwdbwd_syncbn_f32", x, y, global_batch, bn_param_grad_scale, allreduce)

    # ---- nn.Module surface -----------------------------------------------------------------------------
    def forward(self, X):
        return self._bn_forward(X)
