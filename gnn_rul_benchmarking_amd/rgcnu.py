"""Drop-in ``RGCNU_model`` (a ``GCNLayer`` user).  The whole model runs behind three C entries on one
flat parameter buffer (``rulgnn_rgcnu_{forward,backward,fwdbwd}_f32``; ``fused_mse_step`` is forward + MSE + backward + Adam in one
call): the learned adjacency, the per-(sample, time-step) graph convolutions, the 1x1 / 'same' convolutions and the two heads in the
gfx950 kernels of csrc/rgcnu.hip, the LSTM over the time steps in the persistent kernels of csrc/bilstm.hip (one direction).

Mirrors the reference class (models/RGCNU/Model.py:96-119): same constructor kwargs
``(num_nodes, time_length, hidden_dim, encoder_hidden_dim, kernel_size, alpha)``, ``forward(X, train=False)`` returning the
prediction ``[bs, 1]`` or ``(prediction, std)``, the same 22 ``state_dict`` keys and -- sub-modules being created in the reference's
order -- the same initial weights for a torch seed.  Reference quirk kept: graph (b, l) is convolved with the adjacency of sample
``(b * time_length + l) % bs`` (``A.repeat(time_length, 1, 1)`` against sample-major node signals, Model.py:104-106).
SCL's ``Dropout(0.5)`` uses the counter-based hash of the other families (mask = f(seed, step, element); torch's Bernoulli stream
cannot be reproduced by any other implementation).  There is no CPU path: a non-CUDA input raises.
"""
from __future__ import annotations

import torch.nn as nn

from . import _lib
from .flat import DropoutStepModule

SCL_DROPOUT = 0.5          # models/RGCNU/Model.py:31


# ---- parameter holders: created in the reference's order so that a seed gives the reference's initial weights; never called ----
class GCNLayer(nn.Module):
    def __init__(self, in_features, out_features):
        super().__init__()
        self.linear = nn.Linear(in_features, out_features)


class SCL(nn.Module):
    def __init__(self, hidden_dim):
        super().__init__()
        self.gcn1 = GCNLayer(1, hidden_dim)
        self.gcn2 = GCNLayer(hidden_dim, hidden_dim)
        self.conv1d = nn.Conv1d(hidden_dim, 1, kernel_size=1)
        self.dropout = nn.Dropout(p=SCL_DROPOUT)


class TDL(nn.Module):
    def __init__(self, num_nodes, encoder_hidden_dim):
        super().__init__()
        self.lstm = nn.LSTM(num_nodes, encoder_hidden_dim, batch_first=True)


class FusionModule(nn.Module):
    def __init__(self, num_nodes, encoder_hidden_dim, kernel_size, time_length):
        super().__init__()
        self.cnn1 = nn.Conv1d(num_nodes, encoder_hidden_dim, kernel_size=1)
        self.cnn2 = nn.Conv1d(encoder_hidden_dim, encoder_hidden_dim, kernel_size=kernel_size, padding='same')
        self.fc1 = nn.Linear(encoder_hidden_dim * time_length, 1)
        self.fc2 = nn.Linear(encoder_hidden_dim * time_length, 1)


class adj_construction(nn.Module):
    def __init__(self, num_nodes, time_length, alpha):
        super().__init__()
        self.alpha = alpha
        self.trainable_theta1 = nn.Linear(time_length, num_nodes)
        self.trainable_theta2 = nn.Linear(time_length, num_nodes)


PARAM_ORDER = ["adj.trainable_theta1.weight", "adj.trainable_theta1.bias", "adj.trainable_theta2.weight", "adj.trainable_theta2.bias",
               "scl.gcn1.linear.weight", "scl.gcn1.linear.bias", "scl.gcn2.linear.weight", "scl.gcn2.linear.bias",
               "scl.conv1d.weight", "scl.conv1d.bias",
               "tdl.lstm.weight_ih_l0", "tdl.lstm.weight_hh_l0", "tdl.lstm.bias_ih_l0", "tdl.lstm.bias_hh_l0",
               "fusion.cnn1.weight", "fusion.cnn1.bias", "fusion.cnn2.weight", "fusion.cnn2.bias",
               "fusion.fc1.weight", "fusion.fc1.bias", "fusion.fc2.weight", "fusion.fc2.bias"]


class RGCNU_model(DropoutStepModule):
    # graph (b, l) meets the adjacency of sample (b * T + l) % bs: the eval forward depends on WHICH samples share a batch, so a test
    # set must be walked in the reference's batches on every rank, never re-batched per shard (trainer.py / dataloader.data_generator)
    eval_sample_independent = False

    def __init__(self, num_nodes, time_length, hidden_dim, encoder_hidden_dim, kernel_size, alpha):
        super().__init__()
        self.num_nodes, self.time_length = int(num_nodes), int(time_length)
        self.hidden_dim, self.encoder_hidden_dim, self.kernel_size = int(hidden_dim), int(encoder_hidden_dim), int(kernel_size)
        self.alpha = float(alpha)
        self.adj = adj_construction(self.num_nodes, self.time_length, alpha)
        self.scl = SCL(self.hidden_dim)
        self.tdl = TDL(self.num_nodes, self.encoder_hidden_dim)
        self.fusion = FusionModule(self.num_nodes, self.encoder_hidden_dim, self.kernel_size, self.time_length)
        if [n for n, _ in self.named_parameters()] != PARAM_ORDER:
            raise RuntimeError("parameter order differs from the flat layout of include/rulgnn.h")
        self._init_flat()
        # fusion.fc2 (the `std` head) is not in the loss: its gradient is None in the reference and torch's Adam never touches it
        self.num_optimized = self._layout["fusion.fc2.weight"][0]

    flat_order = PARAM_ORDER
    workspace_slots = 4
    output_buffers = 2         # prediction, std head
    consumes_tape = True       # the backward reworks the gate tape in place: one backward per forward
    empty_batch = "RGCNU_model: empty batch"

    # ---- C-ABI calls -----------------------------------------------------------------------------------
    c_family, Args = "rgcnu", _lib.RgcnuArgs
    not_covered = ("RGCNU HIP kernels do not cover this configuration (num_nodes <= 32, time_length <= 64, hidden widths <= 64, odd "
                   "kernel_size <= 7)")

    def _shape(self, batch):
        return _lib.RgcnuShape(batch, self.num_nodes, self.time_length, self.hidden_dim, self.encoder_hidden_dim, self.kernel_size, self.alpha)

    def _check_input(self, x):
        if x.dim() != 3 or x.size(1) != self.num_nodes or x.size(2) != self.time_length:
            raise RuntimeError(f"RGCNU_model expects [bs, {self.num_nodes}, {self.time_length}], got {tuple(x.shape)}")
        self._require_device(x)
        return x.contiguous().float()

    @property
    def dropout_p(self):           # read at every call: SCL's nn.Dropout holds the rate
        return float(self.scl.dropout.p)

    def _args(self, shp, x, training, step, y=None, dpred=None, global_batch=None, sample_offset=0):
        a = super()._args(shp, x, training, step, y, dpred, global_batch, sample_offset)
        a.std_pred = self._out_bufs[1].data_ptr()
        return a

    # ---- nn.Module surface -----------------------------------------------------------------------------
    def forward(self, X, train=False):
        """``train`` selects the return value like the reference (Model.py:115-118); dropout follows ``self.training``."""
        # the second head is returned detached: its only consumer in the reference is a commented-out loss (algorithms.py:288)
        pred, std = self._forward_outputs(X)
        return (pred, std.detach()) if train else pred
