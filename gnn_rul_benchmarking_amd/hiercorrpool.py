"""Drop-in ``HierCorrPool_model``.  The whole model runs behind three C entries on one flat parameter buffer
(``rulgnn_hiercorrpool_{forward,backward,fwdbwd}_f32``; ``fused_mse_step`` is train-mode forward + MSE + backward + Adam in one call)
in the gfx950 kernels of csrc/hiercorrpool.hip: a three-block 1-D CNN encoder whose k = 8 convolutions are matrix-core products on a
channel-last, time-padded layout (train-mode BatchNorm differentiated through its batch statistics, ReLU, max-pool and dropout fused
into one pass per block), then a per-sample graph stage -- correlation graph, soft cluster assignment, coarsening -- that keeps every
N x N and N x d intermediate in LDS, and the message-passing layer and head on the shared SGEMM.

Mirrors the reference class (models/HierCorrPool/Model.py:6-52): same constructor ``(patch_size, num_patch, input_dim, hidden_dim,
embedding_dim, num_nodes, encoder_conv_kernel, num_nodes_out)`` (``input_dim`` is accepted and unused, as there), ``forward(x) -> [bs,
1]``, the same 28 ``state_dict`` keys in the same order (19 parameters, nine BatchNorm buffers) and -- sub-modules being created in the
reference's order -- the same initial weights for a torch seed.  ``model.train()`` uses batch statistics, updates the running ones
(momentum 0.1, unbiased variance, ``num_batches_tracked``) and draws dropout (``dropout_p``, 0.35) from the package's counter hash;
``model.eval()`` uses the running statistics and no dropout.  There is no CPU path: a non-CUDA input raises.

The reference's forward fails inside a reshape when ``L' * 4 * hidden_dim != encoder_conv_kernel * embedding_dim`` (L' = the encoder's
output length); here such a configuration raises at construction and names both numbers.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib
from .flat import DropoutStepModule


def encoder_lengths(num_patch):
    """Output lengths of the three encoder blocks: Conv1d(k 8, padding 4) L -> L + 1, MaxPool1d(2, 2, padding 1) -> (L + 1) // 2 + 1."""
    out, L = [], int(num_patch)
    for _ in range(3):
        L = (L + 1) // 2 + 1
        out.append(L)
    return out


class Feature_extractor_1DCNN(nn.Module):
    def __init__(self, input_channels, num_hidden, kernel_size, stride, dropout):
        super().__init__()
        self.conv_block1 = nn.Sequential(nn.Conv1d(input_channels, num_hidden, kernel_size=kernel_size, stride=stride, bias=False,
                                                   padding=kernel_size // 2),
                                         nn.BatchNorm1d(num_hidden), nn.ReLU(), nn.MaxPool1d(kernel_size=2, stride=2, padding=1), nn.Dropout(dropout))
        self.conv_block2 = nn.Sequential(nn.Conv1d(num_hidden, num_hidden * 2, kernel_size=8, stride=1, bias=False, padding=4),
                                         nn.BatchNorm1d(num_hidden * 2), nn.ReLU(), nn.MaxPool1d(kernel_size=2, stride=2, padding=1))
        self.conv_block3 = nn.Sequential(nn.Conv1d(num_hidden * 2, num_hidden * 4, kernel_size=8, stride=1, bias=False, padding=4),
                                         nn.BatchNorm1d(num_hidden * 4), nn.ReLU(), nn.MaxPool1d(kernel_size=2, stride=2, padding=1))


class MPNN_mk(nn.Module):
    def __init__(self, input_dimension, output_dimension, k):
        super().__init__()
        self.theta = nn.ModuleList([nn.Linear(input_dimension, output_dimension) for _ in range(k)])


class Clustering_Assignment_Matrix_cat_proj_prop(nn.Module):
    def __init__(self, in_num_node, input_dimension, hidden_dimension, out_num_node):
        super().__init__()
        self.dimension_mapping = nn.Linear(input_dimension, hidden_dimension)
        self.matrix = nn.Linear(in_num_node + hidden_dimension, out_num_node)


class Graph_Classification_block(nn.Module):
    def __init__(self, input_dimension, out_dimension, in_nodes, out_nodes):
        super().__init__()
        self.Message_Passing = MPNN_mk(input_dimension, out_dimension, 1)
        self.Graph_Clustering = Clustering_Assignment_Matrix_cat_proj_prop(in_nodes, input_dimension, out_nodes, out_nodes)


_BN_LAYERS = ("Time_Preprocessing.conv_block1.1", "Time_Preprocessing.conv_block2.1", "Time_Preprocessing.conv_block3.1")


class HierCorrPool_model(DropoutStepModule):
    dropout_by_sample_offset = False         # data parallelism is refused (algorithms.py): dp.py has no sample offset to pass

    def __init__(self, patch_size, num_patch, input_dim, hidden_dim, embedding_dim, num_nodes, encoder_conv_kernel, num_nodes_out):
        super().__init__()
        self.patch_size, self.num_patch, self.input_dim = int(patch_size), int(num_patch), input_dim
        self.hidden_dim, self.embedding_dim, self.num_nodes = int(hidden_dim), int(embedding_dim), int(num_nodes)
        self.encoder_conv_kernel, self.num_nodes_out = int(encoder_conv_kernel), int(num_nodes_out)
        N, h, e, K, M = self.num_nodes, self.hidden_dim, self.embedding_dim, self.encoder_conv_kernel, self.num_nodes_out
        self.encoder_out_length = encoder_lengths(self.num_patch)[-1]
        if self.encoder_out_length * 4 * h != K * e:
            raise ValueError(f"HierCorrPool_model: the encoder leaves {self.encoder_out_length} steps of 4 * hidden_dim = {4 * h} features per "
                             f"node, {self.encoder_out_length * 4 * h} in all, but encoder_conv_kernel * embedding_dim = {K * e}: the model's "
                             "reshape to [encoder_conv_kernel, num_nodes, -1] needs the two to be equal")
        self.feature_dim = K * e
        # same construction order as the reference => same RNG consumption => same initial weights; the sub-modules only hold tensors
        self.Time_Preprocessing = Feature_extractor_1DCNN(self.patch_size * N, h * N, 8, 1, 0.35)
        self.gc1 = Graph_Classification_block(e * K, e * K * 3, N, M)
        self.fc_0 = nn.Linear(K * M * e * 3, e * 3)
        self.fc_1 = nn.Linear(e * 3, 1)
        self.dropout_p = 0.35
        self._bn_channels = (h * N, 2 * h * N, 4 * h * N)
        self._bn = self._nbt = None
        self._track_batchnorm_counters()
        self._init_flat()

    # ---- flat storage ----------------------------------------------------------------------------------
    workspace_slots = 3

    def _reflatten_buffers(self, dev):
        bufs = dict(self.named_buffers())
        bn = torch.empty(2 * sum(self._bn_channels), dtype=torch.float32, device=dev)
        nbt = torch.zeros(3, dtype=torch.int64, device=dev)
        off = 0
        for k, (layer, c) in enumerate(zip(_BN_LAYERS, self._bn_channels)):
            for stat in ("running_mean", "running_var"):
                bn[off:off + c].copy_(bufs[f"{layer}.{stat}"].detach().float())
                self._set_buffer(f"{layer}.{stat}", bn[off:off + c])
                off += c
            nbt[k].copy_(bufs[f"{layer}.num_batches_tracked"])
            self._set_buffer(f"{layer}.num_batches_tracked", nbt[k])
        self._bn, self._nbt = bn, nbt

    # ---- C-ABI calls -----------------------------------------------------------------------------------
    c_family, Args = "hiercorrpool", _lib.HiercorrpoolArgs
    not_covered = ("HierCorrPool HIP kernels do not cover this configuration (2 <= num_nodes <= 32, 1 <= num_nodes_out <= 16, "
                   "2 <= num_patch <= 64, 1 <= patch_size <= 64, encoder_conv_kernel * embedding_dim <= 512, 4 * hidden_dim * num_nodes <= 1024)")

    def _shape(self, batch):
        return _lib.HiercorrpoolShape(batch, self.patch_size, self.num_patch, self.hidden_dim, self.embedding_dim, self.num_nodes,
                                      self.encoder_conv_kernel, self.num_nodes_out)

    def _check_input(self, x):
        self._require_device(x)
        if x.dim() != 3 or x.size(1) != self.num_nodes or x.size(2) != self.num_patch * self.patch_size:
            raise RuntimeError(f"expected input [bs, {self.num_nodes}, {self.num_patch * self.patch_size}], got {list(x.shape)}")
        return x.contiguous().float()

    def _args(self, shp, x, training, step, y=None, dpred=None, global_batch=None, sample_offset=0, update_running_stats=True):
        a = super()._args(shp, x, training, step, y, dpred, global_batch, sample_offset)
        a.bn_state = self._bn.data_ptr()
        a.update_running_stats = 1 if (training and update_running_stats and dpred is None) else 0      # (never in a backward)
        return a

    def tap(self, batch, which):
        """Workspace taps of the last forward at this batch size (parity tests): 'encoder' [B, L', C3], 'pooled_x' [B, M, d],
        'pooled_adj' [B, M, M], 'H' [B, M, 3 d]."""
        M, d = self.num_nodes_out, self.feature_dim
        idx, shape = {"encoder": (0, (self.encoder_out_length, 4 * self.hidden_dim * self.num_nodes)), "pooled_x": (1, (M, d)),
                      "pooled_adj": (2, (M, M)), "H": (3, (M, 3 * d))}[which]
        return self._tap(batch, idx, (batch, *shape))

    def fused_mse_step(self, x, y, optimizer=None, global_batch=None, update_running_stats=True, sample_offset=0):
        """train-mode forward + MSE + backward (+ Adam when ``optimizer`` is a FusedAdam over this model) in one C call; fills
        ``self.bucket`` = [grad | loss]; returns (pred [B], loss 0-d tensor) on the device, no host sync."""
        out = super().fused_mse_step(x, y, optimizer, global_batch, sample_offset, update_running_stats=update_running_stats)
        if update_running_stats:
            self._nbt_pending += 1
        return out

    # ---- nn.Module surface -----------------------------------------------------------------------------
    def forward(self, x):
        x = self._check_input(x)
        if x.size(0) == 0:
            raise RuntimeError("HierCorrPool_model: empty batch")
        if not self.training:
            return self._predict(x, False, self._step, autograd=False)[0]
        self._step += 1
        pred = self._predict(x, True, self._step, autograd=self._needs_grad())[0]
        self._nbt_pending += 1
        return pred
