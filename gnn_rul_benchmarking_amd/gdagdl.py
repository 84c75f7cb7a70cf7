"""Drop-in ``GDAGDL_model``: the graph-attention model of the bearing datasets.  The whole model runs behind three C entries on one flat
parameter buffer (``rulgnn_gdagdl_{forward,backward,fwdbwd}_f32``; ``fused_mse_step`` is train-mode forward + MSE + reconstruction loss
+ backward + Adam in one call): the STFT front end with the Pearson mask and one fused graph-attention kernel per layer and direction in
csrc/gdagdl.hip -- a wavefront per graph, nothing ``N x N`` or pair-shaped ever leaves LDS -- every projection as a matrix-core GEMM, the
LSTM over the patches in the persistent kernels of csrc/bilstm.hip.

Mirrors the reference class (models/GDAGDL/Model.py:66-170): same constructor kwargs ``(num_patch, patch_size, num_nodes, nperseg,
input_dim, gat_layer_dim, lstm_hidden_dim, autoencoder_hidden_dim, autoencoder_out_dim)``, ``forward(x, train=False)`` returning the
prediction ``[bs, 1]`` or ``(prediction, reconstruction_loss)``, the same 36 ``state_dict`` keys in the same order and -- sub-modules
being created in the reference's order -- the same initial weights for a torch seed.  Reference behaviour kept: the adjacency is the
outer product of ``(pcc @ node_importance > 0)`` and is applied BEHIND the softmax (rows do not sum to one); it has no gradient, so
``node_importance_linear.{weight, bias}`` never receive one (``grad is None``; they sit first in the flat layout and Adam never touches
them); an all-zero patch makes its Pearson matrix NaN, ``NaN > 0`` is false, and the graph contributes exact zeros.  The attention
dropout (``dropout_p``, 0.5 hard-coded in the reference) follows ``model.train()`` / ``model.eval()`` and draws from the package's counter
hash by sample index in the global batch.  There is no CPU path: a non-CUDA input raises.

Coverage (stated once: ``LIMITS``, mirrored by include/rulgnn.h RULGNN_GDAGDL_MAX_*): all six reference rows run; a model outside the
limits constructs and is refused at its first forward, before any launch.
"""
from __future__ import annotations

import torch.nn as nn

from . import _lib
from .flat import DropoutStepModule

# include/rulgnn.h RULGNN_GDAGDL_MAX_*
LIMITS = {"max_nperseg": 64, "max_frames": 64, "max_layers": 4, "max_width": 512, "max_lstm_hidden": 128, "max_ae_width": 1024}


def within_limits(patch_size, nperseg, gat_layer_dim, lstm_hidden_dim, autoencoder_hidden_dim, autoencoder_out_dim):
    if not (2 <= nperseg <= LIMITS["max_nperseg"] and nperseg % 2 == 0 and patch_size % nperseg == 0 and patch_size > nperseg // 2):
        return False
    return (1 + patch_size // nperseg <= LIMITS["max_frames"] and 1 <= len(gat_layer_dim) <= LIMITS["max_layers"]
            and all(1 <= c <= LIMITS["max_width"] for c in gat_layer_dim) and 1 <= lstm_hidden_dim <= LIMITS["max_lstm_hidden"]
            and 4 <= autoencoder_hidden_dim <= LIMITS["max_ae_width"] and 1 <= autoencoder_out_dim <= LIMITS["max_ae_width"])


class GraphAttentionLayer(nn.Module):
    """Holder of ``linear`` and ``attention`` with the reference's initialisation order (Model.py:6-16); never called."""

    def __init__(self, in_features, out_features, dropout, alpha=0.1):
        super().__init__()
        self.in_features, self.out_features, self.dropout, self.alpha = in_features, out_features, dropout, alpha
        self.linear = nn.Linear(in_features, out_features)
        self.attention = nn.Linear(2 * out_features, 1)


class GDAGDL_model(DropoutStepModule):
    def __init__(self, num_patch, patch_size, num_nodes, nperseg, input_dim, gat_layer_dim, lstm_hidden_dim, autoencoder_hidden_dim,
                 autoencoder_out_dim):
        super().__init__()
        self.num_patch, self.patch_size, self.nperseg = int(num_patch), int(patch_size), int(nperseg)
        self.num_nodes, self.input_dim = int(num_nodes), int(input_dim)
        self.gat_layer_dim = [int(c) for c in gat_layer_dim]
        self.lstm_hidden_dim = int(lstm_hidden_dim)
        self.autoencoder_hidden_dim, self.autoencoder_out_dim = int(autoencoder_hidden_dim), int(autoencoder_out_dim)
        self.dropout_p = 0.5                 # Model.py:78, hard-coded there
        dims = [self.input_dim] + self.gat_layer_dim
        A, O, D = self.autoencoder_hidden_dim, self.autoencoder_out_dim, dims[-1] * self.num_nodes
        # same construction order as the reference => same RNG consumption => same initial weights; never called
        self.gat_layers = nn.ModuleList([GraphAttentionLayer(dims[i], dims[i + 1], dropout=0.5) for i in range(len(dims) - 1)])
        self.node_importance_linear = nn.Linear(self.input_dim, 1)
        self.encoder = nn.Sequential(nn.Linear(D, A), nn.ReLU(), nn.Linear(A, A // 2), nn.ReLU(), nn.Linear(A // 2, A // 4), nn.ReLU(),
                                     nn.Linear(A // 4, O))
        self.decoder = nn.Sequential(nn.Linear(O, A // 4), nn.ReLU(), nn.Linear(A // 4, A // 2), nn.ReLU(), nn.Linear(A // 2, A), nn.ReLU(),
                                     nn.Linear(A, D))
        self.lstm = nn.LSTM(input_size=O, hidden_size=self.lstm_hidden_dim, batch_first=True)
        self.linear = nn.Linear(self.lstm_hidden_dim * self.num_patch, 1)
        # flat layout: the two tensors without a gradient first (include/rulgnn.h), then the reference's order
        gradless = ["node_importance_linear.weight", "node_importance_linear.bias"]
        self.flat_order = gradless + [n for n, _ in self.named_parameters() if n not in gradless]
        self._init_flat()
        self.optimized_range = (self.input_dim + 1, self._count)

    bucket_tail = 2            # [gradient | loss | reconstruction]
    gradless_params = 2        # node_importance_linear.weight, .bias
    workspace_slots = 3
    # the reconstruction gradients are scaled in place by the backward: one backward per forward
    consumes_tape = True
    empty_batch = "GDAGDL_model: empty batch"

    @property
    def bucket(self):
        """[gradient | loss]: what one all-reduce carries in data-parallel training (the reconstruction term sits behind it)."""
        return self._grad_flat[:self._count + 1]

    # ---- C-ABI calls -----------------------------------------------------------------------------------
    c_family, Args = "gdagdl", _lib.GdagdlArgs
    not_covered = ("GDAGDL HIP kernels do not cover this configuration (num_nodes = nperseg / 2 + 1, input_dim = 1 + patch_size / nperseg, "
                   "even nperseg <= {max_nperseg} dividing patch_size, input_dim <= {max_frames}, 1 to {max_layers} GAT layers of width <= "
                   "{max_width}, lstm_hidden_dim <= {max_lstm_hidden}, 4 <= autoencoder_hidden_dim and autoencoder_out_dim <= {max_ae_width}: "
                   "a graph's backward state must fit one compute unit's 160 KB of LDS)").format(**LIMITS)

    def _shape(self, batch):
        s = _lib.GdagdlShape()
        s.batch, s.num_patch, s.patch_size, s.num_nodes, s.nperseg, s.input_dim = batch, self.num_patch, self.patch_size, self.num_nodes, self.nperseg, self.input_dim
        s.num_gat = len(self.gat_layer_dim)
        for i, c in enumerate(self.gat_layer_dim[:4]):
            s.gat_layer_dim[i] = c
        s.lstm_hidden_dim, s.autoencoder_hidden_dim, s.autoencoder_out_dim = self.lstm_hidden_dim, self.autoencoder_hidden_dim, self.autoencoder_out_dim
        return s

    def _check_input(self, x):
        self._require_device(x)
        bs = x.size(0)
        if x.numel() != bs * self.num_patch * self.patch_size:
            raise RuntimeError(f"shape '[{bs}, {self.num_patch}, {self.patch_size}]' is invalid for input of size {x.numel()}")
        if not (within_limits(self.patch_size, self.nperseg, self.gat_layer_dim, self.lstm_hidden_dim, self.autoencoder_hidden_dim,
                              self.autoencoder_out_dim)
                and self.num_nodes == self.nperseg // 2 + 1 and self.input_dim == 1 + self.patch_size // self.nperseg):
            raise RuntimeError(self.not_covered)             # before the library is touched: nothing allocated, nothing launched
        return x.reshape(bs, self.num_patch * self.patch_size).contiguous().float()

    def _args(self, shp, x, training, step, y=None, dpred=None, global_batch=None, sample_offset=0, recon_weight=None):
        a = super()._args(shp, x, training, step, y, dpred, global_batch, sample_offset)
        a.recon = self._grad_flat.data_ptr() + 4 * (self._count + 1)
        a.recon_weight = recon_weight.data_ptr() if recon_weight is not None else None
        return a

    def _run_forward(self, x, *state):
        """(prediction, reconstruction loss): the reconstruction term is a 0-d tensor (a term of the reference's loss)."""
        return super()._run_forward(x, *state) + (self._grad_flat[self._count + 1],)

    def _run_backward(self, x, douts, *state):
        # The reconstruction term enters with whatever weight the objective gave it (the reference: 1, algorithms.py:539; a loss on the
        # prediction alone: 0) -- handed to the kernels as a device scalar, no host round trip.
        w = douts[1].reshape(1).contiguous().float()
        return super()._run_backward(x, douts, *state, recon_weight=w)

    def tap(self, batch, which):
        """Workspace taps of the last forward at this batch size (parity tests): 'mag' [batch, T, N, f], 'ni' and 'mask' [batch, T, N],
        'yo' [batch, T, N * C_last], 'H' (the encoder output) [batch, T, autoencoder_out_dim]."""
        T, N = self.num_patch, self.num_nodes
        idx, shape = {"mag": (0, (batch, T, N, self.input_dim)), "ni": (1, (batch, T, N)), "mask": (2, (batch, T, N)),
                      "yo": (3, (batch, T, N * self.gat_layer_dim[-1])), "H": (4, (batch, T, self.autoencoder_out_dim))}[which]
        return self._tap(batch, idx, shape)

    # ---- nn.Module surface -----------------------------------------------------------------------------
    def forward(self, x, train=False):
        """``train`` only selects the return value, as in the reference."""
        pred, recon = self._forward_outputs(x)
        return (pred, recon) if train else pred
