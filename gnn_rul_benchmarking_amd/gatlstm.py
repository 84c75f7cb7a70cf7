"""Drop-in ``GAT_LSTM_model``: graph attention over a sample's patches under a banded adjacency, then a stack of LSTMs.  The whole model
runs behind three C entries on one flat parameter buffer (``rulgnn_gatlstm_{forward,backward,fwdbwd}_f32``; ``fused_mse_step`` is
train-mode forward + MSE + backward + Adam in one call): the 11 patch statistics and one banded attention kernel per layer and direction
in csrc/gatlstm.hip -- a workgroup per graph, the softmax denominators from the two score vectors, nothing ``N x N`` ever stored --
every projection as a matrix-core GEMM, the LSTMs in the persistent kernels of csrc/bilstm.hip.

Mirrors the reference class (models/GAT_LSTM/Model.py:112-165): same constructor ``(num_patch, patch_size, hidden_dim, lstm_hidden_dim,
dropout=0.1, alpha=0.1)``, ``forward(x)`` returning the prediction ``[bs, 1]``, the same 22 ``state_dict`` keys in the same order and --
sub-modules being created in the reference's order -- the same initial weights for a torch seed.  Reference behaviour kept: the adjacency
(identity plus the two off-diagonals) is applied BEHIND the softmax over all nodes, so rows do not sum to one; a constant patch makes its
skewness and kurtosis NaN (an all-zero one also its four factors), and a NaN node makes the prediction of its own sample, and only that
one, NaN.  ``patch_size <= 3`` raises in the reference (its coefficients divide by zero); here such a model constructs and is refused.
The attention dropout (``dropout_p``) follows ``model.train()`` / ``model.eval()`` and draws from the package's counter hash by sample
index in the global batch; only the band is drawn.  ``alpha`` other than 0.1 (the reference's default, used by every row) is refused: the
kernels hold the slope as a constant.  There is no CPU path: a non-CUDA input raises.

Coverage (stated once: ``LIMITS``, mirrored by include/rulgnn.h RULGNN_GATLSTM_*): all six reference rows run; a model outside the
limits constructs and is refused at its first forward, before any launch.
"""
from __future__ import annotations

import torch.nn as nn

from . import _lib
from .flat import DropoutStepModule

# include/rulgnn.h RULGNN_GATLSTM_*
LIMITS = {"max_num_patch": 128, "min_patch_size": 4, "max_patch_size": 2048, "max_layers": 4, "max_width": 512, "max_lstm_layers": 3,
          "max_lstm_hidden": 128}
NUM_FEATURES = 11


def within_limits(num_patch, patch_size, hidden_dim, lstm_hidden_dim):
    return (1 <= num_patch <= LIMITS["max_num_patch"] and LIMITS["min_patch_size"] <= patch_size <= LIMITS["max_patch_size"]
            and 1 <= len(hidden_dim) <= LIMITS["max_layers"] and all(1 <= c <= LIMITS["max_width"] for c in hidden_dim)
            and 1 <= len(lstm_hidden_dim) <= LIMITS["max_lstm_layers"] and all(1 <= e <= LIMITS["max_lstm_hidden"] for e in lstm_hidden_dim))


class GraphAttentionLayer(nn.Module):
    """Holder of ``linear`` and ``attention`` with the reference's initialisation order (Model.py:76-86); never called."""

    def __init__(self, in_features, out_features, dropout, alpha=0.1):
        super().__init__()
        self.in_features, self.out_features, self.dropout, self.alpha = in_features, out_features, dropout, alpha
        self.linear = nn.Linear(in_features, out_features)
        self.attention = nn.Linear(2 * out_features, 1)


class GAT_LSTM_model(DropoutStepModule):
    def __init__(self, num_patch, patch_size, hidden_dim, lstm_hidden_dim, dropout=0.1, alpha=0.1):
        super().__init__()
        self.num_patch, self.patch_size = int(num_patch), int(patch_size)
        self.hidden_dim = [int(c) for c in hidden_dim]
        self.lstm_hidden_dim = [int(e) for e in lstm_hidden_dim]
        self.dropout_p, self.alpha = float(dropout), float(alpha)
        dims = [NUM_FEATURES] + self.hidden_dim
        ldims = [dims[-1]] + self.lstm_hidden_dim
        # same construction order as the reference => same RNG consumption => same initial weights; never called
        self.gat_layers = nn.ModuleList([GraphAttentionLayer(dims[i], dims[i + 1], dropout, alpha) for i in range(len(dims) - 1)])
        self.lstm_layers = nn.ModuleList([nn.LSTM(ldims[i], ldims[i + 1], num_layers=1, batch_first=True) for i in range(len(ldims) - 1)])
        self.fc = nn.Linear(ldims[-1] * self.num_patch, 1)
        self._init_flat()

    workspace_slots = 3
    empty_batch = "GAT_LSTM_model: empty batch"

    # ---- C-ABI calls -----------------------------------------------------------------------------------
    c_family, Args = "gatlstm", _lib.GatlstmArgs
    not_covered = ("GAT_LSTM HIP kernels do not cover this configuration (num_patch <= {max_num_patch}, {min_patch_size} <= patch_size <= "
                   "{max_patch_size}, 1 to {max_layers} GAT layers of width <= {max_width}, 1 to {max_lstm_layers} LSTM layers of hidden width "
                   "<= {max_lstm_hidden}, alpha = 0.1)").format(**LIMITS)

    def _shape(self, batch):
        s = _lib.GatlstmShape()
        s.batch, s.num_patch, s.patch_size = batch, self.num_patch, self.patch_size
        s.num_gat, s.num_lstm = len(self.hidden_dim), len(self.lstm_hidden_dim)
        for i, c in enumerate(self.hidden_dim[:4]):
            s.hidden_dim[i] = c
        for i, e in enumerate(self.lstm_hidden_dim[:3]):
            s.lstm_hidden_dim[i] = e
        return s

    def _check_input(self, x):
        self._require_device(x)
        bs = x.size(0)
        if x.numel() != bs * self.num_patch * self.patch_size:
            raise RuntimeError(f"shape '[{bs}, {self.num_patch}, {self.patch_size}]' is invalid for input of size {x.numel()}")
        if not (within_limits(self.num_patch, self.patch_size, self.hidden_dim, self.lstm_hidden_dim) and self.alpha == 0.1):
            raise RuntimeError(self.not_covered)             # before the library is touched: nothing allocated, nothing launched
        return x.reshape(bs, self.num_patch * self.patch_size).contiguous().float()

    def tap(self, batch, which):
        """Workspace taps of the last forward at this batch size (parity tests): 'feat' [batch, T, 11], 'h{l}' (the output of GAT layer l)
        [batch, T, hidden_dim[l]], 'lstm' (the last LSTM layer's output) [batch, T, lstm_hidden_dim[-1]]."""
        taps = {"feat": (0, NUM_FEATURES), "lstm": (1 + LIMITS["max_layers"], self.lstm_hidden_dim[-1]),       # RULGNN_GATLSTM_TAP_LSTM
                **{f"h{l}": (1 + l, c) for l, c in enumerate(self.hidden_dim)}}
        idx, width = taps[which]
        return self._tap(batch, idx, (batch, self.num_patch, width))