"""Drop-in ``STFA_model``: multi-head graph attention over the 14 C-MAPSS sensors on a fixed prior-knowledge graph, patch by patch, then
one LSTM and a head on its last step.  The whole model runs behind three C entries on one flat parameter buffer
(``rulgnn_stfa_{forward,backward,fwdbwd}_f32``; ``fused_mse_step`` is train-mode forward + MSE + backward + Adam in one call): the graph
stage is ONE forward and ONE backward kernel of csrc/stfa.hip -- a wavefront per graph, every head's projection, scores, softmax and
neighbour sum in LDS and registers, the result written straight into the LSTM's input row -- the LSTM is the persistent one-direction
kernel of csrc/bilstm.hip.

Mirrors the reference class (models/STFA/Model.py:81-126): same constructor ``(patch_size, num_patch, num_nodes, hidden_dim, output_dim,
encoder_hidden_dim, device, num_heads, dropout)``, ``forward(x)`` with ``x [bs, 14, num_patch * patch_size]`` returning the prediction
``[bs, 1]``, the same 48 ``state_dict`` keys in the same order and -- sub-modules being created in the reference's order -- the same
initial weights for a torch seed.  Reference behaviour kept:

  * the adjacency (22 undirected edges, no self-loops) multiplies the attention BEHIND the softmax over all 14 nodes and behind the
    dropout, so rows do not sum to one;
  * the "ASE" softmax (Model.py:115) acts on a last dimension of one element and is exactly 1: the "global feature" is ``T`` ones in front
    of every LSTM input row, and ``v.weight`` / ``v.bias`` receive gradients that are exactly zero -- zeros, not ``None``, so Adam's
    weight decay still moves ``v``, here as there;
  * the head reads the LSTM's last step only;
  * ``hidden_dim`` is accepted and unused; ``device`` is accepted and ignored (the reference's algorithm writes ``'cuda:0'`` into its
    configs; the graph here is a table in the kernel source, not a tensor);
  * a non-finite sample makes its own prediction, and only that one, NaN.

The attention dropout (``dropout``) follows ``model.train()`` / ``model.eval()`` and draws from the package's counter hash by sample
index in the global batch, patch, head and edge; only the 44 directed edges are drawn.  There is no CPU path: a non-CUDA input raises.

Coverage (stated once: ``LIMITS``, mirrored by include/rulgnn.h RULGNN_STFA_*): the reference row runs; a model outside the limits
constructs and is refused at its first forward, before any launch or allocation.
"""
from __future__ import annotations

import torch.nn as nn

from . import _lib
from .flat import DropoutStepModule

# include/rulgnn.h RULGNN_STFA_*
LIMITS = {"num_nodes": 14, "max_num_patch": 128, "max_patch_size": 64, "max_output_dim": 16, "max_heads": 16, "max_lstm_hidden": 128}
TAP_ROWS, TAP_LSTM = 0, 1


def within_limits(num_nodes, num_patch, patch_size, output_dim, num_heads, encoder_hidden_dim):
    return (num_nodes == LIMITS["num_nodes"] and 1 <= num_patch <= LIMITS["max_num_patch"] and 1 <= patch_size <= LIMITS["max_patch_size"]
            and 1 <= output_dim <= LIMITS["max_output_dim"] and 1 <= num_heads <= LIMITS["max_heads"]
            and 1 <= encoder_hidden_dim <= LIMITS["max_lstm_hidden"])


class GraphAttentionLayer(nn.Module):
    """Holder of ``linear`` and ``attention`` with the reference's initialisation order (Model.py:11-21); never called."""

    def __init__(self, in_features, out_features, dropout, alpha=0.1):
        super().__init__()
        self.in_features, self.out_features, self.dropout, self.alpha = in_features, out_features, dropout, alpha
        self.linear = nn.Linear(in_features, out_features)
        self.attention = nn.Linear(2 * out_features, 1)


class GAT(nn.Module):
    """Holder of ``attention_0 .. attention_{nheads-1}`` (Model.py:47-53); never called."""

    def __init__(self, nfeat, nout, dropout, nheads):
        super().__init__()
        self.dropout = dropout
        for i in range(nheads):
            self.add_module('attention_{}'.format(i), GraphAttentionLayer(nfeat, nout, dropout=dropout))


class STFA_model(DropoutStepModule):
    def __init__(self, patch_size, num_patch, num_nodes, hidden_dim, output_dim, encoder_hidden_dim, device=None, num_heads=1, dropout=0.0):
        super().__init__()
        self.patch_size, self.num_patch, self.num_nodes = int(patch_size), int(num_patch), int(num_nodes)
        self.hidden_dim, self.output_dim, self.encoder_hidden_dim = int(hidden_dim), int(output_dim), int(encoder_hidden_dim)
        self.num_heads, self.dropout_p = int(num_heads), float(dropout)
        # same construction order as the reference => same RNG consumption => same initial weights; never called
        self.gat = GAT(self.patch_size, self.output_dim, nheads=self.num_heads, dropout=dropout)
        self.v = nn.Linear(self.output_dim * self.num_nodes, 1)
        self.lstm = nn.LSTM(self.output_dim * self.num_nodes + self.num_patch, self.encoder_hidden_dim, batch_first=True)
        self.fc = nn.Linear(self.encoder_hidden_dim, 1)
        self._init_flat()

    workspace_slots = 3
    empty_batch = "STFA_model: empty batch"

    # ---- C-ABI calls -----------------------------------------------------------------------------------
    c_family, Args = "stfa", _lib.StfaArgs
    not_covered = ("STFA HIP kernels do not cover this configuration (num_nodes == {num_nodes}, 1 <= num_patch <= {max_num_patch}, "
                   "1 <= patch_size <= {max_patch_size}, 1 <= output_dim <= {max_output_dim}, 1 <= num_heads <= {max_heads}, "
                   "1 <= encoder_hidden_dim <= {max_lstm_hidden})").format(**LIMITS)

    def _shape(self, batch):
        s = _lib.StfaShape()
        s.batch, s.num_patch, s.patch_size, s.num_nodes = batch, self.num_patch, self.patch_size, self.num_nodes
        s.output_dim, s.num_heads, s.encoder_hidden_dim = self.output_dim, self.num_heads, self.encoder_hidden_dim
        return s

    def _check_input(self, x):
        self._require_device(x)
        bs = x.size(0)
        if x.numel() != bs * self.num_nodes * self.num_patch * self.patch_size:
            raise RuntimeError(f"shape '[{bs}, {self.num_nodes}, {self.num_patch}, {self.patch_size}]' is invalid for input of size {x.numel()}")
        if not within_limits(self.num_nodes, self.num_patch, self.patch_size, self.output_dim, self.num_heads, self.encoder_hidden_dim):
            raise RuntimeError(self.not_covered)             # before the library is touched: nothing allocated, nothing launched
        return x.reshape(bs, self.num_nodes * self.num_patch * self.patch_size).contiguous().float()

    def tap(self, batch, which):
        """Workspace taps of the last forward at this batch size (parity tests): 'gat' (the stage output, relu of the heads' mean)
        [batch, T, 14 * output_dim], 'rows' (the LSTM's input: T ones, then 'gat') [batch, T, T + 14 * output_dim], 'lstm' (the LSTM's
        output) [batch, T, encoder_hidden_dim]."""
        T, rows = self.num_patch, (TAP_ROWS, (batch, self.num_patch, self.num_patch + self.num_nodes * self.output_dim))
        out = self._tap(batch, *{"gat": rows, "rows": rows, "lstm": (TAP_LSTM, (batch, T, self.encoder_hidden_dim))}[which])
        return out[:, :, T:].clone() if which == "gat" else out