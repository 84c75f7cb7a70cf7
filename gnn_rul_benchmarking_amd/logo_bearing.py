"""Drop-in ``LOGO_bearing_model``: LOGO (logo.py) behind an STFT front end, for the bearing datasets.  Every patch of a window goes
through ``torch.stft``'s arithmetic (``n_fft = hop = win = nperseg``, periodic Hann, reflect-centred); the ``nperseg / 2 + 1`` frequency
bins are the graph's nodes and the ``1 + patch_size // nperseg`` frames of a patch their features.  From there on it is LOGO with
``patch_size = input_dim``, and it runs on LOGO's code: the fused graph kernels of csrc/logo.hip build the magnitude straight into the
sample's LDS window (``lgb_graph_fwd`` / ``lgb_graph_bwd`` are ``lg_graph_fwd<true>`` / ``lg_graph_bwd<true>``: the spectrogram never
reaches memory), the three Bi-LSTMs recurring along the batch, the head and the loss are LOGO's host chain unchanged (DESIGN.md
section 3t).  Entries ``rulgnn_logob_{forward,backward,fwdbwd}_f32`` on LOGO's argument struct.

Mirrors the reference class (models/LOGO_bearing/Model.py:263-347): same constructor ``(patch_size, num_patch, input_dim, num_nodes,
nperseg, hidden_dim)``, ``forward(X, GL=False, gamma=1)``, the same 46 ``state_dict`` keys in the same order and the same initial weights
for a torch seed.  Like the reference, a model whose ``num_nodes`` / ``input_dim`` do not describe the STFT's shape constructs and fails
at its first forward.  Everything logo.py says about the recurrence along the batch (``eval_sample_independent = False``), ``TD.drop1``,
NaN for a constant row of the spectrogram, the dropout stream and the missing CPU path holds here.

Coverage (stated once: ``LIMITS``, mirrored by include/rulgnn.h ``RULGNN_LOGOB_MAX_*``): both reference geometries -- PHM2012 (patch 64,
40 patches, nperseg 8: 5 nodes of 9 features) and XJTU_SY (1024, 32, 32: 17 nodes of 33) -- and nothing wider: the backward keeps the
gradients of ``MPNN.theta`` and ``nonlin_map`` in registers, 26 + 9 per thread at 33 features.
"""
from __future__ import annotations

import torch.nn as nn
from collections import OrderedDict

import torch

from . import _lib
from .logo import DROPOUT, Bi_LSTM_Standard, Graph_atten_block, LOGO_model, MPNN_mk

# include/rulgnn.h RULGNN_LOGOB_MAX_*
LIMITS = {"max_nodes": 17, "max_input_dim": 33, "max_sequences": 65535, "max_lstm_width": 128}


class LOGO_bearing_model(LOGO_model):
    """LOGO_model's surface (``forward``, ``fused_mse_step``, ``tap``, the autograd path) on the ``logob`` entries."""

    def __init__(self, patch_size, num_patch, input_dim, num_nodes, nperseg, hidden_dim):
        super(LOGO_model, self).__init__()
        self.patch_size, self.num_patch, self.input_dim = int(patch_size), int(num_patch), int(input_dim)
        self.num_nodes, self.nperseg, self.hidden_dim = int(num_nodes), int(nperseg), int(hidden_dim)
        f, T, N, h = self.input_dim, self.num_patch, self.num_nodes, self.hidden_dim
        # same construction order as the reference => same RNG consumption => same initial weights; the sub-modules only hold tensors
        self.nonlin_map = nn.Linear(f, 2 * f)
        self.MPNN = MPNN_mk(2 * f, 3 * f, k=1)
        self.TD = Bi_LSTM_Standard(3 * f, 3 * h)
        self.graph_attn_blk = Graph_atten_block(N, N)
        self.fc = nn.Sequential(OrderedDict([('fc1', nn.Linear(3 * h * T * N, 16)), ('relu1', nn.ReLU(inplace=True)),
                                             ('fc2', nn.Linear(16, 8)), ('relu2', nn.ReLU(inplace=True))]))
        self.cls = nn.Linear(8, 1)
        self.dropout_p = DROPOUT
        self._seed = int(torch.initial_seed()) & 0xFFFFFFFFFFFFFFFF
        self._step = 0
        self._init_flat()

    c_family = "logob"
    not_covered = ("LOGO_bearing HIP kernels do not cover this configuration (nperseg even and >= 2, patch_size > nperseg / 2, "
                   "num_nodes = nperseg / 2 + 1 <= {max_nodes}, input_dim = 1 + patch_size // nperseg <= {max_input_dim}, num_patch >= 1, "
                   "num_nodes * num_patch <= {max_sequences}, 6 * hidden_dim <= {max_lstm_width}: the persistent LSTM's widest layer; a "
                   "sample's whole spectrogram and the graph stage's matrices within one compute unit's 160 KB of LDS)").format(**LIMITS)

    @property
    def _feature_width(self):          # what LOGO_model.tap calls patch_size: the features per node and patch
        return self.input_dim

    def _shape(self, batch):
        return _lib.LogobShape(batch, self.patch_size, self.num_patch, self.input_dim, self.num_nodes, self.nperseg, self.hidden_dim)

    def _check_input(self, x):
        self._require_device(x)
        if x.dim() < 1 or x.size(0) < 1 or x.numel() // x.size(0) != self.num_patch * self.patch_size or x.numel() % x.size(0):
            raise RuntimeError(f"expected input with numel / batch == {self.num_patch * self.patch_size}, got {list(x.shape)}")
        ns, P = self.nperseg, self.patch_size
        if ns >= 2 and ns % 2 == 0 and P > ns // 2 and (self.num_nodes, self.input_dim) != (ns // 2 + 1, 1 + P // ns):
            # the reference's shape error at its first forward (nonlin_map / graph_attn_blk meet a tensor of another width)
            raise RuntimeError(f"LOGO_bearing_model: the STFT of a patch of {P} points at nperseg {ns} has {ns // 2 + 1} frequency bins of "
                               f"{1 + P // ns} frames, the model was constructed with num_nodes {self.num_nodes} and input_dim {self.input_dim}")
        return x.reshape(x.size(0), -1).contiguous().float()
