"""Drop-in ``SAGCN_model``.  The whole model runs behind three C entries on one flat parameter buffer
(``rulgnn_sagcn_{forward,backward,fwdbwd}_f32``; ``fused_mse_step`` is forward + MSE + backward + Adam in one call): the 40
hand-crafted statistics of every patch, the cosine adjacency and its normalised aggregation in the gfx950 kernels of csrc/sagcn.hip,
every Linear layer -- over the node axis or the feature axis -- as a matrix-core GEMM on node-major activations.

Mirrors the reference class (models/SAGCN/Model.py:127-156): same constructor kwargs ``(num_patch, patch_size, gcn_hidden_dim,
attention_hidden_dim)``, ``forward(x) -> [bs, 1]``, the same 16 ``state_dict`` keys in the same order and -- sub-modules being created
in the reference's order -- the same initial weights for a torch seed.  The statistics depend on the input alone: forward-only.
There is no CPU path: a non-CUDA input raises.

One behaviour is pinned where the reference leaves it open: the statistic ``median_freq`` indexes the spectrum through an UNSTABLE
``torch.argsort`` of a power spectrum that is mirrored exactly (every value but DC / Nyquist appears twice); here equal powers keep
their bin order (a stable sort), which is what the reference's CPU sort produces for patches of up to 16 points (its PHM2012
Condition_1 row) -- beyond that the reference's own CPU and GPU sorts disagree with each other on the sign of that one feature.
"""
from __future__ import annotations

import torch.nn as nn

from . import _lib
from .flat import FlatModule


class GCNLayer(nn.Module):
    def __init__(self, in_features, out_features):
        super().__init__()
        self.linear = nn.Linear(in_features, out_features)


class GraphProjectionLayer(nn.Module):
    def __init__(self, in_features, out_features, num_nodes):
        super().__init__()
        self.linear = nn.Linear(in_features, out_features)
        self.project_matrices = nn.Linear(num_nodes, num_nodes)


class SelfAttentionLayer(nn.Module):
    def __init__(self, num_nodes, attention_hidden_dim):
        super().__init__()
        self.tanh_layer = nn.Linear(num_nodes, attention_hidden_dim)
        self.softmax_layer = nn.Linear(attention_hidden_dim, num_nodes)


class SAGCN_model(FlatModule):
    def __init__(self, num_patch, patch_size, gcn_hidden_dim, attention_hidden_dim):
        super().__init__()
        self.num_patch, self.patch_size = int(num_patch), int(patch_size)
        self.gcn_hidden_dim, self.attention_hidden_dim = int(gcn_hidden_dim), int(attention_hidden_dim)
        # same construction order as the reference => same RNG consumption => same initial weights; the sub-modules only hold parameters
        self.gcn1 = GCNLayer(40, self.gcn_hidden_dim)
        self.proj1 = GraphProjectionLayer(self.gcn_hidden_dim, self.gcn_hidden_dim, self.num_patch)
        self.proj2 = GraphProjectionLayer(self.gcn_hidden_dim, self.gcn_hidden_dim, self.num_patch)
        self.attn = SelfAttentionLayer(self.num_patch, self.attention_hidden_dim)
        self.fc = nn.Linear(self.gcn_hidden_dim * self.num_patch, 1)
        self._init_flat()

    # ---- C-ABI calls -----------------------------------------------------------------------------------
    c_family, Args = "sagcn", _lib.SagcnArgs
    not_covered = ("SAGCN HIP kernels do not cover this configuration (num_patch <= 256, 2 <= patch_size <= 2048, hidden sizes <= 4096, "
                   "batch * gcn_hidden_dim * num_patch < 2^31)")

    def _shape(self, batch):
        return _lib.SagcnShape(batch, self.num_patch, self.patch_size, self.gcn_hidden_dim, self.attention_hidden_dim)

    def _check_input(self, x):
        self._require_device(x)
        bs = x.size(0)
        if x.numel() != bs * self.num_patch * self.patch_size:
            raise RuntimeError(f"shape '[{bs}, {self.num_patch}, {self.patch_size}]' is invalid for input of size {x.numel()}")
        return x.reshape(bs, self.num_patch * self.patch_size).contiguous().float()

    def tap(self, batch, which):
        """Workspace taps of the last forward at this batch size (parity tests): 'features' [B, P, 40], 'aggregated' (A_hat X), 'h3',
        'attention' -- the last three returned sample-major [B, P, .] (they are stored node-major)."""
        P = self.num_patch
        if which == "features":
            return self._tap(batch, 0, (batch, P, 40))
        idx, width = {"aggregated": (1, 40), "h3": (2, self.gcn_hidden_dim), "attention": (3, self.gcn_hidden_dim)}[which]
        return self._tap(batch, idx, (P, batch, width)).permute(1, 0, 2).contiguous()

    # ---- nn.Module surface -----------------------------------------------------------------------------
    def forward(self, x):
        x2 = self._check_input(x)
        if x2.size(0) == 0:
            raise RuntimeError("SAGCN_model: empty batch")
        return self._predict(x2, autograd=self._needs_grad())[0]
