"""Drop-in ``AGCN_TF_model``.  The whole model runs behind three C entries on one flat parameter buffer
(``rulgnn_agcntf_{forward,backward,fwdbwd}_f32``; ``fused_mse_step`` is forward + MSE + backward + Adam in one call): SAGCN's 40
hand-crafted statistics of every patch as the front end (the same gfx950 kernels, csrc/sagcn.hip), then the two adjacency MLPs, the two
one-hop message-passing layers, the dense multi-head self-attention over the ``num_patch + 40`` nodes and the linear head in the
kernels of csrc/agcntf.hip.  Neither learned adjacency is ever formed and the attention probabilities are never stored (DESIGN.md
section 3n).

Mirrors the reference class (models/AGCN_TF/Model.py:137-189): same constructor ``(num_patch, patch_size, hidden_adj_dim,
hidden_gnn_dim, num_heads=1)``, ``forward(x) -> [bs, 1]``, the same ``state_dict`` keys in the same order (20 at one head, the
``nn.Sequential`` index names included) and -- sub-modules being created in the reference's order -- the same initial weights for a
torch seed.  The statistics depend on the input alone: forward-only.  No BatchNorm, no dropout: train and eval compute the same
function.  There is no CPU path: a non-CUDA input raises.

One behaviour is pinned where the reference leaves it open, the same one as SAGCN's: the statistic ``median_freq`` indexes the spectrum
through an UNSTABLE ``torch.argsort`` of a power spectrum that is mirrored exactly (every value but DC / Nyquist appears twice); here
equal powers keep their bin order (a stable sort), which is what the reference's CPU sort produces for patches of up to 16 points --
beyond that the reference's own CPU and GPU sorts disagree with each other on the sign of that one feature.
"""
from __future__ import annotations

import torch.nn as nn

from . import _lib
from .flat import FlatModule


class MPNN_mk(nn.Module):
    def __init__(self, input_dimension, output_dimension, k):
        super().__init__()
        self.theta = nn.ModuleList([nn.Linear(input_dimension, output_dimension) for _ in range(k)])


class SelfAttention(nn.Module):
    def __init__(self, d_model):
        super().__init__()
        self.W_q = nn.Linear(d_model, d_model)
        self.W_k = nn.Linear(d_model, d_model)
        self.W_v = nn.Linear(d_model, d_model)


class MultiHeadSelfAttention(nn.Module):
    def __init__(self, d_model, num_heads):
        super().__init__()
        self.heads = nn.ModuleList([SelfAttention(d_model) for _ in range(num_heads)])


class AGCN_TF_model(FlatModule):
    def __init__(self, num_patch, patch_size, hidden_adj_dim, hidden_gnn_dim, num_heads=1):
        super().__init__()
        self.num_patch, self.patch_size = int(num_patch), int(patch_size)
        self.hidden_adj_dim, self.hidden_gnn_dim, self.num_heads = int(hidden_adj_dim), int(hidden_gnn_dim), int(num_heads)
        input_dim = 40
        # same construction order as the reference => same RNG consumption => same initial weights; the sub-modules only hold parameters
        self.attention_spa_adj = nn.Sequential(nn.Linear(self.num_patch, self.hidden_adj_dim), nn.Tanh(),
                                               nn.Linear(self.hidden_adj_dim, input_dim))
        self.attention_tem_adj = nn.Sequential(nn.Linear(input_dim, self.hidden_adj_dim), nn.Tanh(),
                                               nn.Linear(self.hidden_adj_dim, self.num_patch))
        self.spatial_gnn = MPNN_mk(self.num_patch, self.hidden_gnn_dim, k=1)
        self.temporal_gnn = MPNN_mk(input_dim, self.hidden_gnn_dim, k=1)
        self.self_attention = MultiHeadSelfAttention(self.hidden_gnn_dim, self.num_heads)
        self.fc = nn.Linear(self.hidden_gnn_dim * self.num_heads * (self.num_patch + input_dim), 1)
        self._init_flat()

    # ---- C-ABI calls -----------------------------------------------------------------------------------
    c_family, Args = "agcntf", _lib.AgcntfArgs
    not_covered = ("AGCN_TF HIP kernels do not cover this configuration (1 <= num_patch <= 256, 2 <= patch_size <= 2048, "
                   "1 <= hidden_adj_dim, hidden_gnn_dim <= 128, 1 <= num_heads <= 4)")

    def _shape(self, batch):
        return _lib.AgcntfShape(batch, self.num_patch, self.patch_size, self.hidden_adj_dim, self.hidden_gnn_dim, self.num_heads)

    def _check_input(self, x):
        self._require_device(x)
        bs = x.size(0)
        if x.numel() != bs * self.num_patch * self.patch_size:
            raise RuntimeError(f"shape '[{bs}, {self.num_patch}, {self.patch_size}]' is invalid for input of size {x.numel()}")
        return x.reshape(bs, self.num_patch * self.patch_size).contiguous().float()

    def tap(self, batch, which):
        """Workspace taps of the last forward at this batch size (parity tests): 'features' [B, P, 40], 'H' [B, N, Hg] (the 40 spatial
        rows first, as the reference concatenates), 'attention_out' [B, N, heads * Hg]; N = num_patch + 40."""
        idx, shape = {"features": (0, (self.num_patch, 40)), "H": (1, (self.num_patch + 40, self.hidden_gnn_dim)),
                      "attention_out": (2, (self.num_patch + 40, self.num_heads * self.hidden_gnn_dim))}[which]
        return self._tap(batch, idx, (batch, *shape))

    # ---- nn.Module surface -----------------------------------------------------------------------------
    def forward(self, x):
        x2 = self._check_input(x)
        if x2.size(0) == 0:
            raise RuntimeError("AGCN_TF_model: empty batch")
        return self._predict(x2, autograd=self._needs_grad())[0]
