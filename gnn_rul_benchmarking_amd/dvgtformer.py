"""Drop-in ``DVGTformer_model``: the dual-view graph transformer of the aero-engine datasets.  The whole model runs behind three C
entries on one flat parameter buffer (``rulgnn_dvgtformer_{forward,backward,fwdbwd}_f32``; ``fused_mse_step`` is train-mode forward +
MSE + backward + Adam in one call): the input stage, both Pearson graphs and all ``num_blocks`` x 2 half-blocks in the fused gfx950
encoder kernels of csrc/dvgtformer.hip -- one workgroup per sample, the sample's state in LDS, the wide ``d_model`` folded into
parameter-only operands once per call -- and the head on the shared SGEMM.

Mirrors the reference class (models/DVGTformer/Model.py:113-174): same constructor ``(num_nodes, time_length, d_model, num_heads,
lambda_param, d_ff, dropout, num_blocks)``, ``forward(X)`` returning ``[bs, 1]``, the same ``state_dict`` keys in the same order (214
at 3 blocks and 4 heads) and -- sub-modules being created in the reference's order -- the same initial weights for a torch seed.
Reference behaviour kept: both graphs are taken BEFORE the positional encoding is added and are differentiable; the positional encoding
is a constant (neither a buffer nor in ``state_dict``) with the reference's doubled even index; the residuals sit outside the
LayerNorms; only the temporal halves draw dropout (``dropout2`` of the spatial halves is never applied); a constant row or column of the
input-stage output makes a Pearson graph, and with it the prediction, NaN.  ``model.train()`` draws the dropout masks from the package's
counter hash (one mask per temporal block, by sample index in the global batch); ``model.eval()`` draws none.  The gradient of every
``linears_K_*.bias`` is zero in exact arithmetic (the softmax ignores a per-row constant) and comes back as an exact zero.  There is no
CPU path: a non-CUDA input raises.

Coverage (stated once: ``LIMITS``, mirrored by include/rulgnn.h RULGNN_DVGT_MAX_*): all five reference rows run; a model outside the
limits constructs and is refused at its first forward, before any launch.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from . import _lib
from .flat import DropoutStepModule

# include/rulgnn.h RULGNN_DVGT_MAX_*
LIMITS = {"max_nodes": 24, "max_time": 56, "max_heads": 8, "max_blocks": 8, "max_d_model": 1024, "max_d_ff": 128}


def within_limits(num_nodes, time_length, d_model, num_heads, d_ff, num_blocks):
    return (2 <= num_nodes <= LIMITS["max_nodes"] and 1 <= time_length <= LIMITS["max_time"] and 1 <= num_heads <= LIMITS["max_heads"]
            and 1 <= num_blocks <= LIMITS["max_blocks"] and all(1 <= d <= LIMITS["max_d_model"] for d in d_model)
            and all(1 <= f <= LIMITS["max_d_ff"] for f in d_ff))


# ---- parameter holders: created in the reference's order so that a seed gives the reference's initial weights; never called ----
class _HalfBlock(nn.Module):
    def __init__(self, features, d_model, num_heads, d_ff, dropout, view):
        super().__init__()
        heads = lambda: nn.ModuleList([nn.Linear(features, d_model) for _ in range(num_heads)])
        setattr(self, f"linears_Q_{view}", heads())
        setattr(self, f"linears_K_{view}", heads())
        setattr(self, f"linears_V_{view}", heads())
        setattr(self, f"W_O_{view}", nn.Linear(d_model * num_heads, features))
        setattr(self, f"layer_norm1_{view}", nn.LayerNorm(features))
        setattr(self, f"layer_norm2_{view}", nn.LayerNorm(features))
        setattr(self, f"feed_forward_{view}", nn.Sequential(nn.Linear(features, d_ff), nn.GELU(), nn.Linear(d_ff, features)))
        setattr(self, "dropout1" if view == "temp" else "dropout2", nn.Dropout(dropout))


class DVGTformer_model(DropoutStepModule):
    def __init__(self, num_nodes, time_length, d_model, num_heads, lambda_param, d_ff, dropout, num_blocks):
        super().__init__()
        self.num_nodes, self.time_length, self.num_heads, self.num_blocks = int(num_nodes), int(time_length), int(num_heads), int(num_blocks)
        self.d_model, self.d_ff = [int(v) for v in d_model], [int(v) for v in d_ff]
        self.lambda_param, self.dropout_p = float(lambda_param), float(dropout)
        N, L = self.num_nodes, self.time_length
        # same construction order as the reference => same RNG consumption => same initial weights (t_v and x_v draw after linear_x)
        self.linear_t = nn.Linear(L, L)
        self.linear_x = nn.Linear(N, N)
        self.t_v = nn.Parameter(torch.randn(1, 1, N))
        self.x_v = nn.Parameter(torch.randn(1, L + 1, 1))
        self.tvgtformer_blocks = nn.ModuleList([_HalfBlock(N + 1, self.d_model[0], self.num_heads, self.d_ff[0], dropout, "temp")
                                                for _ in range(self.num_blocks)])
        self.svgtformer_blocks = nn.ModuleList([_HalfBlock(L + 1, self.d_model[1], self.num_heads, self.d_ff[1], dropout, "spat")
                                                for _ in range(self.num_blocks)])
        self.output_layer = nn.Sequential(nn.Linear((L + 1) * (N + 1), 100), nn.GELU(), nn.Linear(100, 1))
        self._init_flat()

    workspace_slots = 3          # (an empty batch gives an empty prediction: ``empty_batch`` stays None)

    # ---- C-ABI calls -----------------------------------------------------------------------------------
    c_family, Args = "dvgtformer", _lib.DvgtformerArgs
    not_covered = ("DVGTformer HIP kernels do not cover this configuration (2 <= num_nodes <= {max_nodes}, 1 <= time_length <= {max_time}, "
                   "num_heads <= {max_heads}, num_blocks <= {max_blocks}, d_model <= {max_d_model}, d_ff <= {max_d_ff}: a sample's "
                   "backward state must fit one compute unit's 160 KB of LDS; 0 <= lambda_param <= 1)").format(**LIMITS)

    def _shape(self, batch):
        return _lib.DvgtformerShape(batch, self.num_nodes, self.time_length, self.num_heads, self.num_blocks,
                                    (C.c_int32 * 2)(*self.d_model), (C.c_int32 * 2)(*self.d_ff), self.lambda_param)

    def _check_input(self, x):
        if x.dim() != 3 or x.size(1) != self.num_nodes or x.size(2) != self.time_length:
            raise RuntimeError(f"DVGTformer_model expects [bs, {self.num_nodes}, {self.time_length}], got {tuple(x.shape)}")
        self._require_device(x)
        if not (within_limits(self.num_nodes, self.time_length, self.d_model, self.num_heads, self.d_ff, self.num_blocks)
                and 0.0 <= self.lambda_param <= 1.0):
            raise RuntimeError(self.not_covered)             # before the library is touched: nothing allocated, nothing launched
        return x.contiguous().float()

    def tap(self, batch, which):
        """Workspace taps of the last forward at this batch size (parity tests), both [batch, L+1, N+1]: 'x0' (X behind the input stage
        and the positional encoding), 'enc' (the encoder output, the head's input)."""
        return self._tap(batch, {"x0": 0, "enc": 1}[which], (batch, self.time_length + 1, self.num_nodes + 1))