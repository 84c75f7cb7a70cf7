"""Drop-in ``STMSGCN_model`` whose forward/backward run in the gfx950 HIP kernels (csrc/stmsgcn.hip).

Mirrors the reference class (models/STMSGCN/Model.py:63-112): same constructor kwargs
``(num_patch, patch_size, interval, band_width, gcn_dims, gru_hidden_dim)``, same ``forward(x) -> [bs, 1]``,
the same 14 ``state_dict`` keys (``gcn_layers.{i}.linear.*``, ``gru_layer.gru.*_l0``, ``fc.*``) and -- because the
parameter-holding sub-modules are created in the reference's order -- the same initial weights for a torch seed.
None of the sub-modules is ever *called* (the GRU included): every parameter is a view into one flat fp32 buffer
that the kernels read directly (layout in include/rulgnn.h).

There is no CPU path: calling the model with a non-CUDA tensor raises.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from . import _lib
from .flat import FlatModule, current_stream as _stream


class GCNLayer(nn.Module):
    """Holder of ``linear`` (Model.py:34-37)."""

    def __init__(self, in_features, out_features):
        super().__init__()
        self.linear = nn.Linear(in_features, out_features)


class GRULayer(nn.Module):
    """Holder of ``gru`` = nn.GRU(input_dim, hidden_dim, 1, batch_first=True) (Model.py:52-55); only its four
    tensors are used."""

    def __init__(self, input_dim, hidden_dim, num_layers):
        super().__init__()
        self.gru = nn.GRU(input_dim, hidden_dim, num_layers, batch_first=True)


def param_layout(num_patch, gcn_dims, gru_hidden_dim):
    """state_dict name (without the algorithm's ``model.`` prefix) -> (offset, shape) in the flat buffer."""
    dims = [1] + list(gcn_dims)
    H, Cc = gru_hidden_dim, sum(dims)
    out, off = {}, 0

    def put(name, shape):
        nonlocal off
        n = 1
        for s in shape:
            n *= s
        out[name] = (off, tuple(shape))
        off += n

    for l in range(len(gcn_dims)):
        put(f"gcn_layers.{l}.linear.weight", (dims[l + 1], dims[l]))
        put(f"gcn_layers.{l}.linear.bias", (dims[l + 1],))
    put("gru_layer.gru.weight_ih_l0", (3 * H, Cc))
    put("gru_layer.gru.weight_hh_l0", (3 * H, H))
    put("gru_layer.gru.bias_ih_l0", (3 * H,))
    put("gru_layer.gru.bias_hh_l0", (3 * H,))
    put("fc.weight", (1, H * num_patch))
    put("fc.bias", (1,))
    return out, off


class STMSGCN_model(FlatModule):
    def __init__(self, num_patch, patch_size, interval, band_width, gcn_dims, gru_hidden_dim):
        super().__init__()
        self.num_patch, self.patch_size = int(num_patch), int(patch_size)
        self.interval, self.band_width = int(interval), int(band_width)
        if self.interval < 1 or self.interval >= self.patch_size or (self.patch_size - self.interval) % self.band_width:
            raise RuntimeError(f"shape '[{-1}, {self.band_width}]' is invalid for input of size {self.patch_size - self.interval}")
        dims = [1] + [int(d) for d in gcn_dims]
        self.gcn_dims = dims
        self.gru_hidden_dim = int(gru_hidden_dim)
        # same construction order as the reference => same RNG consumption => same initial weights
        self.gcn_layers = nn.ModuleList([GCNLayer(dims[i], dims[i + 1]) for i in range(len(dims) - 1)])
        self.gru_layer = GRULayer(sum(dims), self.gru_hidden_dim, 1)
        self.fc = nn.Linear(self.gru_hidden_dim * self.num_patch, 1)
        self._init_flat(*param_layout(self.num_patch, dims[1:], self.gru_hidden_dim))

    workspace_slots = 4

    # ---- C-ABI calls -----------------------------------------------------------------------------------
    c_family, Args = "stmsgcn", _lib.StmsgcnArgs
    not_covered = ("STMSGCN kernels do not cover this configuration (nodes <= 32, patch_size <= 512, GCN widths <= 64 with sum <= 128, "
                   "gru_hidden_dim <= 16, num_patch <= 4096)")

    def _shape(self, batch):
        s = _lib.StmsgcnShape()
        s.batch, s.num_patch, s.patch_size = batch, self.num_patch, self.patch_size
        s.interval, s.band_width = self.interval, self.band_width
        s.num_gcn_layers = len(self.gcn_dims) - 1
        if s.num_gcn_layers > _lib.STMSGCN_MAX_LAYERS:
            raise RuntimeError(f"STMSGCN kernels cover at most {_lib.STMSGCN_MAX_LAYERS} GCN layers")
        for i, d in enumerate(self.gcn_dims[1:]):
            s.gcn_dims[i] = d
        s.gru_hidden = self.gru_hidden_dim
        return s

    def _check_input(self, x):
        self._require_device(x)
        bs = x.size(0)
        if x.numel() != bs * self.num_patch * self.patch_size:
            raise RuntimeError(f"shape '[{bs}, {self.num_patch}, {self.patch_size}]' is invalid for input of size {x.numel()}")
        return x.reshape(bs, self.num_patch * self.patch_size).contiguous().float()

    def features(self, x):
        """[bs*num_patch, nodes, sum(dims)]: the concatenated GCN features the reference hands to its GRU
        (Model.py:92-103, before the transpose)."""
        x2d = self._check_input(x)
        n = (self.patch_size - self.interval) // self.band_width
        out = torch.empty(x2d.size(0) * self.num_patch, n, sum(self.gcn_dims), dtype=torch.float32, device=x2d.device)
        shp = self._shape(x2d.size(0))
        _lib.check(_lib.load().rulgnn_stmsgcn_features_f32(C.byref(shp), x2d.data_ptr(), self._flat.data_ptr(), out.data_ptr(),
                                                           _stream()), "rulgnn_stmsgcn_features_f32")
        return out

    # ---- nn.Module surface -----------------------------------------------------------------------------
    def forward(self, x):
        x2d = self._check_input(x)
        if x2d.size(0) == 0:
            return torch.empty(0, 1, dtype=torch.float32, device=x2d.device)
        return self._predict(x2d, autograd=self._needs_grad())[0]
