"""Drop-in ``GRU_CM_model`` (reference models/GRU_CM/Model.py:43-82): per (sample, time step) an edge-MLP message-passing layer over all
ordered sensor pairs, a max over the sensors, a GRU over the time steps and a linear head.  The whole model runs behind three C entries
on one flat parameter buffer (``rulgnn_grucm_{forward,backward,fwdbwd}_f32``; ``fused_mse_step`` is forward + MSE + backward + Adam in
one call): the graph stage and the head in the gfx950 kernels of csrc/grucm.hip, the recurrence in the persistent kernel of
csrc/gru_seq.hip where it applies (gru_hidden_dim == 64) and in the step loop of csrc/gru.hip elsewhere.

Mirrors the reference class: same constructor ``(time_length, num_nodes, gru_hidden_dim=128)``, ``forward(x)`` returning ``[bs, 1]``,
the same 12 ``state_dict`` keys and -- sub-modules being created in the reference's order -- the same initial weights for a torch seed.
The three ``nn.Dropout`` use the counter-based hash of the other families (mask = f(seed, step, site, element); torch's Bernoulli
stream cannot be reproduced by any other implementation); their rates are read from ``dropout1/2/3.p`` at every call.  There is no CPU
path: a non-CUDA input raises.
"""
from __future__ import annotations

import torch.nn as nn

from . import _lib
from .flat import DropoutStepModule


# ---- parameter holders: created in the reference's order so that a seed gives the reference's initial weights; never called ----
class GNNLayer(nn.Module):
    def __init__(self, input_dim, output_dim):
        super().__init__()
        self.edge_mlp = nn.Sequential(nn.Linear(2 * input_dim, output_dim), nn.ReLU())
        self.node_mlp = nn.Sequential(nn.Linear(input_dim + output_dim, output_dim), nn.ReLU())


PARAM_ORDER = ["input_linear.weight", "input_linear.bias", "gnn.edge_mlp.0.weight", "gnn.edge_mlp.0.bias",
               "gnn.node_mlp.0.weight", "gnn.node_mlp.0.bias",
               "gru.weight_ih_l0", "gru.weight_hh_l0", "gru.bias_ih_l0", "gru.bias_hh_l0",
               "output_linear.weight", "output_linear.bias"]


def param_layout(num_nodes, time_length, gru_hidden_dim):
    """name -> (offset, shape) in the flat buffer the kernels read (include/rulgnn.h), in state_dict order, and the float count."""
    h, H, L = int(num_nodes) // 2, int(gru_hidden_dim), int(time_length)
    shapes = [(h, 1), (h,), (h, 2 * h), (h,), (h, 2 * h), (h,), (3 * H, h), (3 * H, H), (3 * H,), (3 * H,), (1, H * L), (1,)]
    layout, off = {}, 0
    for name, shape in zip(PARAM_ORDER, shapes):
        n = 1
        for d in shape:
            n *= d
        layout[name] = (off, shape)
        off += n
    return layout, off


class GRU_CM_model(DropoutStepModule):
    def __init__(self, time_length, num_nodes, gru_hidden_dim=128):
        super().__init__()
        self.time_length, self.num_nodes, self.gru_hidden_dim = int(time_length), int(num_nodes), int(gru_hidden_dim)
        hidden_dim = int(self.num_nodes / 2)
        self.hidden_dim = hidden_dim
        self.input_linear = nn.Linear(1, hidden_dim)
        self.dropout1 = nn.Dropout(0.2)
        self.gnn = GNNLayer(hidden_dim, hidden_dim)
        self.dropout2 = nn.Dropout(0.2)
        self.gru = nn.GRU(hidden_dim, self.gru_hidden_dim, batch_first=True)
        self.dropout3 = nn.Dropout(0.2)
        self.output_linear = nn.Linear(self.gru_hidden_dim * self.time_length, 1)
        self.gru_path = _lib.GRUCM_GRU_AUTO  # debugging / measurement: _lib.GRUCM_GRU_STEP_LOOP runs the recurrence on csrc/gru.hip
        if [n for n, _ in self.named_parameters()] != PARAM_ORDER:
            raise RuntimeError("parameter order differs from the flat layout of include/rulgnn.h")
        self._init_flat(*param_layout(self.num_nodes, self.time_length, self.gru_hidden_dim))

    flat_order = PARAM_ORDER
    workspace_slots = 4
    # like the reference: reshape(0, -1) is ambiguous (Model.py:77)
    empty_batch = ("cannot reshape tensor of 0 elements into shape [0, -1] because the unspecified dimension size -1 can be any value and is "
                   "ambiguous")

    # ---- C-ABI calls -----------------------------------------------------------------------------------
    c_family, Args = "grucm", _lib.GrucmArgs
    not_covered = ("GRU_CM HIP kernels do not cover this configuration (2 <= num_nodes <= 32, time_length <= 1024, gru_hidden_dim <= 1024, "
                   "gru_hidden_dim * time_length <= 65536)")

    def _shape(self, batch):
        return _lib.GrucmShape(batch, self.num_nodes, self.time_length, self.gru_hidden_dim)

    def _check_input(self, x):
        if x.dim() != 3 or x.size(1) != self.num_nodes or x.size(2) != self.time_length:
            raise RuntimeError(f"GRU_CM_model expects [bs, {self.num_nodes}, {self.time_length}], got {tuple(x.shape)}")
        self._require_device(x)
        return x.contiguous().float()

    @property
    def dropout_p(self):           # read at every call: a rate per dropout site, held by the three nn.Dropout
        mods = self._modules           # (nn.Module.__getattr__ costs half a microsecond a name)
        return mods["dropout1"].p, mods["dropout2"].p, mods["dropout3"].p

    def _args(self, shp, x, training, step, y=None, dpred=None, global_batch=None, sample_offset=0):
        a = super()._args(shp, x, training, step, y, dpred, global_batch, sample_offset)
        a.gru_path = int(self.gru_path)
        return a
