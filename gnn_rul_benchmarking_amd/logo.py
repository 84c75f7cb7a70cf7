"""Drop-in ``LOGO_model``.  The whole model runs behind three C entries on one flat parameter buffer
(``rulgnn_logo_{forward,backward,fwdbwd}_f32``; ``fused_mse_step`` is train-mode forward + MSE + theta * L_GL + backward + Adam in one
call): the graph half -- per-(sample, patch) local graph, per-sample Pearson graph, gated fusion, message passing and the partial sums
of the graph-learning loss -- in the fused gfx950 kernels of csrc/logo.hip, which keep every N x N and N x 2p intermediate in LDS, the
three bidirectional LSTM layers in the persistent recurrences of csrc/bilstm.hip, the head on the shared SGEMM.

Mirrors the reference class (models/LOGO/Model.py:198-262): same constructor ``(patch_size, num_patch, num_nodes, hidden_dim)``,
``forward(X, GL=False, gamma=1)`` returning the prediction ``[bs, 1]`` or ``(prediction, L_GL)`` with both differentiable, the same
46 ``state_dict`` keys in the same order and -- sub-modules being created in the reference's order -- the same initial weights for a
torch seed.  Reference behaviour kept: the LSTMs recur ALONG THE BATCH (one sequence per (patch, sensor), one step per sample,
Model.py:245-251), in train and in eval, so every prediction depends on which samples share a batch and in which order
(``eval_sample_independent = False``: a test set is walked in the reference's batches, never re-batched); ``TD.drop1`` is never
applied; a constant sensor makes the Pearson graph, and with it every prediction of the batch, NaN.  ``model.train()`` draws the two
dropouts (``dropout_p``, 0.2) from the package's counter hash; ``model.eval()`` applies none.  There is no CPU path: a non-CUDA input
raises.

Coverage (stated once: ``LIMITS``, mirrored by include/rulgnn.h): the reference's FD001, FD002, FD004 and N-CMAPSS rows run; FD003
(``hidden_dim`` 32: the middle LSTM is 192 wide, beyond the persistent LSTM's 128) constructs and is refused at its first forward.
"""
from __future__ import annotations

from collections import OrderedDict

import torch
import torch.nn as nn

from . import _lib
from .flat import FlatModule

DROPOUT = 0.2              # models/LOGO/Model.py:96,104
# include/rulgnn.h RULGNN_LOGO_MAX_*
LIMITS = {"max_nodes": 32, "max_patch_size": 16, "max_sequences": 65535, "max_lstm_width": 128}


# ---- parameter holders: created in the reference's order so that a seed gives the reference's initial weights; never called ----
class MPNN_mk(nn.Module):
    def __init__(self, input_dimension, output_dimension, k):
        super().__init__()
        self.theta = nn.ModuleList([nn.Linear(input_dimension, output_dimension) for _ in range(k)])


class Bi_LSTM_Standard(nn.Module):
    def __init__(self, input_dim, num_hidden):
        super().__init__()
        self.bi_lstm1 = nn.LSTM(input_size=input_dim, hidden_size=num_hidden, num_layers=1, batch_first=True, dropout=0, bidirectional=True)
        self.drop1 = nn.Dropout(p=DROPOUT)
        self.bi_lstm2 = nn.LSTM(input_size=num_hidden, hidden_size=num_hidden * 2, num_layers=1, batch_first=True, dropout=0,
                                bidirectional=True)
        self.drop2 = nn.Dropout(p=DROPOUT)
        self.bi_lstm3 = nn.LSTM(input_size=num_hidden * 2, hidden_size=num_hidden, num_layers=1, batch_first=True, bidirectional=True)
        self.drop3 = nn.Dropout(p=DROPOUT)


class Graph_atten_block(nn.Module):
    def __init__(self, num_node, out_dimension):
        super().__init__()
        self.W_Z_T = nn.Linear(num_node, out_dimension)
        self.W_Z_G = nn.Linear(num_node, out_dimension)
        self.W_R_T = nn.Linear(num_node, num_node)
        self.W_R_G = nn.Linear(num_node, num_node)
        self.W_h_T = nn.Linear(num_node, num_node)
        self.W_h = nn.Linear(num_node, num_node)


class LOGO_model(FlatModule):
    # the recurrence runs along the batch: the eval forward depends on WHICH samples share a batch, so a test set must be walked in the
    # reference's batches on every rank, never re-batched per shard (trainer.py / dataloader.data_generator)
    eval_sample_independent = False

    def __init__(self, patch_size, num_patch, num_nodes, hidden_dim):
        super().__init__()
        self.patch_size, self.num_patch, self.num_nodes, self.hidden_dim = int(patch_size), int(num_patch), int(num_nodes), int(hidden_dim)
        p, T, N, h = self.patch_size, self.num_patch, self.num_nodes, self.hidden_dim
        # same construction order as the reference => same RNG consumption => same initial weights; the sub-modules only hold tensors
        self.nonlin_map = nn.Linear(p, 2 * p)
        self.MPNN = MPNN_mk(2 * p, 3 * p, k=1)
        self.TD = Bi_LSTM_Standard(3 * p, 3 * h)
        self.graph_attn_blk = Graph_atten_block(N, N)
        self.fc = nn.Sequential(OrderedDict([('fc1', nn.Linear(3 * h * T * N, 16)), ('relu1', nn.ReLU(inplace=True)),
                                             ('fc2', nn.Linear(16, 8)), ('relu2', nn.ReLU(inplace=True))]))
        self.cls = nn.Linear(8, 1)
        self.dropout_p = DROPOUT
        self._seed = int(torch.initial_seed()) & 0xFFFFFFFFFFFFFFFF
        self._step = 0
        self._init_flat()

    workspace_slots = 3
    output_buffers = 2         # prediction, L_GL (its first element)

    # ---- C-ABI calls -----------------------------------------------------------------------------------
    c_family, Args = "logo", _lib.LogoArgs
    not_covered = ("LOGO HIP kernels do not cover this configuration (2 <= num_nodes <= {max_nodes}, 1 <= patch_size <= {max_patch_size}, "
                   "num_patch >= 1, num_nodes * num_patch <= {max_sequences}, 6 * hidden_dim <= {max_lstm_width}: the persistent LSTM's "
                   "widest layer; a sample's whole window and the graph stage's matrices within one compute unit's 160 KB of LDS, "
                   "roughly num_nodes * num_patch * patch_size <= 38 000)").format(**LIMITS)

    @property
    def _feature_width(self):          # features per node and patch (LOGO_bearing: the STFT's frames)
        return self.patch_size

    def _shape(self, batch):
        return _lib.LogoShape(batch, self.patch_size, self.num_patch, self.num_nodes, self.hidden_dim)

    def _check_input(self, x):
        self._require_device(x)
        if x.dim() != 3 or x.size(1) != self.num_nodes or x.size(2) != self.num_patch * self.patch_size:
            raise RuntimeError(f"expected input [bs, {self.num_nodes}, {self.num_patch * self.patch_size}], got {list(x.shape)}")
        return x.contiguous().float()

    def _args(self, shp, x, training, step, theta=0.0, gamma=1.0, y=None, dpred=None, global_batch=None):
        """``training`` and ``step`` of a backward must be the forward's: it redraws the forward's dropout masks from them."""
        a = super()._args(shp, x, y, dpred, global_batch)
        a.loss_gl = self._out_bufs[1].data_ptr()
        a.theta, a.gamma = float(theta), float(gamma)
        a.dropout_p = float(self.dropout_p)
        a.seed, a.step = self._seed, int(step)
        a.training = 1 if training else 0
        return a

    def _workspace_entry(self, key, nbytes, unsupported, make=None):
        # (L_GL needs one float even where the prediction buffer of an odd batch size would do: two floats each, sliced)
        return super()._workspace_entry(key, nbytes, unsupported, make=lambda dev: (
            torch.empty(max(int(key), 1), dtype=torch.float32, device=dev)[:int(key)], torch.zeros(1, dtype=torch.float32, device=dev)))

    def _run_forward(self, x, *state):
        """One ``forward`` call; returns (prediction [B, 1], L_GL 0-d) as views of the output buffers, valid until the next call."""
        super()._run_forward(x, *state)
        return self._out_bufs[0].view(-1, 1), self._out_bufs[1].view(())

    def _run_backward(self, x, douts, training, step, theta, gamma):
        # the incoming gradient of L_GL takes theta's place (one host read; the fused step never comes here)
        coef = float(douts[1]) if len(douts) > 1 and douts[1] is not None else 0.0
        dpred = douts[0] if douts[0] is not None else torch.zeros(x.size(0), dtype=torch.float32, device=x.device)
        return super()._run_backward(x, (dpred,), training, step, coef, gamma)

    def tap(self, batch, which):
        """Workspace taps of the last forward at this batch size (parity tests): 'mpnn' [T N, B, 3p] (the graph stage's output, the
        LSTM stack's input), 'lstm' [T N, B, 3h] (the stack's output behind its closing leaky ReLU), 'gl' (L_GL, 0-d)."""
        Q, p3, H1 = self.num_patch * self.num_nodes, 3 * self._feature_width, 3 * self.hidden_dim
        out = self._tap(batch, *{"mpnn": (0, (Q, batch, p3)), "lstm": (1, (batch, Q, H1)), "gl": (2, ())}[which])
        return out.permute(1, 0, 2).contiguous() if which == "lstm" else out          # kept as [B][T N][3h], the layout fc1 reads

    def fused_mse_step(self, x, y, optimizer=None, global_batch=None, theta=0.0, gamma=1.0):
        """train-mode forward + MSE + ``theta`` * L_GL + backward (+ Adam when ``optimizer`` is a FusedAdam over this model) in one C
        call; fills ``self.bucket`` = [grad | loss]; returns (pred [B], loss 0-d tensor) on the device, no host sync."""
        x, yv = self._step_inputs(x, y)
        self._step += 1
        return self._fused_step(x, yv, optimizer, global_batch, True, self._step, theta, gamma)

    def fused_mse_step_args(self, x, y, optimizer=None, theta=0.0, gamma=1.0):
        """What ``fused_mse_step`` would hand to its C call, short of calling: ``(shape, args, rulgnn_adam_args or None, the checked
        tensors the structs point to)``; the step counters advance as there (runs.LOGO_runs: several runs in one grouped call)."""
        x, yv = self._step_inputs(x, y)
        self._step += 1
        return self._fused_step_args(x, yv, optimizer, None, True, self._step, theta, gamma) + ((x, yv),)

    # ---- nn.Module surface -----------------------------------------------------------------------------
    def forward(self, X, GL=False, gamma=1):
        x = self._check_input(X)
        if x.size(0) == 0:
            raise RuntimeError("LOGO_model: empty batch")
        if self.training:
            self._step += 1
        pred, gl = self._predict(x, self.training, self._step, 0.0, float(gamma), autograd=self._needs_grad())
        return (pred, gl) if GL else pred
