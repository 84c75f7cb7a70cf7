"""Drop-in ``STNet_model`` (a ``ChebNet`` user).  The whole model runs behind three C entries on one flat
parameter buffer (``rulgnn_stnet_{forward,backward,fwdbwd}_f32``; ``fused_mse_step`` is forward + MSE + reconstruction loss +
backward + Adam in one call): the STFT front end, the thresholded adjacency and the Chebyshev terms in the gfx950 kernels of
csrc/stnet.hip, every projection as a matrix-core GEMM, the LSTM over the patches in the persistent kernels of csrc/bilstm.hip.

Mirrors the reference class (models/STNet/Model.py:44-169): same constructor kwargs ``(num_patch, patch_size, num_nodes, nperseg,
input_dim, Cheb_layers, lstm_hidden_dim, autoencoder_hidden_dim)``, ``forward(x, train=False)`` returning the prediction ``[bs, 1]``
or ``(prediction, reconstruction_loss)``, the same ``state_dict`` keys in the same order and -- sub-modules being created in the
reference's order -- the same initial weights for a torch seed.  ``cnn`` (the 1x1 convolution behind the 0.7 threshold) never
receives a gradient, exactly as in the reference.  There is no CPU path: a non-CUDA input raises.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib
from .flat import FlatModule


class ChebNet(nn.Module):
    """Holder of ``filters`` [K, in_channels, out_channels] with the reference's initialisation (Model.py:7-20)."""

    def __init__(self, in_channels, out_channels, K):
        super().__init__()
        self.in_channels, self.out_channels, self.K = in_channels, out_channels, K
        self.filters = nn.Parameter(torch.Tensor(K, in_channels, out_channels))
        nn.init.xavier_uniform_(self.filters)


class STNet_model(FlatModule):
    def __init__(self, num_patch, patch_size, num_nodes, nperseg, input_dim, Cheb_layers, lstm_hidden_dim, autoencoder_hidden_dim):
        super().__init__()
        self.num_patch, self.patch_size, self.nperseg = int(num_patch), int(patch_size), int(nperseg)
        self.num_nodes, self.input_dim = int(num_nodes), int(input_dim)
        self.cheb_layers = [int(c) for c in Cheb_layers]
        self.lstm_hidden_dim, self.autoencoder_hidden_dim = int(lstm_hidden_dim), int(autoencoder_hidden_dim)
        dims = [self.input_dim] + self.cheb_layers
        A = self.autoencoder_hidden_dim
        # same construction order as the reference => same RNG consumption => same initial weights; never called
        self.cnn = nn.Conv2d(in_channels=2, out_channels=1, kernel_size=(1, 1))
        self.chebnets = nn.ModuleList([ChebNet(dims[i], dims[i + 1], 3) for i in range(len(dims) - 1)])
        self.encoder = nn.Sequential(nn.Linear(dims[-1] * self.num_nodes, A), nn.ReLU(), nn.Linear(A, A), nn.ReLU(), nn.Linear(A, A), nn.ReLU(),
                                     nn.Linear(A, A))
        self.decoder = nn.Sequential(nn.Linear(A, A), nn.ReLU(), nn.Linear(A, A), nn.ReLU(), nn.Linear(A, A), nn.ReLU(),
                                     nn.Linear(A, dims[-1] * self.num_nodes))
        self.lstm = nn.LSTM(input_size=A, hidden_size=self.lstm_hidden_dim, batch_first=True)
        self.linear = nn.Linear(self.lstm_hidden_dim * self.num_patch, 1)
        self._init_flat()
        self.optimized_range = (3, self._count)  # cnn.weight [2] + cnn.bias [1] come first and have no gradient

    bucket_tail = 2            # [gradient | loss | reconstruction]
    gradless_params = 2        # cnn.weight, cnn.bias
    # the reconstruction gradients are scaled in place by the backward: one backward per forward
    consumes_tape = True

    @property
    def bucket(self):
        """[gradient | loss]: what one all-reduce carries in data-parallel training (the reconstruction term sits behind it)."""
        return self._grad_flat[:self._count + 1]

    # ---- C-ABI calls -----------------------------------------------------------------------------------
    c_family, Args = "stnet", _lib.StnetArgs
    not_covered = ("STNet HIP kernels do not cover this configuration (num_nodes = nperseg / 2 + 1, input_dim = 1 + patch_size / nperseg, "
                   "even nperseg <= 64, <= 4 ChebNets)")

    def _shape(self, batch):
        s = _lib.StnetShape()
        s.batch, s.num_patch, s.patch_size, s.num_nodes, s.nperseg, s.input_dim = batch, self.num_patch, self.patch_size, self.num_nodes, self.nperseg, self.input_dim
        s.num_cheb = len(self.cheb_layers)
        for i, c in enumerate(self.cheb_layers[:4]):
            s.cheb_layers[i] = c
        s.lstm_hidden_dim, s.autoencoder_hidden_dim = self.lstm_hidden_dim, self.autoencoder_hidden_dim
        return s

    def _check_input(self, x):
        self._require_device(x)
        bs = x.size(0)
        if x.numel() != bs * self.num_patch * self.patch_size:
            raise RuntimeError(f"shape '[{bs}, {self.num_patch}, {self.patch_size}]' is invalid for input of size {x.numel()}")
        if len(self.cheb_layers) > 4:
            raise RuntimeError("STNet HIP kernels cover up to 4 ChebNet layers")
        return x.reshape(bs, self.num_patch * self.patch_size).contiguous().float()

    def _args(self, shp, x, y=None, dpred=None, global_batch=None, recon_weight=None):
        a = super()._args(shp, x, y, dpred, global_batch)
        a.recon = self._grad_flat.data_ptr() + 4 * (self._count + 1)
        a.recon_weight = recon_weight.data_ptr() if recon_weight is not None else None
        return a

    def _run_forward(self, x):
        """(prediction, reconstruction loss): the reconstruction term is a 0-d tensor whose incoming gradient must be 1 (it is a term of
        the reference's loss)."""
        return super()._run_forward(x) + (self._grad_flat[self._count + 1],)

    def _run_backward(self, x, douts):
        # The reconstruction term enters with whatever weight the objective gave it (the reference: 1, algorithms.py:458; a loss on the
        # prediction alone: 0) -- handed to the kernels as a device scalar, no host round trip.
        w = douts[1].reshape(1).contiguous().float()
        return super()._run_backward(x, douts, recon_weight=w)

    # ---- nn.Module surface -----------------------------------------------------------------------------
    def forward(self, x, train=False):
        x2 = self._check_input(x)
        if x2.size(0) == 0:
            raise RuntimeError("STNet_model: empty batch")
        pred, recon = self._predict(x2, autograd=self._needs_grad())
        return (pred, recon) if train else pred
