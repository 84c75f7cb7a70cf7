"""Drop-in ``HierCorrPool_bearing_model``: HierCorrPool (hiercorrpool.py) behind an STFT front end, for the bearing datasets.  Every
patch of a raw window goes through ``torch.stft``'s arithmetic (``n_fft = hop = win = nperseg``, periodic Hann, reflect-centred); the
``nperseg / 2 + 1`` frequency bins are the graph's nodes and the ``1 + patch_size // nperseg`` frames of a patch their features, so the
encoder's first block reads ``input_dim * num_nodes`` channels over ``num_patch`` steps.  From there on it is HierCorrPool and runs on
HierCorrPool's code: one kernel of csrc/hiercorrpool.hip (``hcpb_stft_input_kernel``) writes the magnitude straight into the
channel-last, time-padded block-1 input -- the spectrogram exists in no other layout or buffer -- and the encoder, the LDS-resident
graph stage, the head and the backward chain are the shared host chain unchanged.  The STFT is not
differentiated.  Entries ``rulgnn_hcpb_{forward,backward,fwdbwd}_f32`` on HierCorrPool's argument struct.

Mirrors the reference class (models/HierCorrPool_bearing/Model.py:6-67): same constructor ``(patch_size, num_patch, input_dim,
hidden_dim, embedding_dim, num_nodes, nperseg, encoder_conv_kernel, num_nodes_out)``, ``forward(X) -> [bs, 1]`` for any ``X`` with
``numel / bs == num_patch * patch_size``, the same 28 ``state_dict`` keys in the same order and the same initial weights for a torch
seed.  Like the reference, a model whose ``num_nodes`` / ``input_dim`` do not describe the STFT's shape constructs and fails at its
first forward.  Everything hiercorrpool.py says about BatchNorm, the dropout stream, the reshape condition and the missing CPU path
holds here.

Coverage (stated once: ``LIMITS``, mirrored by include/rulgnn.h ``RULGNN_HCPB_MAX_*``): all six reference rows of PHM2012 and XJTU_SY
(``num_patch`` up to 128, ``encoder_conv_kernel * embedding_dim`` up to 720).
"""
from __future__ import annotations

import torch.nn as nn

from . import _lib
from .hiercorrpool import Feature_extractor_1DCNN, Graph_Classification_block, HierCorrPool_model, encoder_lengths

# include/rulgnn.h RULGNN_HCPB_MAX_* (and HierCorrPool's own num_nodes_out and 4 * hidden_dim * num_nodes limits)
LIMITS = {"max_nperseg": 32, "max_nodes": 17, "max_input_dim": 33, "max_num_patch": 128, "max_d": 720, "max_nodes_out": 16,
          "max_c3": 1024}


class HierCorrPool_bearing_model(HierCorrPool_model):
    """HierCorrPool_model's surface (``forward``, ``fused_mse_step``, ``tap``, the autograd path, BatchNorm state) on the ``hcpb``
    entries."""

    def __init__(self, patch_size, num_patch, input_dim, hidden_dim, embedding_dim, num_nodes, nperseg, encoder_conv_kernel, num_nodes_out):
        super(HierCorrPool_model, self).__init__()
        self.patch_size, self.num_patch, self.input_dim = int(patch_size), int(num_patch), int(input_dim)
        self.hidden_dim, self.embedding_dim, self.num_nodes = int(hidden_dim), int(embedding_dim), int(num_nodes)
        self.nperseg, self.encoder_conv_kernel, self.num_nodes_out = int(nperseg), int(encoder_conv_kernel), int(num_nodes_out)
        N, h, e, K, M = self.num_nodes, self.hidden_dim, self.embedding_dim, self.encoder_conv_kernel, self.num_nodes_out
        self.encoder_out_length = encoder_lengths(self.num_patch)[-1]
        if self.encoder_out_length * 4 * h != K * e:
            raise ValueError(f"HierCorrPool_bearing_model: the encoder leaves {self.encoder_out_length} steps of 4 * hidden_dim = {4 * h} "
                             f"features per node, {self.encoder_out_length * 4 * h} in all, but encoder_conv_kernel * embedding_dim = "
                             f"{K * e}: the model's reshape to [encoder_conv_kernel, num_nodes, -1] needs the two to be equal")
        self.feature_dim = K * e
        # same construction order as the reference => same RNG consumption => same initial weights; the sub-modules only hold tensors
        self.Time_Preprocessing = Feature_extractor_1DCNN(self.input_dim * N, h * N, 8, 1, 0.35)
        self.gc1 = Graph_Classification_block(e * K, e * K * 3, N, M)
        self.fc_0 = nn.Linear(K * M * e * 3, e * 3)
        self.fc_1 = nn.Linear(e * 3, 1)
        self.dropout_p = 0.35
        self._bn_channels = (h * N, 2 * h * N, 4 * h * N)
        self._bn = self._nbt = None
        self._track_batchnorm_counters()
        self._init_flat()

    c_family = "hcpb"
    not_covered = ("HierCorrPool_bearing HIP kernels do not cover this configuration (nperseg even, 2 <= nperseg <= {max_nperseg}, "
                   "patch_size > nperseg / 2, num_nodes = nperseg / 2 + 1 <= {max_nodes}, input_dim = 1 + patch_size // nperseg <= "
                   "{max_input_dim}, 2 <= num_patch <= {max_num_patch}, 1 <= num_nodes_out <= {max_nodes_out}, encoder_conv_kernel * "
                   "embedding_dim <= {max_d}, 4 * hidden_dim * num_nodes <= {max_c3}; the graph stage within one compute unit's 160 KB "
                   "of LDS)").format(**LIMITS)

    def _shape(self, batch):
        return _lib.HcpbShape(batch, self.patch_size, self.num_patch, self.input_dim, self.hidden_dim, self.embedding_dim, self.num_nodes,
                              self.nperseg, self.encoder_conv_kernel, self.num_nodes_out)

    def _check_input(self, x):
        self._require_device(x)
        if x.dim() < 1 or x.size(0) < 1 or x.numel() // x.size(0) != self.num_patch * self.patch_size or x.numel() % x.size(0):
            raise RuntimeError(f"expected input with numel / batch == {self.num_patch * self.patch_size}, got {list(x.shape)}")
        ns, P = self.nperseg, self.patch_size
        if ns >= 2 and ns % 2 == 0 and P > ns // 2 and (self.num_nodes, self.input_dim) != (ns // 2 + 1, 1 + P // ns):
            # the reference's shape error at its first forward (conv_block1 meets a tensor of another width)
            raise RuntimeError(f"HierCorrPool_bearing_model: the STFT of a patch of {P} points at nperseg {ns} has (num_nodes, input_dim) = "
                               f"({ns // 2 + 1}, {1 + P // ns}) frequency bins and frames, the model was constructed with "
                               f"({self.num_nodes}, {self.input_dim})")
        return x.reshape(x.size(0), -1).contiguous().float()

    def tap(self, batch, which):
        """HierCorrPool_model's taps and 'stft': the block-1 input [B, num_patch + 8, num_nodes * input_dim], the magnitude
        spectrogram (channel ``n * input_dim + j`` = bin n, frame j) between four zero rows on each side."""
        if which != "stft":
            return super().tap(batch, which)
        return self._tap(batch, 4, (batch, self.num_patch + 8, self.num_nodes * self.input_dim))
