"""fp64 numpy oracle of the HierCorrPool_bearing family (reference models/HierCorrPool_bearing/Model.py:6-67, algorithms.py:633-658):
tests/logo_bearing_oracle.py's STFT magnitude feeding tests/hiercorrpool_oracle.py with ``patch_size = input_dim``.  Neither part is
restated here.

  x [B, P p] -> per patch mag [N, f] (logo_bearing_oracle.stft_mag: N = ns / 2 + 1 bins, f = 1 + p // ns frames)
  -> HierCorrPool's window X[b, n, t f + j] = mag[b, t, n, j], whose encoder input channel is n f + j at step t

Also the torch restatement (``torch.stft`` + hiercorrpool_oracle.torch_forward: fp32 noise floor of the gradient gate, timing)."""
import numpy as np

import hiercorrpool_oracle as HO
import logo_bearing_oracle as SO

KEYS = "patch_size num_patch input_dim hidden_dim embedding_dim num_nodes nperseg encoder_conv_kernel num_nodes_out".split()
param_names, state_keys, lengths, running_after = HO.param_names, HO.state_keys, HO.lengths, HO.running_after
ZERO_GRAD, ENC = HO.ZERO_GRAD, HO.ENC


def core_cfg(cfg):
    """The HierCorrPool configuration behind the front end: nodes = frequency bins, patch_size = frames."""
    return dict({k: cfg[k] for k in KEYS if k != "nperseg"}, patch_size=cfg["input_dim"])


def stft_shape(cfg):
    return SO.stft_shape(cfg)


def stft_mag(x, cfg):
    """[B, P, N, f] in fp64."""
    return SO.stft_mag(np.asarray(x).reshape(np.asarray(x).shape[0], -1), cfg)


def block1_input(x, cfg):
    """What the packing kernel writes: [B, P + 8, N f], the magnitude at channel n f + j between four zero rows on each side."""
    mag = stft_mag(x, cfg)
    B, P, N, f = mag.shape
    return np.pad(mag.reshape(B, P, N * f), ((0, 0), (4, 4), (0, 0)))


def window(x, cfg):
    """HierCorrPool's input [B, N, P f]."""
    return SO.window(np.asarray(x).reshape(np.asarray(x).shape[0], -1), cfg)


def forward(sd, x, cfg, training=True, keep_mask=None, dropout_p=0.35):
    return HO.forward(sd, window(x, cfg), core_cfg(cfg), training, keep_mask, dropout_p)


def loss_and_grads(sd, x, y, cfg, keep_mask=None, dropout_p=0.35):
    return HO.loss_and_grads(sd, window(x, cfg), y, core_cfg(cfg), keep_mask, dropout_p)


# ---- torch restatement -------------------------------------------------------------------------------------------------------------------
def torch_window(x, cfg):
    """The reference's front end (Model.py:27-43) -> HierCorrPool's input [B, N, P f]."""
    return SO.torch_window(x.reshape(x.shape[0], -1), cfg)


def torch_forward(sd, x, cfg, training=True, keep_scale=None, track=False):
    return HO.torch_forward(sd, torch_window(x, cfg), core_cfg(cfg), training, keep_scale, track)


def torch_grads(sd_np, x, y, cfg, dtype, keep_scale=None):
    """(pred, loss, grads) of the torch restatement on the CPU at ``dtype``, ``torch.stft`` included (it is not differentiated: x
    carries no gradient)."""
    import torch
    win = torch_window(torch.tensor(np.asarray(x), dtype=dtype), cfg).numpy()
    return HO.torch_grads(sd_np, win, y, core_cfg(cfg), dtype, keep_scale)


def torch_step(sd, opt, x, y, cfg, dropout_p=0.35):
    """One training step of the restatement (timing): ``torch.stft``, then hiercorrpool_oracle.torch_step."""
    return HO.torch_step(sd, opt, torch_window(x, cfg), y, core_cfg(cfg), dropout_p)
