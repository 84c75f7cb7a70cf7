"""fp64 numpy oracle of the LOGO_bearing family (reference models/LOGO_bearing/Model.py:263-347, algorithms.py:601-629): an STFT
magnitude written from the formula, feeding tests/logo_oracle.py with ``patch_size = input_dim``.  Nothing of LOGO is restated here.

  x [B, T P] -> per patch mag [N, f] = |sum_m w[m] xpad[j ns + m] e^{-2 pi i k m / ns}|, xpad = the patch reflect-padded by ns / 2
  on both sides without repeating the edge sample, w = periodic Hann, N = ns / 2 + 1 bins k, f = 1 + P // ns frames j
  -> LOGO's window X[b, n, t f + j] = mag[b, t, n, j]

Also the torch restatement (``torch.stft`` + logo_oracle.torch_forward: fp32 noise floor of the gradient gate, timing)."""
import numpy as np

import logo_oracle as LO

KEYS = "patch_size num_patch input_dim num_nodes nperseg hidden_dim".split()
param_names, state_keys = LO.param_names, LO.state_keys


def logo_cfg(cfg):
    """The LOGO configuration behind the front end: nodes = frequency bins, patch_size = frames."""
    return dict(patch_size=cfg["input_dim"], num_patch=cfg["num_patch"], num_nodes=cfg["num_nodes"], hidden_dim=cfg["hidden_dim"])


def stft_shape(cfg):
    return cfg["nperseg"] // 2 + 1, 1 + cfg["patch_size"] // cfg["nperseg"]


def param_shapes(cfg):
    return LO.param_shapes(logo_cfg(cfg))


def param_count(cfg):
    return LO.param_count(logo_cfg(cfg))


def keep_masks(bs, cfg, seed, step, p=LO.DROPOUT):
    return LO.keep_masks(bs, logo_cfg(cfg), seed, step, p)


def stft_mag(x, cfg):
    """[B, T, N, f] in fp64."""
    P, T, ns = cfg["patch_size"], cfg["num_patch"], cfg["nperseg"]
    N, f = stft_shape(cfg)
    x = np.asarray(x, np.float64)
    xp = np.pad(x.reshape(x.shape[0], T, P), ((0, 0), (0, 0), (ns // 2, ns // 2)), mode="reflect")
    m = np.arange(ns)
    w = 0.5 - 0.5 * np.cos(2 * np.pi * m / ns)
    frames = np.stack([xp[..., j * ns:(j + 1) * ns] for j in range(f)], -2) * w                   # [B, T, f, ns]
    basis = np.exp(-2j * np.pi * np.outer(np.arange(N), m) / ns)                                  # [N, ns]
    return np.abs(np.einsum("btjm,km->btkj", frames, basis))


def window(x, cfg):
    """LOGO's input [B, N, T f]."""
    mag = stft_mag(x, cfg)
    B, T, N, f = mag.shape
    return mag.transpose(0, 2, 1, 3).reshape(B, N, T * f)


def forward(sd, x, cfg, training=False, keep=None, p_drop=LO.DROPOUT, gamma=1.0):
    return LO.forward(sd, window(x, cfg), logo_cfg(cfg), training, keep, p_drop, gamma)


def loss_and_grads(sd, x, y, cfg, theta, keep_mask=None, p_drop=LO.DROPOUT, gamma=1.0):
    return LO.loss_and_grads(sd, window(x, cfg), y, logo_cfg(cfg), theta, keep_mask, p_drop, gamma)


# ---- torch restatement -------------------------------------------------------------------------------------------------------------------
def torch_window(x, cfg):
    """The reference's front end (Model.py:289-309) -> LOGO's input [B, N, T f]."""
    import torch
    ns, T = cfg["nperseg"], cfg["num_patch"]
    B = x.shape[0]
    z = torch.stft(x.reshape(B * T, cfg["patch_size"]), n_fft=ns, hop_length=ns, win_length=ns,
                   window=torch.hann_window(ns, periodic=True, dtype=x.dtype, device=x.device), return_complex=True).abs()
    return z.reshape(B, T, z.shape[-2], z.shape[-1]).transpose(1, 2).reshape(B, z.shape[-2], -1)


def torch_forward(sd, x, cfg, keep_scale=None, gamma=1.0):
    return LO.torch_forward(sd, torch_window(x, cfg), logo_cfg(cfg), keep_scale, gamma)


def torch_grads(sd_np, x, y, cfg, theta, dtype, keep_scale=None):
    """(pred, loss, grads) of the torch restatement on the CPU at ``dtype``, ``torch.stft`` included."""
    import torch
    sd = {k: torch.tensor(np.asarray(v), dtype=dtype) for k, v in sd_np.items()}
    names = param_names()
    for k in names:
        sd[k].requires_grad_(True)
    ks = None if keep_scale is None else tuple(torch.tensor(np.asarray(k), dtype=dtype) for k in keep_scale)
    pred, gl = torch_forward(sd, torch.tensor(np.asarray(x), dtype=dtype), cfg, ks)
    loss = ((pred - torch.tensor(np.asarray(y), dtype=dtype).reshape(-1, 1)) ** 2).mean() + theta * gl
    grads = torch.autograd.grad(loss, [sd[k] for k in names])
    return pred.detach().numpy(), float(loss.detach()), {k: gr.numpy() for k, gr in zip(names, grads)}


def torch_step(sd, opt, x, y, cfg, theta, dropout_p=LO.DROPOUT):
    """One training step of the restatement (timing): ``torch.stft``, then logo_oracle.torch_step."""
    return LO.torch_step(sd, opt, torch_window(x, cfg), y, logo_cfg(cfg), theta, dropout_p)
