"""fp64 numpy oracle of the LOGO family, written from the formulas (reference models/LOGO/Model.py:17-262, algorithms.py:125-136):
forward, ``loss = MSE + theta * L_GL`` and all 46 gradients by hand; the Bi-LSTM forward and BPTT are oracle/hagcn_oracle.py's.  Also a
torch restatement (fp32 noise floor of the gradient gate, timing).

  x [B, N, T p]; graphs g = (b, t): Xg = x[b, :, t p:(t + 1) p]; E = Xg Wn^T + bn; A_T = softmax_row(leaky(E E^T - 1e8 I)) + I
  A_G = Pearson(x[b]) (per sample); z = sig(W_Z_T A_T + W_Z_G A_G), r = sig(W_R_T A_T + W_R_G A_G), A^ = tanh(W_h_T A_G + W_h r)
  C = softmax_row((1 - z) A_T + z A^ - 1e8 I) + I; Hg = leaky((C E) Theta^T + b)
  sequences q = t N + n, steps = samples b: three Bi-LSTM layers with summed halves, dropout behind layers 2 and 3, leaky
  per sample flat [T N 3h] -> fc1, ReLU, fc2, ReLU, cls
  L_GL = mean(D . C) + gamma sqrt(mean(C^2)), D[i, j] = |Xg_i - Xg_j|^2

Dropout: ``keep`` = (keep2 [Q, B, 6h], keep3 [Q, B, 3h]) of zeros and ones over the layers' outputs [q][b][j]; ``keep_masks`` restates the
kernels' counter hash: key = dropout_layer_key(seed, step, site) with site 0 behind bi_lstm2 and 1 behind bi_lstm3, element counter
((q B + b) W + j) mod 2^32, dropped where lowbias32(counter ^ key) < round(p 2^32)."""
import numpy as np

from oracle import hagcn_oracle as HO
from oracle import stgcn_oracle as SO

LEAKY = 0.01
DIAG = 1e8
DROPOUT = 0.2
KEYS = "patch_size num_patch num_nodes hidden_dim".split()
FUSION = ("W_Z_T", "W_Z_G", "W_R_T", "W_R_G", "W_h_T", "W_h")
LSTMS = ("TD.bi_lstm1", "TD.bi_lstm2", "TD.bi_lstm3")


def param_names():
    names = ["nonlin_map.weight", "nonlin_map.bias", "MPNN.theta.0.weight", "MPNN.theta.0.bias"]
    for l in LSTMS:
        for sfx in ("", "_reverse"):
            names += [f"{l}.{w}_l0{sfx}" for w in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    for f in FUSION:
        names += [f"graph_attn_blk.{f}.weight", f"graph_attn_blk.{f}.bias"]
    return names + ["fc.fc1.weight", "fc.fc1.bias", "fc.fc2.weight", "fc.fc2.bias", "cls.weight", "cls.bias"]


state_keys = param_names          # no buffers: the 46 state_dict keys are the 46 parameters


def param_shapes(cfg):
    p, T, N, h = (cfg[k] for k in KEYS)
    s = {"nonlin_map.weight": (2 * p, p), "nonlin_map.bias": (2 * p,), "MPNN.theta.0.weight": (3 * p, 2 * p), "MPNN.theta.0.bias": (3 * p,)}
    for l, (I, H) in zip(LSTMS, ((3 * p, 3 * h), (3 * h, 6 * h), (6 * h, 3 * h))):
        for sfx in ("", "_reverse"):
            s[f"{l}.weight_ih_l0{sfx}"], s[f"{l}.weight_hh_l0{sfx}"] = (4 * H, I), (4 * H, H)
            s[f"{l}.bias_ih_l0{sfx}"] = s[f"{l}.bias_hh_l0{sfx}"] = (4 * H,)
    for f in FUSION:
        s[f"graph_attn_blk.{f}.weight"], s[f"graph_attn_blk.{f}.bias"] = (N, N), (N,)
    s.update({"fc.fc1.weight": (16, 3 * h * T * N), "fc.fc1.bias": (16,), "fc.fc2.weight": (8, 16), "fc.fc2.bias": (8,),
              "cls.weight": (1, 8), "cls.bias": (1,)})
    return {k: s[k] for k in param_names()}


def param_count(cfg):
    return int(sum(int(np.prod(v)) for v in param_shapes(cfg).values()))


def keep_masks(bs, cfg, seed, step, p=DROPOUT):
    """The kernels' two dropout masks, restated (see the module docstring)."""
    Q, h = cfg["num_patch"] * cfg["num_nodes"], cfg["hidden_dim"]
    out = []
    for site, W in ((0, 6 * h), (1, 3 * h)):
        ctr = np.arange(Q * bs * W, dtype=np.uint64).astype(np.uint32)
        key = SO.dropout_layer_key(seed, step, site)
        with np.errstate(over="ignore"):
            keep = SO._lowbias32(ctr ^ np.uint32(key)) >= np.uint32(SO.dropout_threshold(p))
        out.append(keep.reshape(Q, bs, W).astype(np.float64))
    return tuple(out)


def _leaky(v):
    return np.where(v > 0, v, LEAKY * v)


def _dleaky(v):
    return np.where(v > 0, 1.0, LEAKY)


def _softmax(v):
    e = np.exp(v - v.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def _sig(v):
    return 0.5 * (1.0 + np.tanh(0.5 * v))


def pearson(x):
    c = x - x.mean(-1, keepdims=True)
    nrm = np.sqrt((c * c).sum(-1, keepdims=True))
    with np.errstate(invalid="ignore", divide="ignore"):
        return (c @ c.transpose(0, 2, 1)) / (nrm @ nrm.transpose(0, 2, 1))


def _lin(sd, name, v):
    return v @ np.asarray(sd[f"graph_attn_blk.{name}.weight"], np.float64).T + np.asarray(sd[f"graph_attn_blk.{name}.bias"], np.float64)


def forward(sd, x, cfg, training=False, keep=None, p_drop=DROPOUT, gamma=1.0):
    """Everything the backward needs; 'pred' [B, 1], 'gl', taps 'mpnn' [Q, B, 3p] and 'lstm' [Q, B, 3h].  ``keep`` applies only when
    ``training``."""
    sd = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    x = np.asarray(x, np.float64)
    p, T, N, h = (cfg[k] for k in KEYS)
    B = x.shape[0]
    c = {"sd": sd, "B": B}
    AG = np.repeat(pearson(x)[:, None], T, 1).reshape(B * T, N, N)
    Xg = x.reshape(B, N, T, p).transpose(0, 2, 1, 3).reshape(B * T, N, p)
    E = Xg @ sd["nonlin_map.weight"].T + sd["nonlin_map.bias"]
    eye = np.eye(N)[None]
    G = E @ E.transpose(0, 2, 1) - DIAG * eye
    PT = _softmax(_leaky(G))
    AT = PT + eye
    z = _sig(_lin(sd, "W_Z_T", AT) + _lin(sd, "W_Z_G", AG))
    r = _sig(_lin(sd, "W_R_T", AT) + _lin(sd, "W_R_G", AG))
    AH = np.tanh(_lin(sd, "W_h_T", AG) + _lin(sd, "W_h", r))
    PC = _softmax((1 - z) * AT + z * AH - DIAG * eye)
    C = PC + eye
    CE = C @ E
    Hpre = CE @ sd["MPNN.theta.0.weight"].T + sd["MPNN.theta.0.bias"]
    Hg = _leaky(Hpre)                                                   # [B T, N, 3p]
    seq = Hg.reshape(B, T * N, 3 * p).transpose(1, 0, 2)                # [Q, B, 3p]
    o1 = HO.bilstm_sum(seq, sd, LSTMS[0])
    o2 = HO.bilstm_sum(o1, sd, LSTMS[1])
    k2 = k3 = None
    if training and keep is not None:
        k2, k3 = (np.asarray(k, np.float64) / (1.0 - p_drop) for k in keep)
    o2d = o2 if k2 is None else o2 * k2
    o3 = HO.bilstm_sum(o2d, sd, LSTMS[2])
    o3d = o3 if k3 is None else o3 * k3
    td = _leaky(o3d)                                                    # [Q, B, 3h]
    flat = td.transpose(1, 0, 2).reshape(B, -1)
    pre1 = flat @ sd["fc.fc1.weight"].T + sd["fc.fc1.bias"]
    a1 = np.maximum(pre1, 0)
    pre2 = a1 @ sd["fc.fc2.weight"].T + sd["fc.fc2.bias"]
    a2 = np.maximum(pre2, 0)
    pred = a2 @ sd["cls.weight"].T + sd["cls.bias"]
    D = ((Xg[:, :, None, :] - Xg[:, None, :, :]) ** 2).sum(-1)
    gl = (D * C).mean() + gamma * np.sqrt((C * C).mean())
    c.update(AG=AG, Xg=Xg, E=E, G=G, PT=PT, AT=AT, z=z, r=r, AH=AH, PC=PC, C=C, CE=CE, Hpre=Hpre, seq=seq, o1=o1, o2d=o2d, o3d=o3d, k2=k2, k3=k3,
             td=td, flat=flat, pre1=pre1, a1=a1, pre2=pre2, a2=a2, D=D, pred=pred, gl=float(gl), mpnn=seq, lstm=td, gamma=gamma)
    return c


def loss_and_grads(sd, x, y, cfg, theta, keep_mask=None, p_drop=DROPOUT, gamma=1.0):
    """(loss, {name: gradient}, forward cache) of a train-mode step: loss = mean((pred - y)^2) + theta * L_GL."""
    c = forward(sd, x, cfg, True, keep_mask, p_drop, gamma)
    sd = c["sd"]
    p, T, N, h = (cfg[k] for k in KEYS)
    B = c["B"]
    y = np.asarray(y, np.float64).reshape(-1, 1)
    loss = float(((c["pred"] - y) ** 2).mean() + theta * c["gl"])
    g = {}
    dp = 2.0 * (c["pred"] - y) / B
    g["cls.weight"], g["cls.bias"] = dp.T @ c["a2"], dp.sum(0)
    d2 = (dp @ sd["cls.weight"]) * (c["pre2"] > 0)
    g["fc.fc2.weight"], g["fc.fc2.bias"] = d2.T @ c["a1"], d2.sum(0)
    d1 = (d2 @ sd["fc.fc2.weight"]) * (c["pre1"] > 0)
    g["fc.fc1.weight"], g["fc.fc1.bias"] = d1.T @ c["flat"], d1.sum(0)
    dtd = (d1 @ sd["fc.fc1.weight"]).reshape(B, T * N, 3 * h).transpose(1, 0, 2)
    d = dtd * _dleaky(c["o3d"])
    if c["k3"] is not None:
        d = d * c["k3"]
    d, g3 = HO.bilstm_sum_backward(c["o2d"], sd, LSTMS[2], d)
    if c["k2"] is not None:
        d = d * c["k2"]
    d, g2 = HO.bilstm_sum_backward(c["o1"], sd, LSTMS[1], d)
    d, g1 = HO.bilstm_sum_backward(c["seq"], sd, LSTMS[0], d)
    for gg in (g1, g2, g3):
        g.update(gg)
    dH = d.transpose(1, 0, 2).reshape(B * T, N, 3 * p) * _dleaky(c["Hpre"])
    T_ = lambda v: v.transpose(0, 2, 1)
    g["MPNN.theta.0.weight"] = np.einsum("gno,gnc->oc", dH, c["CE"])
    g["MPNN.theta.0.bias"] = dH.sum((0, 1))
    dCE = dH @ sd["MPNN.theta.0.weight"]
    C, E, AT, AG, z, r, AH = c["C"], c["E"], c["AT"], c["AG"], c["z"], c["r"], c["AH"]
    cnt = float(C.size)
    dC = dCE @ T_(E) + theta * (c["D"] / cnt + c["gamma"] * C / (cnt * np.sqrt((C * C).mean())))
    dE = T_(C) @ dCE
    PC = c["PC"]
    dF = PC * (dC - (PC * dC).sum(-1, keepdims=True))
    dz = dF * (AH - AT) * z * (1 - z)
    dAT = dF * (1 - z)
    dh = dF * z * (1 - AH * AH)
    W = lambda n: sd[f"graph_attn_blk.{n}.weight"]

    def lin_grads(name, dpre, inp):
        g[f"graph_attn_blk.{name}.weight"] = np.einsum("gij,gik->jk", dpre, inp)
        g[f"graph_attn_blk.{name}.bias"] = dpre.sum((0, 1))
    lin_grads("W_h", dh, r)
    lin_grads("W_h_T", dh, AG)
    dr = (dh @ W("W_h")) * r * (1 - r)
    lin_grads("W_Z_T", dz, AT)
    lin_grads("W_Z_G", dz, AG)
    lin_grads("W_R_T", dr, AT)
    lin_grads("W_R_G", dr, AG)
    dAT = dAT + dz @ W("W_Z_T") + dr @ W("W_R_T")
    PT = c["PT"]
    dG = PT * (dAT - (PT * dAT).sum(-1, keepdims=True)) * _dleaky(c["G"])
    dE = dE + (dG + T_(dG)) @ E
    g["nonlin_map.weight"] = np.einsum("gnc,gnj->cj", dE, c["Xg"])
    g["nonlin_map.bias"] = dE.sum((0, 1))
    return loss, {k: g[k] for k in param_names()}, c


# ---- torch restatement -------------------------------------------------------------------------------------------------------------------
def _t_bilstm_sum(v, sd, name):
    """nn.LSTM(bidirectional=True, batch_first=True) on v [Q, B, I] with halves summed, through torch's own LSTM kernel."""
    import torch
    ws = [sd[f"{name}.{w}_l0{sfx}"] for sfx in ("", "_reverse") for w in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    H = ws[1].shape[1]
    z = torch.zeros(2, v.shape[0], H, dtype=v.dtype, device=v.device)
    # (train = True: the vendor LSTM on the GPU refuses a backward otherwise; with its own dropout at 0 the flag changes nothing else)
    out = torch._VF.lstm(v, (z, z), ws, True, 1, 0.0, True, True, True)[0]
    return out[..., :H] + out[..., H:]


def torch_forward(sd, x, cfg, keep_scale=None, gamma=1.0):
    """The same forward in torch ops on ``sd``'s tensors (any dtype / device) -> (pred [B, 1], L_GL); autograd differentiates it.
    ``keep_scale`` = (mask2 / (1 - p), mask3 / (1 - p)) or None."""
    import torch
    import torch.nn.functional as Fn
    p, T, N, h = (cfg[k] for k in KEYS)
    B = x.shape[0]
    cen = x - x.mean(-1, keepdim=True)
    nrm = cen.norm(dim=-1, keepdim=True)
    AG = ((cen @ cen.transpose(1, 2)) / (nrm @ nrm.transpose(1, 2))).unsqueeze(1).repeat(1, T, 1, 1).reshape(B * T, N, N)
    Xg = x.reshape(B, N, T, p).transpose(1, 2).reshape(B * T, N, p)
    E = Xg @ sd["nonlin_map.weight"].T + sd["nonlin_map.bias"]
    eye = torch.eye(N, dtype=x.dtype, device=x.device)
    AT = torch.softmax(Fn.leaky_relu(E @ E.transpose(1, 2) - DIAG * eye), -1) + eye
    lin = lambda n, v: v @ sd[f"graph_attn_blk.{n}.weight"].T + sd[f"graph_attn_blk.{n}.bias"]
    z = torch.sigmoid(lin("W_Z_T", AT) + lin("W_Z_G", AG))
    r = torch.sigmoid(lin("W_R_T", AT) + lin("W_R_G", AG))
    AH = torch.tanh(lin("W_h_T", AG) + lin("W_h", r))
    C = torch.softmax((1 - z) * AT + z * AH - DIAG * eye, -1) + eye
    Hg = Fn.leaky_relu((C @ E) @ sd["MPNN.theta.0.weight"].T + sd["MPNN.theta.0.bias"])
    v = Hg.reshape(B, T * N, 3 * p).transpose(0, 1)
    v = _t_bilstm_sum(v, sd, LSTMS[0])
    v = _t_bilstm_sum(v, sd, LSTMS[1])
    if keep_scale is not None:
        v = v * keep_scale[0]
    v = _t_bilstm_sum(v, sd, LSTMS[2])
    if keep_scale is not None:
        v = v * keep_scale[1]
    flat = Fn.leaky_relu(v).transpose(0, 1).reshape(B, -1)
    a = torch.relu(flat @ sd["fc.fc1.weight"].T + sd["fc.fc1.bias"])
    a = torch.relu(a @ sd["fc.fc2.weight"].T + sd["fc.fc2.bias"])
    pred = a @ sd["cls.weight"].T + sd["cls.bias"]
    D = ((Xg.unsqueeze(-3) - Xg.unsqueeze(-2)) ** 2).sum(-1)
    gl = (D * C).mean() + gamma * torch.sqrt((C * C).mean())
    return pred, gl


def torch_grads(sd_np, x, y, cfg, theta, dtype, keep_scale=None):
    """(pred, loss, grads) of the torch restatement on the CPU at ``dtype``: at float32 the noise term of the gradient gate."""
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


def torch_step(sd, opt, x, y, cfg, theta, dropout_p=DROPOUT):
    """One training step of the restatement (timing): forward with two ATen dropout draws, MSE + theta * L_GL, backward, ``opt.step()``."""
    import torch
    opt.zero_grad(set_to_none=True)
    Q, h, B = cfg["num_patch"] * cfg["num_nodes"], cfg["hidden_dim"], x.shape[0]
    keep = tuple((torch.rand(Q, B, W, device=x.device) >= dropout_p).to(x.dtype) / (1.0 - dropout_p) for W in (6 * h, 3 * h))
    pred, gl = torch_forward(sd, x, cfg, keep)
    loss = ((pred - y.reshape(-1, 1)) ** 2).mean() + theta * gl
    loss.backward()
    opt.step()
    return loss
