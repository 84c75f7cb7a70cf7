"""fp64 oracle of the STFA family (reference models/STFA/Model.py, algorithms/algorithms.py:166-192), written from the formulas: forward
with taps, the MSE loss and the gradient of every one of the 48 tensors by a hand-written backward (no autograd).  ``torch_forward``
restates the same model on torch tensors the way the reference computes it -- the pair tensor ``cat(Wh_i, Wh_j)``, the repeated dense
adjacency, the ``v`` / tanh / singleton-softmax branch included -- for the fp32 noise floor of the reference's arithmetic and as the ATen
baseline of tools/time_stfa.py; ``keep_masks`` restates the kernels' dropout masks (counter hash of oracle/stgcn_oracle.py, key =
dropout_layer_key(seed, step, 0), counter = (((sample_offset + b) T + t) Hd + h) 44 + e with e the directed edge's row-major index:
only the 44 directed edges are drawn).

x [bs, 14, T * P] -> [bs, T, 14, P]: G = bs T graphs -> per head Z = x W^T + b, u_ij = a1 . Z_i + a2 . Z_j + c, p = softmax_j(leakyrelu(u,
0.1)) over all 14 nodes, q = p o D o A, h' = q Z -> relu(mean over heads) -> rows [1 x T | 14 C] -> one LSTM -> Linear(E, 1) on the last step.
"""
import numpy as np

from oracle import stgcn_oracle as SO
from gatlstm_oracle import lstm_backward, lstm_forward, softmax

SLOPE, N = 0.1, 14
CFG_KEYS = ("patch_size", "num_patch", "num_nodes", "hidden_dim", "output_dim", "encoder_hidden_dim", "num_heads", "dropout")
# Model.py:65-68, 1-based
CONNECTIONS = [[1, 2], [1, 12], [1, 4], [1, 9], [1, 5], [1, 3], [2, 4], [2, 7], [2, 8], [2, 13], [3, 14], [3, 13], [3, 10], [3, 6], [4, 7],
               [4, 8], [5, 9], [5, 11], [6, 10], [7, 8], [8, 13], [9, 11]]
LSTM = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


def adjacency():
    A = np.zeros((N, N))
    for i, j in CONNECTIONS:
        A[i - 1, j - 1] = A[j - 1, i - 1] = 1.0
    return A


def param_names(cfg):
    """The reference's named_parameters() / state_dict() order (48 names at ten heads)."""
    names = []
    for h in range(cfg["num_heads"]):
        names += [f"gat.attention_{h}.linear.weight", f"gat.attention_{h}.linear.bias", f"gat.attention_{h}.attention.weight",
                  f"gat.attention_{h}.attention.bias"]
    return names + ["v.weight", "v.bias"] + ["lstm." + n for n in LSTM] + ["fc.weight", "fc.bias"]


KEYS = param_names


def param_shapes(cfg):
    P, T, C, E = cfg["patch_size"], cfg["num_patch"], cfg["output_dim"], cfg["encoder_hidden_dim"]
    W = T + N * C
    sh = {}
    for h in range(cfg["num_heads"]):
        sh[f"gat.attention_{h}.linear.weight"], sh[f"gat.attention_{h}.linear.bias"] = (C, P), (C,)
        sh[f"gat.attention_{h}.attention.weight"], sh[f"gat.attention_{h}.attention.bias"] = (1, 2 * C), (1,)
    sh["v.weight"], sh["v.bias"] = (1, N * C), (1,)
    sh.update({"lstm.weight_ih_l0": (4 * E, W), "lstm.weight_hh_l0": (4 * E, E), "lstm.bias_ih_l0": (4 * E,), "lstm.bias_hh_l0": (4 * E,)})
    sh["fc.weight"], sh["fc.bias"] = (1, E), (1,)
    return sh


def param_count(cfg):
    return int(sum(np.prod(s) for s in param_shapes(cfg).values()))


def noise_partner(name):
    """The tensor whose fp32 noise a one-element tensor shares, or None: ``attention.bias``'s gradient is the sum of the very ``du`` terms
    whose weighted sums form ``attention.weight``'s gradient and cancels row by row (tests/gatlstm_oracle.py: noise_partner)."""
    return name[:-len("bias")] + "weight" if name.endswith(".attention.bias") else None


def keep_masks(bs, cfg, seed, step, p, sample_offset=0):
    """[bs, T, Hd, 14, 14] keep masks (1 / 0, unscaled): the draws on the 44 directed edges, ones elsewhere (where the adjacency
    multiplies zeros)."""
    T, Hd = cfg["num_patch"], cfg["num_heads"]
    edges = np.argwhere(adjacency() > 0)                      # row-major, columns ascending
    assert len(edges) == 44
    n = bs * T * Hd * 44
    ctr = (np.arange(n, dtype=np.uint64) + np.uint64(sample_offset * T * Hd * 44)).astype(np.uint32)
    key = SO.dropout_layer_key(seed, step, 0)
    with np.errstate(over="ignore"):
        keep = (SO._lowbias32(ctr ^ np.uint32(key)) >= np.uint32(SO.dropout_threshold(p))).reshape(bs, T, Hd, 44)
    D = np.ones((bs, T, Hd, N, N))
    D[:, :, :, edges[:, 0], edges[:, 1]] = keep.astype(np.float64)
    return D


def graphs(x, cfg):
    """[bs, 14, T P] -> [bs T, 14, P] (Model.py:95-103)."""
    T, P = cfg["num_patch"], cfg["patch_size"]
    x = np.asarray(x, np.float64)
    return x.reshape(x.shape[0], N, T, P).transpose(0, 2, 1, 3).reshape(-1, N, P)


def forward_backward(Pm, x, y, cfg, keep=None, dropout_p=0.0, global_batch=None, want_grads=True):
    """``Pm``: name -> array.  ``keep``: ``keep_masks`` output (train mode with dropout) or None.  Returns a dict: pred [bs, 1], loss (this
    shard's share under ``global_batch``), the taps gat [bs, T, 14 C] / rows [bs, T, T + 14 C] / lstm [bs, T, E], the arguments of every
    kink (``kinks``: name -> array) and, with ``want_grads``, grads name -> array."""
    Pm = {k: np.asarray(v, np.float64) for k, v in Pm.items()}
    T, C, Hd = cfg["num_patch"], cfg["output_dim"], cfg["num_heads"]
    bs = np.asarray(x).shape[0]
    gb = bs if global_batch is None else global_batch
    xg = graphs(x, cfg)
    A = adjacency()
    scale = 1.0 / (1.0 - dropout_p) if keep is not None else 1.0
    caches, kinks = [], {}
    with np.errstate(invalid="ignore", over="ignore"):
        acc = np.zeros((bs * T, N, C))
        for h in range(Hd):
            W, b = Pm[f"gat.attention_{h}.linear.weight"], Pm[f"gat.attention_{h}.linear.bias"]
            aw, ab = Pm[f"gat.attention_{h}.attention.weight"].reshape(-1), Pm[f"gat.attention_{h}.attention.bias"].reshape(())
            Z = xg @ W.T + b
            u = (Z @ aw[:C])[:, :, None] + (Z @ aw[C:])[:, None, :] + ab
            Pr = softmax(np.where(u > 0, u, SLOPE * u))
            DM = A * (keep.reshape(bs * T, Hd, N, N)[:, h] * scale if keep is not None else 1.0)
            Q = Pr * DM
            caches.append((Z, u, Pr, DM, Q))
            kinks[f"leakyrelu{h}"] = u
            acc = acc + Q @ Z
        M = acc / Hd
        kinks["relu"] = M
        gat = np.where(M < 0, 0.0, M).reshape(bs, T, N * C)           # (a NaN stays a NaN, as F.relu)
        rows = np.concatenate([np.ones((bs, T, T)), gat], -1)
        hs, lc = lstm_forward(rows, *(Pm["lstm." + n] for n in LSTM))
        pred = hs[:, -1] @ Pm["fc.weight"].T + Pm["fc.bias"]
    out = {"gat": gat, "rows": rows, "lstm": hs, "pred": pred, "kinks": kinks}
    if y is None:
        return out
    yv = np.asarray(y, np.float64).reshape(bs, 1)
    out["loss"] = float(((pred - yv) ** 2).sum() / gb)
    if not want_grads:
        return out
    G = {}
    dpred = 2.0 * (pred - yv) / gb
    G["fc.weight"], G["fc.bias"] = dpred.T @ hs[:, -1], dpred.sum(0)
    dhs = np.zeros_like(hs)
    dhs[:, -1] = dpred @ Pm["fc.weight"]
    drows, G["lstm.weight_ih_l0"], G["lstm.weight_hh_l0"], dbl = lstm_backward(dhs, rows, lc, Pm["lstm.weight_ih_l0"], Pm["lstm.weight_hh_l0"])
    G["lstm.bias_ih_l0"], G["lstm.bias_hh_l0"] = dbl, dbl.copy()
    G["v.weight"], G["v.bias"] = np.zeros((1, N * C)), np.zeros(1)        # the softmax over one element is constant
    dH = drows[:, :, T:].reshape(bs * T, N, C) * (M > 0) / Hd
    for h in range(Hd):
        Z, u, Pr, DM, Q = caches[h]
        aw = Pm[f"gat.attention_{h}.attention.weight"].reshape(-1)
        dZ = Q.transpose(0, 2, 1) @ dH
        dP = (dH @ Z.transpose(0, 2, 1)) * DM
        de = Pr * (dP - (dP * Pr).sum(-1, keepdims=True))
        du = de * np.where(u > 0, 1.0, SLOPE)
        ds, dt = du.sum(2), du.sum(1)
        G[f"gat.attention_{h}.attention.bias"] = np.array([du.sum()])
        G[f"gat.attention_{h}.attention.weight"] = np.concatenate([(ds[:, :, None] * Z).sum((0, 1)), (dt[:, :, None] * Z).sum((0, 1))])[None]
        dZ = dZ + ds[:, :, None] * aw[:C] + dt[:, :, None] * aw[C:]
        G[f"gat.attention_{h}.linear.weight"] = dZ.reshape(-1, C).T @ xg.reshape(-1, xg.shape[-1])
        G[f"gat.attention_{h}.linear.bias"] = dZ.sum((0, 1))
    sh = param_shapes(cfg)
    out["grads"] = {k: G[k].reshape(sh[k]) for k in param_names(cfg)}
    return out


def kink_margin(out):
    """min over the kink tensors of min|argument| / (16 * 2^-23 * max|argument|): > 1 means no fp32 evaluation within 16 ulps of the
    tensor's largest magnitude can land on the other side of a leakyrelu or ReLU kink.  Exact zeros are left out: under dropout a ReLU
    argument is exactly zero where every neighbour of a node was dropped in every head, and a sum of exact zeros is zero in any precision."""
    worst = np.inf
    for v in out["kinks"].values():
        v = v[np.isfinite(v) & (v != 0)]
        if v.size:
            worst = min(worst, float(np.abs(v).min() / (16 * 2.0 ** -23 * np.abs(v).max())))
    return worst


def seeded_input(cfg, bs, seed):
    """[bs, 14, T * P] fp32: every sensor a random walk with its own level and step size, like a normalised C-MAPSS window."""
    rng = np.random.default_rng(seed + 7)
    L = cfg["num_patch"] * cfg["patch_size"]
    level = rng.standard_normal((bs, N, 1))
    step = np.exp(rng.uniform(np.log(0.05), np.log(0.5), size=(bs, N, 1)))
    return (level + np.cumsum(step * rng.standard_normal((bs, N, L)), -1)).astype(np.float32)


# ---- the same model on torch tensors, computed the reference's way ---------------------------------------------------------------------
def torch_forward(Pm, x, cfg, keep=None, dropout_p=0.0, torch_dropout=False, vendor_lstm=False):
    """``Pm``: name -> torch tensor (any float dtype / device); ``keep``: [bs T, Hd, 14, 14] tensor or None; ``torch_dropout``: draw the
    masks with F.dropout as the reference does (timing); ``vendor_lstm``: the LSTM through ``torch._VF.lstm``, what the reference's
    ``nn.LSTM`` runs (timing), instead of the step loop written out below.  Returns (pred, taps)."""
    import torch
    import torch.nn.functional as Fn
    T, Pz, C, Hd, E = cfg["num_patch"], cfg["patch_size"], cfg["output_dim"], cfg["num_heads"], cfg["encoder_hidden_dim"]
    bs = x.shape[0]
    dt = Pm["fc.bias"].dtype
    xg = x.to(dt).reshape(bs, N, T, Pz).transpose(1, 2).reshape(bs * T, N, Pz)
    adj = torch.tensor(adjacency(), dtype=dt, device=x.device).unsqueeze(0).repeat(bs * T, 1, 1)
    heads = []
    for h in range(Hd):
        Wh = Fn.linear(xg, Pm[f"gat.attention_{h}.linear.weight"], Pm[f"gat.attention_{h}.linear.bias"])
        # the pair tensor [G, 14 * 14, 2 C]: row (i, j) holds (Wh_i | Wh_j), materialised as the reference materialises it
        pair = torch.cat([Wh[:, :, None, :].expand(-1, -1, N, -1), Wh[:, None, :, :].expand(-1, N, -1, -1)], dim=-1).reshape(bs * T, N * N, 2 * C)
        e = Fn.linear(pair, Pm[f"gat.attention_{h}.attention.weight"], Pm[f"gat.attention_{h}.attention.bias"])
        att = Fn.softmax(Fn.leaky_relu(e, SLOPE).view(bs * T, N, N), dim=2)
        if keep is not None:
            att = att * keep[:, h] / (1.0 - dropout_p)
        elif torch_dropout:
            att = Fn.dropout(att, dropout_p, training=True)
        heads.append(torch.matmul(att * adj, Wh))
    gat = Fn.relu(torch.stack(heads, dim=0).mean(0)).view(bs, T, -1)
    ase = Fn.softmax(Fn.linear(torch.tanh(gat), Pm["v.weight"], Pm["v.bias"]), -1)
    rows = torch.cat([ase.view(bs, -1).unsqueeze(1).repeat(1, T, 1), gat], dim=-1)
    Wih, Whh, bih, bhh = (Pm["lstm." + n] for n in LSTM)
    if vendor_lstm:
        z0 = torch.zeros(1, bs, E, dtype=dt, device=x.device)
        hs = torch._VF.lstm(rows, (z0, z0), [Wih, Whh, bih, bhh], True, 1, 0.0, True, False, True)[0]
    else:
        gi = Fn.linear(rows, Wih, bih)
        hh = torch.zeros(bs, E, dtype=dt, device=x.device)
        cc = torch.zeros_like(hh)
        outs = []
        for t in range(T):
            z = gi[:, t] + Fn.linear(hh, Whh, bhh)
            i_, f_, g_, o_ = z[:, :E].sigmoid(), z[:, E:2 * E].sigmoid(), z[:, 2 * E:3 * E].tanh(), z[:, 3 * E:].sigmoid()
            cc = f_ * cc + i_ * g_
            hh = o_ * cc.tanh()
            outs.append(hh)
        hs = torch.stack(outs, 1)
    return Fn.linear(hs[:, -1, :], Pm["fc.weight"], Pm["fc.bias"]), {"gat": gat, "rows": rows, "lstm": hs}


def torch_grads(P_np, x, y, cfg, dtype, keep=None, p=0.0):
    """(pred, loss, grads) of the restatement in ``dtype`` on the CPU: the reference's own arithmetic and its rounding.  ``keep``:
    ``keep_masks`` output."""
    import torch
    Pm = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in P_np.items()}
    kp = None if keep is None else torch.tensor(keep.reshape((-1,) + keep.shape[2:]), dtype=dtype)
    pred, _ = torch_forward(Pm, torch.tensor(np.asarray(x), dtype=dtype), cfg, kp, p)
    loss = torch.nn.functional.mse_loss(pred, torch.tensor(np.asarray(y), dtype=dtype).reshape(-1, 1))
    loss.backward()
    return pred.detach().numpy(), float(loss.detach()), {k: v.grad.numpy().copy() for k, v in Pm.items()}


def torch_step(Pm, opt, x, y, cfg, dropout_p):
    """One training step of the restatement with torch's own dropout, the vendor LSTM and torch's optimizer (tools/time_stfa.py)."""
    import torch
    pred, _ = torch_forward(Pm, x, cfg, None, dropout_p, torch_dropout=dropout_p > 0, vendor_lstm=True)
    loss = torch.nn.functional.mse_loss(pred, y.reshape(-1, 1))
    opt.zero_grad()
    loss.backward()
    opt.step()
    return loss
