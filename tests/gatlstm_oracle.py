"""fp64 oracle of the GAT_LSTM family (reference models/GAT_LSTM/Model.py, algorithms/algorithms.py:492-517), written from the formulas:
forward with taps, the MSE loss and the gradient of every one of the 22 tensors by a hand-written backward (no autograd).
``torch_forward`` restates the same model on torch tensors the way the reference computes it -- the pair tensor ``cat(Wh_i, Wh_j)`` and
the dense adjacency included -- for the fp32 noise floor of the reference's arithmetic and as the ATen baseline of
tools/time_gatlstm.py; ``keep_masks`` restates the kernels' dropout masks (counter hash of oracle/stgcn_oracle.py, key =
dropout_layer_key(seed, step, layer), counter = ((sample_offset + b) T + i) 3 + (j - i + 1): only the band is drawn).

x [bs, T * P] -> 11 statistics per patch (mean, unbiased std, (mean sqrt|x|)^2, rms, (max - min) / 2, skewness, kurtosis, crest,
clearance, shape and impulse factor; no epsilon: NaN on a constant patch) -> one graph per sample, adj_ij = [|i - j| <= 1] -> per layer
Z = h W^T + b, u_ij = a1 . Z_i + a2 . Z_j + c, p = softmax_j(leakyrelu(u, 0.1)) over all j, q = p o D o adj, h = leakyrelu(q Z, 0.01)
-> stacked one-layer LSTMs over the T nodes -> Linear(E_last T -> 1).
"""
import numpy as np

from oracle import stgcn_oracle as SO

SLOPE, OUT_SLOPE, F = 0.1, 0.01, 11
CFG_KEYS = ("num_patch", "patch_size", "hidden_dim", "lstm_hidden_dim", "dropout")


def param_names(cfg):
    """The reference's named_parameters() / state_dict() order (22 names at three GAT and two LSTM layers)."""
    names = []
    for l in range(len(cfg["hidden_dim"])):
        names += [f"gat_layers.{l}.linear.weight", f"gat_layers.{l}.linear.bias", f"gat_layers.{l}.attention.weight",
                  f"gat_layers.{l}.attention.bias"]
    for k in range(len(cfg["lstm_hidden_dim"])):
        names += [f"lstm_layers.{k}.weight_ih_l0", f"lstm_layers.{k}.weight_hh_l0", f"lstm_layers.{k}.bias_ih_l0", f"lstm_layers.{k}.bias_hh_l0"]
    return names + ["fc.weight", "fc.bias"]


KEYS = param_names          # the families' oracles call their name list KEYS


def param_shapes(cfg):
    dims = [F] + list(cfg["hidden_dim"])
    ld = [dims[-1]] + list(cfg["lstm_hidden_dim"])
    sh = {}
    for l in range(len(dims) - 1):
        sh[f"gat_layers.{l}.linear.weight"], sh[f"gat_layers.{l}.linear.bias"] = (dims[l + 1], dims[l]), (dims[l + 1],)
        sh[f"gat_layers.{l}.attention.weight"], sh[f"gat_layers.{l}.attention.bias"] = (1, 2 * dims[l + 1]), (1,)
    for k in range(len(ld) - 1):
        E = ld[k + 1]
        sh.update({f"lstm_layers.{k}.weight_ih_l0": (4 * E, ld[k]), f"lstm_layers.{k}.weight_hh_l0": (4 * E, E),
                   f"lstm_layers.{k}.bias_ih_l0": (4 * E,), f"lstm_layers.{k}.bias_hh_l0": (4 * E,)})
    sh["fc.weight"], sh["fc.bias"] = (1, ld[-1] * cfg["num_patch"]), (1,)
    return sh


def param_count(cfg):
    return int(sum(np.prod(s) for s in param_shapes(cfg).values()))


def noise_partner(name):
    """The tensor whose fp32 noise a one-element tensor shares, or None: ``attention.bias``'s gradient is the sum of the very ``du`` terms
    whose weighted sums form ``attention.weight``'s gradient and cancels row by row (tests/gdagdl_oracle.py: noise_partner)."""
    return name[:-len("bias")] + "weight" if name.endswith(".attention.bias") else None


def keep_masks(bs, cfg, seed, step, p, sample_offset=0):
    """[layers][bs, T, 3] keep masks (1 / 0, unscaled) of the band entries (i, i - 1 + b)."""
    T = cfg["num_patch"]
    n = bs * T * 3
    out = []
    for layer in range(len(cfg["hidden_dim"])):
        ctr = (np.arange(n, dtype=np.uint64) + np.uint64(sample_offset * T * 3)).astype(np.uint32)
        key = SO.dropout_layer_key(seed, step, layer)
        with np.errstate(over="ignore"):
            keep = SO._lowbias32(ctr ^ np.uint32(key)) >= np.uint32(SO.dropout_threshold(p))
        out.append(keep.reshape(bs, T, 3).astype(np.float64))
    return out


def band(T):
    return (np.abs(np.arange(T)[:, None] - np.arange(T)[None, :]) <= 1).astype(np.float64)


def dense_keep(k3):
    """[bs, T, 3] band draws -> [bs, T, T] (ones off the band, where the adjacency multiplies zeros)."""
    bs, T, _ = k3.shape
    D = np.ones((bs, T, T))
    for b in range(3):
        for i in range(T):
            j = i - 1 + b
            if 0 <= j < T:
                D[:, i, j] = k3[:, i, b]
    return D


# ---- pieces ---------------------------------------------------------------------------------------------------------------------------
def features(x, cfg):
    """[bs, T, 11] in fp64; NaN where the reference divides 0 by 0."""
    T, m = cfg["num_patch"], cfg["patch_size"]
    d = np.asarray(x, np.float64).reshape(-1, m)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = d.mean(-1)
        c = d - mean[:, None]
        std = np.sqrt((c * c).sum(-1) / (m - 1))
        rmsa = np.sqrt(np.abs(d)).mean(-1) ** 2
        rms = np.sqrt((d * d).mean(-1))
        p2p = 0.5 * (d.max(-1) - d.min(-1))
        cs = m / ((m - 1) * (m - 2))
        ck = (m * (m + 1) - 3 * (m - 1) ** 3) / ((m - 1) * (m - 2) * (m - 3))
        skew = cs * (c ** 3).sum(-1) / std ** 3
        kurt = ck * (c ** 4).sum(-1) / std ** 4
        mxa, mab = np.abs(d).max(-1), np.abs(d).mean(-1)
        f = np.stack([mean, std, rmsa, rms, p2p, skew, kurt, mxa / rms, mxa / rmsa, rms / mab, mxa / mab], -1)
    return f.reshape(-1, T, F)


def softmax(v):
    e = np.exp(v - v.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def _sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def lstm_forward(xs, Wih, Whh, bih, bhh):
    B, T, _ = xs.shape
    E = Whh.shape[1]
    h, c = np.zeros((B, E)), np.zeros((B, E))
    cache, outs = [], []
    for t in range(T):
        z = xs[:, t] @ Wih.T + h @ Whh.T + bih + bhh
        i, f, g, o = _sig(z[:, :E]), _sig(z[:, E:2 * E]), np.tanh(z[:, 2 * E:3 * E]), _sig(z[:, 3 * E:])
        c2 = f * c + i * g
        h2 = o * np.tanh(c2)
        cache.append((h, c, i, f, g, o, c2))
        h, c = h2, c2
        outs.append(h)
    return np.stack(outs, 1), cache


def lstm_backward(dout, xs, cache, Wih, Whh):
    B, T, _ = xs.shape
    E = Whh.shape[1]
    dWih, dWhh, db = np.zeros_like(Wih), np.zeros_like(Whh), np.zeros(4 * E)
    dx = np.zeros_like(xs)
    dh, dc = np.zeros((B, E)), np.zeros((B, E))
    for t in range(T - 1, -1, -1):
        hp, cp, i, f, g, o, c2 = cache[t]
        dh = dh + dout[:, t]
        tc = np.tanh(c2)
        dc = dc + dh * o * (1 - tc * tc)
        dz = np.concatenate([dc * g * i * (1 - i), dc * cp * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)], 1)
        dWih += dz.T @ xs[:, t]
        dWhh += dz.T @ hp
        db += dz.sum(0)
        dx[:, t] = dz @ Wih
        dh = dz @ Whh
        dc = dc * f
    return dx, dWih, dWhh, db


def forward_backward(P, x, y, cfg, keep=None, dropout_p=0.0, global_batch=None, want_grads=True):
    """``P``: name -> array.  ``keep``: ``keep_masks`` output (train mode with dropout) or None.  Returns a dict: pred [bs, 1], loss (this
    shard's share under ``global_batch``), the taps feat / h0.. / lstm and, with ``want_grads``, grads name -> array."""
    P = {k: np.asarray(v, np.float64) for k, v in P.items()}
    T = cfg["num_patch"]
    L, K = len(cfg["hidden_dim"]), len(cfg["lstm_hidden_dim"])
    bs = np.asarray(x).shape[0]
    gb = bs if global_batch is None else global_batch
    feat = features(x, cfg)
    adj = band(T)
    scale = 1.0 / (1.0 - dropout_p) if keep is not None else 1.0
    out = {"feat": feat}
    h, caches = feat, []
    with np.errstate(invalid="ignore"):
        for l in range(L):
            W, b = P[f"gat_layers.{l}.linear.weight"], P[f"gat_layers.{l}.linear.bias"]
            aw, ab = P[f"gat_layers.{l}.attention.weight"].reshape(-1), P[f"gat_layers.{l}.attention.bias"].reshape(())
            C = W.shape[0]
            Z = h @ W.T + b
            u = (Z @ aw[:C])[:, :, None] + (Z @ aw[C:])[:, None, :] + ab
            Pm = softmax(np.where(u > 0, u, SLOPE * u))
            DM = adj * (dense_keep(keep[l]) * scale if keep is not None else 1.0)
            Q = Pm * DM
            Y = Q @ Z
            caches.append((h, Z, u, Pm, DM, Q, Y))
            h = np.where(Y > 0, Y, OUT_SLOPE * Y)
            out[f"h{l}"] = h
        xs, lcs = h, []
        for k in range(K):
            hs, lc = lstm_forward(xs, *(P[f"lstm_layers.{k}.{n}"] for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")))
            lcs.append((xs, lc))
            xs = hs
        pred = xs.reshape(bs, -1) @ P["fc.weight"].T + P["fc.bias"]
    out.update(pred=pred, lstm=xs)
    if y is None:
        return out
    yv = np.asarray(y, np.float64).reshape(bs, 1)
    out["loss"] = float(((pred - yv) ** 2).sum() / gb)
    if not want_grads:
        return out
    G = {}
    dpred = 2.0 * (pred - yv) / gb
    G["fc.weight"], G["fc.bias"] = dpred.T @ xs.reshape(bs, -1), dpred.sum(0)
    d = (dpred @ P["fc.weight"]).reshape(xs.shape)
    for k in range(K - 1, -1, -1):
        xin, lc = lcs[k]
        d, G[f"lstm_layers.{k}.weight_ih_l0"], G[f"lstm_layers.{k}.weight_hh_l0"], dbl = lstm_backward(
            d, xin, lc, P[f"lstm_layers.{k}.weight_ih_l0"], P[f"lstm_layers.{k}.weight_hh_l0"])
        G[f"lstm_layers.{k}.bias_ih_l0"], G[f"lstm_layers.{k}.bias_hh_l0"] = dbl, dbl.copy()
    dh = d
    for l in range(L - 1, -1, -1):
        hin, Z, u, Pm, DM, Q, Y = caches[l]
        W = P[f"gat_layers.{l}.linear.weight"]
        aw = P[f"gat_layers.{l}.attention.weight"].reshape(-1)
        C = W.shape[0]
        dY = dh * np.where(Y > 0, 1.0, OUT_SLOPE)
        dZ = Q.transpose(0, 2, 1) @ dY
        dPm = (dY @ Z.transpose(0, 2, 1)) * DM
        de = Pm * (dPm - (dPm * Pm).sum(-1, keepdims=True))
        du = de * np.where(u > 0, 1.0, SLOPE)
        ds, dt = du.sum(2), du.sum(1)
        G[f"gat_layers.{l}.attention.bias"] = np.array([du.sum()])
        G[f"gat_layers.{l}.attention.weight"] = np.concatenate([(ds[:, :, None] * Z).sum((0, 1)), (dt[:, :, None] * Z).sum((0, 1))])[None]
        dZ = dZ + ds[:, :, None] * aw[:C] + dt[:, :, None] * aw[C:]
        G[f"gat_layers.{l}.linear.weight"] = dZ.reshape(-1, C).T @ hin.reshape(-1, hin.shape[-1])
        G[f"gat_layers.{l}.linear.bias"] = dZ.sum((0, 1))
        dh = dZ @ W
    out["grads"] = {k: G[k].reshape(param_shapes(cfg)[k]) for k in G}
    return out


def seeded_input(cfg, bs, seed):
    """[bs, T * P] fp32: every patch ``amp * randn + dc`` with amp log-uniform in [0.03, 3] and dc normal(0, amp)."""
    rng = np.random.default_rng(seed + 7)
    G, P = bs * cfg["num_patch"], cfg["patch_size"]
    amp = np.exp(rng.uniform(np.log(0.03), np.log(3.0), size=(G, 1)))
    return (amp * rng.standard_normal((G, P)) + amp * rng.standard_normal((G, 1))).astype(np.float32).reshape(bs, -1)


# ---- the same model on torch tensors, computed the reference's way ---------------------------------------------------------------------
def torch_features(data):
    import torch
    m = data.shape[1]
    mean = torch.mean(data, dim=-1)
    std = torch.std(data, dim=-1)
    rmsa = torch.mean(torch.sqrt(torch.abs(data)), dim=-1) ** 2
    rms = torch.sqrt(torch.mean(data ** 2, dim=-1))
    p2p = 0.5 * (torch.max(data, dim=-1).values - torch.min(data, dim=-1).values)
    c = data - mean.unsqueeze(-1)
    skew = m / ((m - 1) * (m - 2)) * torch.sum(c ** 3, dim=-1) / (std ** 3)
    kurt = (m * (m + 1) - 3 * (m - 1) ** 3) / ((m - 1) * (m - 2) * (m - 3)) * torch.sum(c ** 4, dim=-1) / (std ** 4)
    mxa, mab = torch.max(torch.abs(data), dim=-1).values, torch.mean(torch.abs(data), dim=-1)
    return torch.stack([mean, std, rmsa, rms, p2p, skew, kurt, mxa / rms, mxa / rmsa, rms / mab, mxa / mab], dim=-1)


def torch_forward(P, x, cfg, keep=None, dropout_p=0.0, torch_dropout=False, vendor_lstm=False):
    """``P``: name -> torch tensor (any float dtype / device); ``keep``: list of dense [bs, T, T] tensors or None; ``torch_dropout``: draw
    the masks with F.dropout as the reference does (timing); ``vendor_lstm``: the LSTM layers through ``torch._VF.lstm``, what the
    reference's ``nn.LSTM`` runs (timing), instead of the step loop written out below.  Returns (pred, taps)."""
    import torch
    import torch.nn.functional as Fn
    T, Pz = cfg["num_patch"], cfg["patch_size"]
    bs = x.shape[0]
    dt = P["fc.bias"].dtype
    h = torch_features(x.reshape(bs * T, Pz).to(dt)).reshape(bs, T, -1)
    taps = {"feat": h}
    adj = torch.eye(T, device=x.device, dtype=dt).unsqueeze(0).repeat(bs, 1, 1)
    idx = torch.arange(T - 1, device=x.device)
    adj[:, idx, idx + 1] = 1
    adj[:, idx + 1, idx] = 1
    for l in range(len(cfg["hidden_dim"])):
        Wh = Fn.linear(h, P[f"gat_layers.{l}.linear.weight"], P[f"gat_layers.{l}.linear.bias"])
        C = Wh.shape[-1]
        Wh1 = Wh.unsqueeze(2).repeat(1, 1, T, 1).view(bs, T * T, C)
        Wh2 = Wh.unsqueeze(1).repeat(1, T, 1, 1).view(bs, T * T, C)
        e = Fn.linear(torch.cat([Wh1, Wh2], dim=2), P[f"gat_layers.{l}.attention.weight"], P[f"gat_layers.{l}.attention.bias"])
        att = Fn.softmax(Fn.leaky_relu(e, SLOPE).view(bs, T, T), dim=2)
        if keep is not None:
            att = att * keep[l] / (1.0 - dropout_p)
        elif torch_dropout:
            att = Fn.dropout(att, dropout_p, training=True)
        h = Fn.leaky_relu(torch.matmul(att * adj, Wh))
        taps[f"h{l}"] = h
    for k in range(len(cfg["lstm_hidden_dim"])):
        E = cfg["lstm_hidden_dim"][k]
        Wih, Whh, bih, bhh = (P[f"lstm_layers.{k}.{n}"] for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"))
        if vendor_lstm:
            z0 = torch.zeros(1, bs, E, dtype=dt, device=x.device)
            # (train = True: the vendor LSTM on the GPU refuses a backward otherwise; with its own dropout at 0 the flag changes nothing else)
            h = torch._VF.lstm(h, (z0, z0), [Wih, Whh, bih, bhh], True, 1, 0.0, True, False, True)[0]
            continue
        gi = Fn.linear(h, Wih, bih)
        hh = torch.zeros(bs, E, dtype=dt, device=x.device)
        cc = torch.zeros_like(hh)
        outs = []
        for t in range(T):
            z = gi[:, t] + Fn.linear(hh, Whh, bhh)
            i_, f_, g_, o_ = z[:, :E].sigmoid(), z[:, E:2 * E].sigmoid(), z[:, 2 * E:3 * E].tanh(), z[:, 3 * E:].sigmoid()
            cc = f_ * cc + i_ * g_
            hh = o_ * cc.tanh()
            outs.append(hh)
        h = torch.stack(outs, 1)
    taps["lstm"] = h
    return Fn.linear(h.reshape(bs, -1), P["fc.weight"], P["fc.bias"]), taps


def torch_grads(P_np, x, y, cfg, dtype, keep=None, dropout_p=0.0):
    """(pred, loss, grads) of the restatement in ``dtype`` on the CPU: the reference's own arithmetic and its rounding.  ``keep``:
    ``keep_masks`` output."""
    import torch
    P = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in P_np.items()}
    kp = None if keep is None else [torch.tensor(dense_keep(k), dtype=dtype) for k in keep]
    pred, _ = torch_forward(P, torch.tensor(np.asarray(x), dtype=dtype), cfg, kp, dropout_p)
    loss = torch.nn.functional.mse_loss(pred, torch.tensor(np.asarray(y), dtype=dtype).reshape(-1, 1))
    loss.backward()
    return pred.detach().numpy(), float(loss.detach()), {k: v.grad.numpy().copy() for k, v in P.items()}


def torch_step(P, opt, x, y, cfg, dropout_p):
    """One training step of the restatement with torch's own dropout, the vendor LSTM and torch's optimizer (tools/time_gatlstm.py)."""
    import torch
    pred, _ = torch_forward(P, x, cfg, None, dropout_p, torch_dropout=dropout_p > 0, vendor_lstm=True)
    loss = torch.nn.functional.mse_loss(pred, y.reshape(-1, 1))
    opt.zero_grad()
    loss.backward()
    opt.step()
    return loss
