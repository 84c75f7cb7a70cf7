"""fp64 oracle of the GDAGDL family (reference models/GDAGDL/Model.py, algorithms/algorithms.py:519-544), written from the formulas:
forward, ``MSE + reconstruction`` and the gradient of every one of the 34 live tensors by a hand-written backward (no autograd).
``torch_forward`` restates the same model on torch tensors the way the reference computes it -- the pair tensor ``cat(Wh_i, Wh_j)``
included -- for the fp32 noise floor of the reference's arithmetic and as the ATen baseline of tools/time_gdagdl.py; ``keep_masks``
restates the kernels' dropout masks (counter hash of oracle/stgcn_oracle.py, key = dropout_layer_key(seed, step, layer), counter =
(((sample_offset + b) T + t) N + i) N + j).

x [bs, T * P] -> mag = |STFT| [bs T, N, f] (n_fft = hop = win = nperseg, periodic Hann, reflect-centred) -> c = mag - mean_f(mag),
pcc = c reshape(c, [f, N]) / (|c_i| |c_j|) (the reference reshapes the second operand where a Pearson matrix would transpose it,
Model.py:51: restated as it computes; no epsilon: NaN on an all-zero patch) -> ni = pcc (mag w_ni + b_ni) -> m = (ni > 0), M = m m^T -> per layer
Z = h W^T + b, u_ij = a1 . Z_i + a2 . Z_j + b_att, Pm = softmax_j(leakyrelu(u, 0.1)), Q = Pm o D o M, h = ELU(Q Z) -> Y_o -> encoder /
decoder (reconstruction = mean((Y_o - Y_o')^2)) -> LSTM over the patches -> Linear.
"""
import numpy as np

from oracle import stgcn_oracle as SO

SLOPE = 0.1
CFG_KEYS = ("num_patch", "patch_size", "num_nodes", "nperseg", "input_dim", "gat_layer_dim", "lstm_hidden_dim", "autoencoder_hidden_dim",
            "autoencoder_out_dim")
GRADLESS = ("node_importance_linear.weight", "node_importance_linear.bias")


def param_names(cfg):
    """The reference's named_parameters() / state_dict() order (36 names at three GAT layers)."""
    names = []
    for l in range(len(cfg["gat_layer_dim"])):
        names += [f"gat_layers.{l}.linear.weight", f"gat_layers.{l}.linear.bias", f"gat_layers.{l}.attention.weight",
                  f"gat_layers.{l}.attention.bias"]
    names += list(GRADLESS)
    for mod in ("encoder", "decoder"):
        for i in (0, 2, 4, 6):
            names += [f"{mod}.{i}.weight", f"{mod}.{i}.bias"]
    return names + ["lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0", "lstm.bias_hh_l0", "linear.weight", "linear.bias"]


def flat_names(cfg):
    """The flat layout: the two gradless tensors first."""
    return list(GRADLESS) + [n for n in param_names(cfg) if n not in GRADLESS]


def ae_widths(cfg):
    A, O = cfg["autoencoder_hidden_dim"], cfg["autoencoder_out_dim"]
    D = cfg["num_nodes"] * cfg["gat_layer_dim"][-1]
    return [D, A, A // 2, A // 4, O]


def param_shapes(cfg):
    dims = [cfg["input_dim"]] + list(cfg["gat_layer_dim"])
    sh = {}
    for l in range(len(dims) - 1):
        sh[f"gat_layers.{l}.linear.weight"], sh[f"gat_layers.{l}.linear.bias"] = (dims[l + 1], dims[l]), (dims[l + 1],)
        sh[f"gat_layers.{l}.attention.weight"], sh[f"gat_layers.{l}.attention.bias"] = (1, 2 * dims[l + 1]), (1,)
    sh["node_importance_linear.weight"], sh["node_importance_linear.bias"] = (1, cfg["input_dim"]), (1,)
    w = ae_widths(cfg)
    for k, i in enumerate((0, 2, 4, 6)):
        sh[f"encoder.{i}.weight"], sh[f"encoder.{i}.bias"] = (w[k + 1], w[k]), (w[k + 1],)
        sh[f"decoder.{i}.weight"], sh[f"decoder.{i}.bias"] = (w[3 - k], w[4 - k]), (w[3 - k],)
    E, O, T = cfg["lstm_hidden_dim"], cfg["autoencoder_out_dim"], cfg["num_patch"]
    sh.update({"lstm.weight_ih_l0": (4 * E, O), "lstm.weight_hh_l0": (4 * E, E), "lstm.bias_ih_l0": (4 * E,), "lstm.bias_hh_l0": (4 * E,),
               "linear.weight": (1, E * T), "linear.bias": (1,)})
    return sh


KEYS = param_names          # the families' oracles call their name list KEYS


def noise_partner(name):
    """The tensor whose fp32 noise a one-element tensor shares, or None.  ``attention.bias``'s gradient is the sum of the very ``du``
    terms whose weighted sums form ``attention.weight``'s gradient, and it cancels row by row (the softmax's Jacobian): a single fp32
    run of one scalar is one draw, not a noise level -- it came out 17 times smaller on another CPU -- so the bias is given at least its
    layer's ``attention.weight`` noise."""
    return name[:-len("bias")] + "weight" if name.endswith(".attention.bias") else None


def param_count(cfg):
    return int(sum(np.prod(s) for s in param_shapes(cfg).values()))


def keep_masks(bs, cfg, seed, step, p, sample_offset=0):
    """[layers][bs * T, N, N] keep masks (1 / 0, unscaled) of the attention dropout."""
    T, N = cfg["num_patch"], cfg["num_nodes"]
    n = bs * T * N * N
    out = []
    for layer in range(len(cfg["gat_layer_dim"])):
        ctr = (np.arange(n, dtype=np.uint64) + np.uint64(sample_offset * T * N * N)).astype(np.uint32)
        key = SO.dropout_layer_key(seed, step, layer)
        with np.errstate(over="ignore"):
            keep = SO._lowbias32(ctr ^ np.uint32(key)) >= np.uint32(SO.dropout_threshold(p))
        out.append(keep.reshape(bs * T, N, N).astype(np.float64))
    return out


# ---- pieces ---------------------------------------------------------------------------------------------------------------------------
def stft_mag(x, cfg):
    """[bs * T, N, f] magnitudes, fp64."""
    T, P, ns = cfg["num_patch"], cfg["patch_size"], cfg["nperseg"]
    xp = np.asarray(x, np.float64).reshape(-1, P)
    xp = np.pad(xp, ((0, 0), (ns // 2, ns // 2)), mode="reflect")
    f = 1 + P // ns
    win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(ns) / ns)
    frames = np.stack([xp[:, t * ns:(t + 1) * ns] for t in range(f)], axis=1) * win          # [G, f, ns]
    return np.abs(np.fft.rfft(frames, axis=-1)).transpose(0, 2, 1)                           # [G, N, f]


def graph_mask(mag, w_ni, b_ni):
    """(ni [G, N] -- NaN on a graph with a constant row --, m [G, N] 0 / 1, pcc, lin)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        c = mag - mag.mean(-1, keepdims=True)
        nrm = np.sqrt((c * c).sum(-1))
        pcc = (c @ c.reshape(c.shape[0], c.shape[2], c.shape[1])) / (nrm[:, :, None] * nrm[:, None, :])      # reshaped, not transposed
        lin = mag @ w_ni.reshape(-1) + b_ni.reshape(())
        ni = (pcc * lin[:, None, :]).sum(-1)
        m = (ni > 0).astype(np.float64)
    return ni, m, pcc, lin


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
    """``P``: name -> array.  ``keep``: ``keep_masks`` output (train mode with dropout) or None.  Returns a dict: pred [bs, 1], mse, recon,
    loss (this shard's shares under ``global_batch``), the taps mag / ni / mask / yo / H and, with ``want_grads``, grads name -> array."""
    P = {k: np.asarray(v, np.float64) for k, v in P.items()}
    T, N = cfg["num_patch"], cfg["num_nodes"]
    L = len(cfg["gat_layer_dim"])
    bs = np.asarray(x).shape[0]
    gb = bs if global_batch is None else global_batch
    mag = stft_mag(x, cfg)
    ni, m, _, _ = graph_mask(mag, P["node_importance_linear.weight"], P["node_importance_linear.bias"])
    M = m[:, :, None] * m[:, None, :]
    scale = 1.0 / (1.0 - dropout_p) if keep is not None else 1.0
    h, caches = mag, []
    for l in range(L):
        W, b = P[f"gat_layers.{l}.linear.weight"], P[f"gat_layers.{l}.linear.bias"]
        aw, ab = P[f"gat_layers.{l}.attention.weight"].reshape(-1), P[f"gat_layers.{l}.attention.bias"].reshape(())
        C = W.shape[0]
        Z = h @ W.T + b
        u = (Z @ aw[:C])[:, :, None] + (Z @ aw[C:])[:, None, :] + ab
        Pm = softmax(np.where(u > 0, u, SLOPE * u))
        DM = M * (keep[l] * scale if keep is not None else 1.0)
        Q = Pm * DM
        Hp = Q @ Z
        caches.append((h, Z, u, Pm, DM, Q, Hp))
        h = np.where(Hp > 0, Hp, np.expm1(np.minimum(Hp, 0)))
    Yo = h.reshape(bs, T, -1)
    acts, a = [Yo], Yo
    for k, i in enumerate((0, 2, 4, 6)):
        a = a @ P[f"encoder.{i}.weight"].T + P[f"encoder.{i}.bias"]
        if k < 3:
            a = np.maximum(a, 0)
        acts.append(a)
    H = a
    dacts = [H]
    for k, i in enumerate((0, 2, 4, 6)):
        a = a @ P[f"decoder.{i}.weight"].T + P[f"decoder.{i}.bias"]
        if k < 3:
            a = np.maximum(a, 0)
        dacts.append(a)
    Yp = a
    diff = Yo - Yp
    nel = gb * T * Yo.shape[-1]
    recon = float((diff * diff).sum() / nel)
    hs, lc = lstm_forward(H, P["lstm.weight_ih_l0"], P["lstm.weight_hh_l0"], P["lstm.bias_ih_l0"], P["lstm.bias_hh_l0"])
    pred = hs.reshape(bs, -1) @ P["linear.weight"].T + P["linear.bias"]
    out = {"pred": pred, "recon": recon, "mag": mag.reshape(bs, T, N, -1), "ni": ni.reshape(bs, T, N), "mask": m.reshape(bs, T, N),
           "yo": Yo, "H": H}
    if y is None:
        return out
    yv = np.asarray(y, np.float64).reshape(bs, 1)
    out["mse"] = float(((pred - yv) ** 2).sum() / gb)
    out["loss"] = out["mse"] + recon
    if not want_grads:
        return out
    G = {}
    dpred = 2.0 * (pred - yv) / gb
    G["linear.weight"], G["linear.bias"] = dpred.T @ hs.reshape(bs, -1), dpred.sum(0)
    dhs = (dpred @ P["linear.weight"]).reshape(hs.shape)
    dH, G["lstm.weight_ih_l0"], G["lstm.weight_hh_l0"], dbl = lstm_backward(dhs, H, lc, P["lstm.weight_ih_l0"], P["lstm.weight_hh_l0"])
    G["lstm.bias_ih_l0"], G["lstm.bias_hh_l0"] = dbl, dbl.copy()
    d = -2.0 * diff / nel                                   # d Yp
    dYo = 2.0 * diff / nel
    for k, i in reversed(list(enumerate((0, 2, 4, 6)))):
        if k < 3:
            d = d * (dacts[k + 1] > 0)
        flat_in, flat_d = dacts[k].reshape(-1, dacts[k].shape[-1]), d.reshape(-1, d.shape[-1])
        G[f"decoder.{i}.weight"], G[f"decoder.{i}.bias"] = flat_d.T @ flat_in, flat_d.sum(0)
        d = d @ P[f"decoder.{i}.weight"]
    d = d + dH
    for k, i in reversed(list(enumerate((0, 2, 4, 6)))):
        if k < 3:
            d = d * (acts[k + 1] > 0)
        flat_in, flat_d = acts[k].reshape(-1, acts[k].shape[-1]), d.reshape(-1, d.shape[-1])
        G[f"encoder.{i}.weight"], G[f"encoder.{i}.bias"] = flat_d.T @ flat_in, flat_d.sum(0)
        d = d @ P[f"encoder.{i}.weight"]
    dh = (d + dYo).reshape(bs * T, N, -1)
    for l in range(L - 1, -1, -1):
        hin, Z, u, Pm, DM, Q, Hp = caches[l]
        W = P[f"gat_layers.{l}.linear.weight"]
        aw = P[f"gat_layers.{l}.attention.weight"].reshape(-1)
        C = W.shape[0]
        dHp = dh * np.where(Hp > 0, 1.0, np.exp(np.minimum(Hp, 0)))
        dZ = Q.transpose(0, 2, 1) @ dHp
        dPm = (dHp @ Z.transpose(0, 2, 1)) * DM
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


# ---- inputs whose mask decisions stand three orders above fp32 rounding (fixtures and seeded GPU cases) -----------------------------------
MASK_MARGIN = 1e-3          # |ni_i| >= MASK_MARGIN * sum_j |pcc_ij| |lin_j|: the absolute-sum scale of the node's own dot product


def classify_patches(patches, cfg, w, b):
    """Per patch: kind (0 all live, 1 exactly one, 2 some, 3 none, -1 NaN) and whether the mask margin holds."""
    one = dict(cfg, num_patch=1)
    mag = stft_mag(patches, one)
    ni, m, pcc, lin = graph_mask(mag, w, b)
    with np.errstate(invalid="ignore"):
        ok = (np.abs(ni) >= MASK_MARGIN * (np.abs(pcc) * np.abs(lin)[:, None, :]).sum(-1)).all(-1)
    N = cfg["num_nodes"]
    live = m.sum(-1)
    kind = np.where(live == N, 0, np.where(live == 1, 1, np.where(live > 0, 2, 3)))
    kind = np.where(np.isnan(ni).any(-1), -1, kind)
    return kind, ok & (kind >= 0)


def draw_inputs(cfg, bs, seed, w, b, planted=True):
    """[bs, T * P] fp32 input whose graphs all hold the mask margin (every patch is ``amp * randn + dc``, amp log-uniform in [0.03, 3],
    dc normal(0, amp), drawn until the margin holds); with ``planted`` graphs 0 .. 3 are one of each kind, graph 3 the zero patch."""
    rng = np.random.default_rng(seed + 7)
    T, P = cfg["num_patch"], cfg["patch_size"]
    G = bs * T
    good, by_kind = [], {0: None, 1: None, 2: None}
    while len(good) < G or (planted and any(v is None for v in by_kind.values())):
        amp = np.exp(rng.uniform(np.log(0.03), np.log(3.0), size=(512, 1)))
        cand = (amp * rng.standard_normal((512, P)) + amp * rng.standard_normal((512, 1))).astype(np.float32)
        kind, ok = classify_patches(cand, cfg, w, b)
        for i in np.nonzero(ok)[0]:
            if by_kind.get(int(kind[i]), 0) is None:
                by_kind[int(kind[i])] = cand[i]
            elif len(good) < G:
                good.append(cand[i])
    x = np.stack(good[:G])
    if planted:
        assert G >= 4
        for k in (0, 1, 2):
            x[k] = by_kind[k]
        x[3] = 0.0
    return x.reshape(bs, T * P)


# ---- the same model on torch tensors, computed the reference's way ---------------------------------------------------------------------
def torch_forward(P, x, cfg, keep=None, dropout_p=0.0, torch_dropout=False):
    """``P``: name -> torch tensor (any float dtype / device); ``keep``: list of [bs T, N, N] tensors or None; ``torch_dropout``: draw the
    masks with F.dropout as the reference does (timing).  Returns (pred, recon, taps)."""
    import torch
    import torch.nn.functional as F
    T, Pz, ns = cfg["num_patch"], cfg["patch_size"], cfg["nperseg"]
    bs = x.shape[0]
    dt = P["linear.bias"].dtype
    xx = x.reshape(bs * T, Pz).to(dt)
    win = torch.hann_window(ns, periodic=True, dtype=dt, device=x.device)
    mag = torch.stft(xx, n_fft=ns, hop_length=ns, win_length=ns, window=win, return_complex=True).abs()       # [G, N, f]
    G_, N, f = mag.shape
    c = mag - mag.mean(-1, keepdim=True)
    nrm = torch.norm(c, dim=-1, keepdim=True)
    pcc = torch.bmm(c, c.reshape(G_, f, N)) / torch.bmm(nrm, nrm.transpose(1, 2))
    lin = F.linear(mag.reshape(-1, f), P["node_importance_linear.weight"], P["node_importance_linear.bias"]).reshape(G_, N, 1)
    ni = (pcc @ lin).reshape(G_, N)
    m = (ni > 0).to(dt)
    adj = m.unsqueeze(-1) * m.unsqueeze(-2)
    h = mag
    for l in range(len(cfg["gat_layer_dim"])):
        Wh = F.linear(h, P[f"gat_layers.{l}.linear.weight"], P[f"gat_layers.{l}.linear.bias"])
        C = Wh.shape[-1]
        Wh1 = Wh.unsqueeze(2).repeat(1, 1, N, 1).view(G_, N * N, C)
        Wh2 = Wh.unsqueeze(1).repeat(1, N, 1, 1).view(G_, N * N, C)
        e = F.linear(torch.cat([Wh1, Wh2], dim=2), P[f"gat_layers.{l}.attention.weight"], P[f"gat_layers.{l}.attention.bias"])
        att = F.softmax(F.leaky_relu(e, SLOPE).view(G_, N, N), dim=2)
        if keep is not None:
            att = att * keep[l] / (1.0 - dropout_p)
        elif torch_dropout:
            att = F.dropout(att, dropout_p, training=True)
        h = F.elu(torch.matmul(att * adj, Wh))
    Yo = h.reshape(bs, T, -1)
    a = Yo
    for k, i in enumerate((0, 2, 4, 6)):
        a = F.linear(a, P[f"encoder.{i}.weight"], P[f"encoder.{i}.bias"])
        a = F.relu(a) if k < 3 else a
    H = a
    for k, i in enumerate((0, 2, 4, 6)):
        a = F.linear(a, P[f"decoder.{i}.weight"], P[f"decoder.{i}.bias"])
        a = F.relu(a) if k < 3 else a
    recon = F.mse_loss(Yo, a)
    E = cfg["lstm_hidden_dim"]
    hh = torch.zeros(bs, E, dtype=dt, device=x.device)
    cc = torch.zeros_like(hh)
    outs = []
    for t in range(T):
        z = F.linear(H[:, t], P["lstm.weight_ih_l0"], P["lstm.bias_ih_l0"]) + F.linear(hh, P["lstm.weight_hh_l0"], P["lstm.bias_hh_l0"])
        i_, f_, g_, o_ = z[:, :E].sigmoid(), z[:, E:2 * E].sigmoid(), z[:, 2 * E:3 * E].tanh(), z[:, 3 * E:].sigmoid()
        cc = f_ * cc + i_ * g_
        hh = o_ * cc.tanh()
        outs.append(hh)
    pred = F.linear(torch.stack(outs, 1).reshape(bs, -1), P["linear.weight"], P["linear.bias"])
    return pred, recon, {"mag": mag, "ni": ni, "mask": m, "yo": Yo, "H": H}


def torch_grads(P_np, x, y, cfg, dtype, keep=None, dropout_p=0.0):
    """(pred, mse, recon, grads) of the restatement in ``dtype`` on the CPU: the reference's own arithmetic and its rounding."""
    import torch
    P = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=k not in GRADLESS) for k, v in P_np.items()}
    kp = None if keep is None else [torch.tensor(k, dtype=dtype) for k in keep]
    pred, recon, _ = torch_forward(P, torch.tensor(np.asarray(x), dtype=dtype), cfg, kp, dropout_p)
    mse = torch.nn.functional.mse_loss(pred, torch.tensor(np.asarray(y), dtype=dtype).reshape(-1, 1))
    (mse + recon).backward()
    return (pred.detach().numpy(), float(mse.detach()), float(recon.detach()),
            {k: v.grad.numpy().copy() for k, v in P.items() if k not in GRADLESS})


def torch_step(P, opt, x, y, cfg, dropout_p):
    """One training step of the restatement with torch's own dropout and optimizer (tools/time_gdagdl.py)."""
    import torch
    pred, recon, _ = torch_forward(P, x, cfg, None, dropout_p, torch_dropout=dropout_p > 0)
    loss = torch.nn.functional.mse_loss(pred, y.reshape(-1, 1)) + recon
    opt.zero_grad()
    loss.backward()
    opt.step()
    return loss
