"""fp64 oracle of the HierCorrPool family (pure numpy, imports nothing from the package), written from the formulas and not through
autograd: forward, MSE loss and all 19 parameter gradients, plus a torch restatement of the same forward (timing, fp32 noise).

    x [bs, N, P p] -> encoder input [bs, C0 = N p, P]: in[b][n p + j][t] = x[b][n][t p + j]
    three blocks  Conv1d(k 8, pad 4, no bias) -> BatchNorm1d -> ReLU -> MaxPool1d(2, 2, pad 1) (-> dropout behind block 1)
    F [bs, L', C3] flat per sample -> X [N, d]: X[n][k e + q] = F.flat[(k N + n) e + q],  d = K e = L' 4 h
    G = X X^T, A = softmax_row(leaky(G) off the diagonal) + I
    Z = sigmoid((A X) Wd^T + bd), S = softmax over the NODES of ([A | Z] Wm^T + bm)
    X' = S^T X, A' = S^T A S, H = leaky((A' X') Wt^T + bt), out = leaky(fc_1(leaky(fc_0(H.flat))))

``keep_mask`` [bs, C1, L1] (1 = kept) is the dropout draw behind block 1 at probability ``dropout_p``; None = no dropout.
"""
import numpy as np

SLOPE, EPS, MOMENTUM = 0.01, 1e-5, 0.1
ENC = "Time_Preprocessing.conv_block{}."
P_THETA_W, P_THETA_B = "gc1.Message_Passing.theta.0.weight", "gc1.Message_Passing.theta.0.bias"
P_WD, P_BD = "gc1.Graph_Clustering.dimension_mapping.weight", "gc1.Graph_Clustering.dimension_mapping.bias"
P_WM, P_BM = "gc1.Graph_Clustering.matrix.weight", "gc1.Graph_Clustering.matrix.bias"
ZERO_GRAD = P_BM          # constant along the softmax axis: its gradient is zero in exact arithmetic


def param_names():
    names = []
    for l in (1, 2, 3):
        names += [ENC.format(l) + "0.weight", ENC.format(l) + "1.weight", ENC.format(l) + "1.bias"]
    return names + [P_THETA_W, P_THETA_B, P_WD, P_BD, P_WM, P_BM, "fc_0.weight", "fc_0.bias", "fc_1.weight", "fc_1.bias"]


def state_keys():
    keys = []
    for l in (1, 2, 3):
        keys += [ENC.format(l) + "0.weight"] + [ENC.format(l) + "1." + s for s in ("weight", "bias", "running_mean", "running_var",
                                                                                     "num_batches_tracked")]
    return keys + param_names()[9:]


def lengths(num_patch):
    """Pooled lengths (L1, L2, L3 = L') of the three blocks."""
    out, L = [], num_patch
    for _ in range(3):
        L = (L + 1) // 2 + 1
        out.append(L)
    return out


def _leaky(v):
    return np.where(v > 0, v, SLOPE * v)


def _dleaky(v):
    return np.where(v > 0, 1.0, SLOPE)


def _cols(a):
    """[B, C, L] -> the convolution's windows [B, C, L + 1, 8] (four zeros on each side)."""
    L = a.shape[2]
    ap = np.pad(a, ((0, 0), (0, 0), (4, 4)))
    return np.stack([ap[:, :, k:k + L + 1] for k in range(8)], axis=-1)


def _pool(r):
    """MaxPool1d(2, 2, padding 1) over the last axis: (pooled, index of the winner in the padded pairs); ties go to the first."""
    Lc = r.shape[-1]
    Lp = Lc // 2 + 1
    rp = np.full(r.shape[:-1] + (2 * Lp,), -np.inf)
    rp[..., 1:1 + Lc] = r
    w = rp.reshape(r.shape[:-1] + (Lp, 2))
    arg = np.argmax(w, axis=-1)
    return np.take_along_axis(w, arg[..., None], -1)[..., 0], arg


def _unpool(dp, arg, Lc):
    Lp = dp.shape[-1]
    d = np.zeros(dp.shape[:-1] + (Lp, 2))
    np.put_along_axis(d, arg[..., None], dp[..., None], -1)
    return d.reshape(dp.shape[:-1] + (2 * Lp,))[..., 1:1 + Lc]


def forward(sd, x, cfg, training=True, keep_mask=None, dropout_p=0.35):
    """Returns a dict: pred [bs, 1], taps (encoder [bs, L', C3], pooled_x, pooled_adj, H), the batch statistics of the three BatchNorms
    (``bn_mean`` / ``bn_var`` biased / ``bn_count``) and what the backward needs."""
    f = lambda k: np.asarray(sd[k], np.float64)
    p, P, N, e, K, M = (cfg[k] for k in ("patch_size", "num_patch", "num_nodes", "embedding_dim", "encoder_conv_kernel", "num_nodes_out"))
    x = np.asarray(x, np.float64)
    bs = x.shape[0]
    a = x.reshape(bs, N, P, p).transpose(0, 1, 3, 2).reshape(bs, N * p, P)
    c = {"blocks": [], "bn_mean": [], "bn_var": [], "bn_count": []}
    for l in (1, 2, 3):
        W, gam, bet = f(ENC.format(l) + "0.weight"), f(ENC.format(l) + "1.weight"), f(ENC.format(l) + "1.bias")
        cols = _cols(a)
        z = np.einsum("bctk,ock->bot", cols, W)
        if training:
            mean, var = z.mean(axis=(0, 2)), z.var(axis=(0, 2))
        else:
            mean, var = f(ENC.format(l) + "1.running_mean"), f(ENC.format(l) + "1.running_var")
        inv = 1.0 / np.sqrt(var + EPS)
        xhat = (z - mean[None, :, None]) * inv[None, :, None]
        yv = xhat * gam[None, :, None] + bet[None, :, None]
        pooled, arg = _pool(np.maximum(yv, 0.0))
        scale = None
        if l == 1 and training and keep_mask is not None:
            scale = np.asarray(keep_mask, np.float64) / (1.0 - dropout_p)
            pooled = pooled * scale
        c["blocks"].append(dict(cols=cols, W=W, gam=gam, inv=inv, xhat=xhat, y=yv, arg=arg, scale=scale, Lc=z.shape[2]))
        c["bn_mean"].append(mean); c["bn_var"].append(var); c["bn_count"].append(z.shape[0] * z.shape[2])
        a = pooled
    Fm = a.transpose(0, 2, 1)                                     # [bs, L', C3]
    if Fm.shape[1] * Fm.shape[2] != K * N * e:
        raise ValueError(f"L' 4h = {Fm.shape[1] * Fm.shape[2] // N} but K e = {K * e}")
    X = Fm.reshape(bs, K, N, e).transpose(0, 2, 1, 3).reshape(bs, N, K * e)
    G = X @ X.transpose(0, 2, 1)
    eye = np.eye(N)
    lk = _leaky(G)
    lk_off = np.where(eye[None] > 0, -np.inf, lk)
    ex = np.exp(lk_off - lk_off.max(-1, keepdims=True))
    Pm = ex / ex.sum(-1, keepdims=True)
    A = Pm + eye[None]
    AX = A @ X
    Wd, bd, Wm, bm = f(P_WD), f(P_BD), f(P_WM), f(P_BM)
    Z = 1.0 / (1.0 + np.exp(-(AX @ Wd.T + bd)))
    T = np.concatenate([A, Z], -1) @ Wm.T + bm
    et = np.exp(T - T.max(1, keepdims=True))
    S = et / et.sum(1, keepdims=True)
    St = S.transpose(0, 2, 1)
    Xp = St @ X
    Ap = St @ A @ S
    Q = Ap @ Xp
    Hpre = Q @ f(P_THETA_W).T + f(P_THETA_B)
    H = _leaky(Hpre)
    pre0 = H.reshape(bs, -1) @ f("fc_0.weight").T + f("fc_0.bias")
    a0 = _leaky(pre0)
    pre1 = a0 @ f("fc_1.weight").T + f("fc_1.bias")
    c.update(pred=_leaky(pre1), encoder=Fm, pooled_x=Xp, pooled_adj=Ap, H=H, X=X, G=G, Pm=Pm, A=A, AX=AX, Z=Z, S=S, Q=Q, Hpre=Hpre,
             pre0=pre0, a0=a0, pre1=pre1)
    return c


def loss_and_grads(sd, x, y, cfg, keep_mask=None, dropout_p=0.35):
    """(loss, {parameter name: gradient}, forward dict) of the train-mode step; the loss is mean((pred - y)^2)."""
    f = lambda k: np.asarray(sd[k], np.float64)
    N, e, K, M = (cfg[k] for k in ("num_nodes", "embedding_dim", "encoder_conv_kernel", "num_nodes_out"))
    c = forward(sd, x, cfg, True, keep_mask, dropout_p)
    bs = c["pred"].shape[0]
    y = np.asarray(y, np.float64).reshape(bs, 1)
    diff = c["pred"] - y
    loss = float((diff ** 2).mean())
    g = {}
    d1 = 2.0 * diff / bs * _dleaky(c["pre1"])
    g["fc_1.weight"], g["fc_1.bias"] = d1.T @ c["a0"], d1.sum(0)
    d0 = (d1 @ f("fc_1.weight")) * _dleaky(c["pre0"])
    Hf = c["H"].reshape(bs, -1)
    g["fc_0.weight"], g["fc_0.bias"] = d0.T @ Hf, d0.sum(0)
    dHpre = (d0 @ f("fc_0.weight")).reshape(c["H"].shape) * _dleaky(c["Hpre"])
    g[P_THETA_W] = np.einsum("bmo,bmi->oi", dHpre, c["Q"])
    g[P_THETA_B] = dHpre.sum((0, 1))
    dQ = dHpre @ f(P_THETA_W)
    X, A, S, Z, AX, Pm = c["X"], c["A"], c["S"], c["Z"], c["AX"], c["Pm"]
    Xp, Ap = c["pooled_x"], c["pooled_adj"]
    T_ = lambda v: v.transpose(0, 2, 1)
    dAp = dQ @ T_(Xp)
    dXp = T_(Ap) @ dQ
    dS = X @ T_(dXp) + A @ S @ T_(dAp) + T_(A) @ S @ dAp
    dX = S @ dXp
    dA = S @ dAp @ T_(S)
    dT = S * (dS - (S * dS).sum(1, keepdims=True))
    Wm, Wd = f(P_WM), f(P_WD)
    Wa, Wz = Wm[:, :N], Wm[:, N:]
    g[P_WM] = np.concatenate([np.einsum("bnm,bnj->mj", dT, A), np.einsum("bnm,bnj->mj", dT, Z)], -1)
    g[P_BM] = dT.sum((0, 1))
    dA = dA + dT @ Wa
    dZp = (dT @ Wz) * Z * (1.0 - Z)
    g[P_WD] = np.einsum("bnm,bnd->md", dZp, AX)
    g[P_BD] = dZp.sum((0, 1))
    dAX = dZp @ Wd
    dA = dA + dAX @ T_(X)
    dX = dX + T_(A) @ dAX
    dlk = Pm * (dA - (Pm * dA).sum(-1, keepdims=True))
    dG = dlk * _dleaky(c["G"]) * (1.0 - np.eye(N)[None])
    dX = dX + (dG + T_(dG)) @ X
    dF = dX.reshape(bs, N, K, e).transpose(0, 2, 1, 3).reshape(c["encoder"].shape)
    da = dF.transpose(0, 2, 1)                                    # [bs, C3, L']
    for l in (3, 2, 1):
        b = c["blocks"][l - 1]
        if b["scale"] is not None:
            da = da * b["scale"]
        dy = _unpool(da, b["arg"], b["Lc"]) * (b["y"] > 0)
        g[ENC.format(l) + "1.weight"] = (dy * b["xhat"]).sum((0, 2))
        g[ENC.format(l) + "1.bias"] = dy.sum((0, 2))
        dz = (b["gam"] * b["inv"])[None, :, None] * (dy - dy.mean((0, 2), keepdims=True) - b["xhat"] * (dy * b["xhat"]).mean((0, 2), keepdims=True))
        g[ENC.format(l) + "0.weight"] = np.einsum("bot,bctk->ock", dz, b["cols"])
        if l > 1:
            L = b["cols"].shape[2] - 1
            dap = np.zeros(b["cols"].shape[:2] + (L + 8,))
            for k in range(8):
                dap[:, :, k:k + L + 1] += np.einsum("bot,oc->bct", dz, b["W"][:, :, k])
            da = dap[:, :, 4:4 + L]
    return loss, g, c


def running_after(sd, c, times=1):
    """The BatchNorm buffers after ``times`` identical train-mode forwards with the statistics of ``c``."""
    out = {}
    for l in (1, 2, 3):
        n = c["bn_count"][l - 1]
        rm, rv = np.asarray(sd[ENC.format(l) + "1.running_mean"], np.float64), np.asarray(sd[ENC.format(l) + "1.running_var"], np.float64)
        for _ in range(times):
            rm = (1 - MOMENTUM) * rm + MOMENTUM * c["bn_mean"][l - 1]
            rv = (1 - MOMENTUM) * rv + MOMENTUM * c["bn_var"][l - 1] * (n / (n - 1.0) if n > 1 else 1.0)
        out[ENC.format(l) + "1.running_mean"], out[ENC.format(l) + "1.running_var"] = rm, rv
    return out


def torch_forward(sd, x, cfg, training=True, keep_scale=None, track=False):
    """The same forward in torch ops on ``sd``'s tensors (any dtype / device); autograd differentiates it.  ``keep_scale`` multiplies
    block 1's pooled output (mask / (1 - p)).  Train mode uses batch statistics and leaves the running ones alone unless ``track``."""
    import torch
    import torch.nn.functional as Fn
    p, P, N, e, K = (cfg[k] for k in ("patch_size", "num_patch", "num_nodes", "embedding_dim", "encoder_conv_kernel"))
    bs = x.shape[0]
    a = x.reshape(bs, N, P, p).transpose(1, 2).reshape(bs, P, N * p).transpose(1, 2)
    for l in (1, 2, 3):
        z = Fn.conv1d(a, sd[ENC.format(l) + "0.weight"], padding=4)
        rm, rv = (None, None) if training and not track else (sd[ENC.format(l) + "1.running_mean"], sd[ENC.format(l) + "1.running_var"])
        z = Fn.batch_norm(z, rm, rv, sd[ENC.format(l) + "1.weight"], sd[ENC.format(l) + "1.bias"], training, MOMENTUM, EPS)
        a = Fn.max_pool1d(Fn.relu(z), 2, 2, 1)
        if l == 1 and keep_scale is not None:
            a = a * keep_scale
    X = a.transpose(1, 2).reshape(bs, K, N, -1).transpose(1, 2).reshape(bs, N, -1)
    eye = torch.eye(N, dtype=X.dtype, device=X.device)
    A = torch.softmax(Fn.leaky_relu(X @ X.transpose(1, 2) - 1e8 * eye), -1) + eye
    Z = torch.sigmoid((A @ X) @ sd[P_WD].T + sd[P_BD])
    S = torch.softmax(torch.cat([A, Z], -1) @ sd[P_WM].T + sd[P_BM], -2)
    Xp = S.transpose(1, 2) @ X
    Ap = S.transpose(1, 2) @ A @ S
    H = Fn.leaky_relu((Ap @ Xp) @ sd[P_THETA_W].T + sd[P_THETA_B])
    return Fn.leaky_relu(Fn.leaky_relu(H.reshape(bs, -1) @ sd["fc_0.weight"].T + sd["fc_0.bias"]) @ sd["fc_1.weight"].T + sd["fc_1.bias"])


def torch_grads(sd_np, x, y, cfg, dtype, keep_scale=None):
    """(pred, loss, grads) of the torch restatement on the CPU at ``dtype``: at float32 the noise term of the gradient gate."""
    import torch
    sd = {k: torch.tensor(np.asarray(v), dtype=dtype if np.asarray(v).dtype.kind == "f" else None) for k, v in sd_np.items()}
    names = param_names()
    for k in names:
        sd[k].requires_grad_(True)
    ks = None if keep_scale is None else torch.tensor(keep_scale, dtype=dtype)
    pred = torch_forward(sd, torch.tensor(np.asarray(x), dtype=dtype), cfg, True, ks)
    loss = ((pred - torch.tensor(np.asarray(y), dtype=dtype).reshape(-1, 1)) ** 2).mean()
    grads = torch.autograd.grad(loss, [sd[k] for k in names], allow_unused=True)
    return pred.detach().numpy(), float(loss.detach()), {k: (np.zeros(sd[k].shape) if gr is None else gr.numpy()) for k, gr in zip(names, grads)}


def torch_step(sd, opt, x, y, cfg, dropout_p=0.35):
    """One training step of the restatement (timing): train-mode forward with an ATen dropout draw, running statistics tracked, MSE,
    backward and ``opt.step()``; ``sd`` holds the parameters (requires_grad) and the BatchNorm buffers."""
    import torch
    opt.zero_grad(set_to_none=True)
    C1, L1 = cfg["hidden_dim"] * cfg["num_nodes"], lengths(cfg["num_patch"])[0]
    keep = (torch.rand(x.shape[0], C1, L1, device=x.device) >= dropout_p).to(x.dtype) / (1.0 - dropout_p)
    loss = ((torch_forward(sd, x, cfg, True, keep, track=True) - y.reshape(-1, 1)) ** 2).mean()
    loss.backward()
    opt.step()
    return loss
