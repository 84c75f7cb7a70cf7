"""fp64 oracle of the DVGTformer family (reference models/DVGTformer/Model.py, algorithms/algorithms.py:326-351), written from the
formulas: forward, MSE loss and the gradient of every one of the 214 tensors by a hand-written backward (no autograd), UNFOLDED --
Q, K, V, the head concatenation and W_O are formed as the reference forms them, so a wrong fold or unfold in csrc/dvgtformer.hip shows
here.  ``torch_forward`` restates the same model on torch tensors (fp32 noise of the reference's arithmetic, the ATen baseline of
tools/time_dvgtformer.py); ``keep_masks`` restates the kernels' dropout masks (counter hash of oracle/stgcn_oracle.py, key =
dropout_layer_key(seed, step, block), counter = ((sample_offset + b) (L + 1) + l) (N + 1) + n mod 2^32).

x [bs, N, L] -> linear_t over L, transpose, linear_x over N, append the row t_v and the column x_v -> X [bs, L+1, N+1];
A_temp = PCC(X), A_spat = PCC(X^T) BEFORE the positional encoding is added; blocks of (temporal half, spatial half); flatten; head.
A half on tokens T and features F: per head P = softmax((1-lam) softmax(Q K^T / sqrt(d)) + lam softmax(relu(A))), head = P V;
O = concat W_O^T + b; R = LN1(O) + X; D = dropout(R) (temporal halves, train mode); out = LN2(FF(D)) + D.
"""
import math

import numpy as np

from oracle import stgcn_oracle as SO

LN_EPS = 1e-5
INPUT_KEYS = ["t_v", "x_v", "linear_t.weight", "linear_t.bias", "linear_x.weight", "linear_x.bias"]
HEAD_KEYS = ["output_layer.0.weight", "output_layer.0.bias", "output_layer.2.weight", "output_layer.2.bias"]


def half_names(view, blk, heads):
    v = "temp" if view == 0 else "spat"
    pre = f"{'tvgtformer_blocks' if view == 0 else 'svgtformer_blocks'}.{blk}."
    out = []
    for t in "QKV":
        for h in range(heads):
            out += [f"{pre}linears_{t}_{v}.{h}.weight", f"{pre}linears_{t}_{v}.{h}.bias"]
    for leaf in (f"W_O_{v}", f"layer_norm1_{v}", f"layer_norm2_{v}", f"feed_forward_{v}.0", f"feed_forward_{v}.2"):
        out += [f"{pre}{leaf}.weight", f"{pre}{leaf}.bias"]
    return out


def param_names(cfg):
    """The reference's named_parameters() order: the flat layout."""
    names = list(INPUT_KEYS)
    for view in (0, 1):
        for b in range(cfg["num_blocks"]):
            names += half_names(view, b, cfg["num_heads"])
    return names + HEAD_KEYS


def param_shapes(cfg):
    N, L, H = cfg["num_nodes"], cfg["time_length"], cfg["num_heads"]
    sh = {"t_v": (1, 1, N), "x_v": (1, L + 1, 1), "linear_t.weight": (L, L), "linear_t.bias": (L,), "linear_x.weight": (N, N),
          "linear_x.bias": (N,)}
    for view in (0, 1):
        F, d, ff = (N + 1, L + 1)[view], cfg["d_model"][view], cfg["d_ff"][view]
        for b in range(cfg["num_blocks"]):
            names = half_names(view, b, H)
            for i in range(3 * H):
                sh[names[2 * i]], sh[names[2 * i + 1]] = (d, F), (d,)
            rest = names[6 * H:]
            for n_, s in zip(rest, [(F, d * H), (F,), (F,), (F,), (F,), (F,), (ff, F), (ff,), (F, ff), (F,)]):
                sh[n_] = s
    sh.update({"output_layer.0.weight": (100, (L + 1) * (N + 1)), "output_layer.0.bias": (100,), "output_layer.2.weight": (1, 100),
               "output_layer.2.bias": (1,)})
    return sh


KEYS = param_names          # the families' oracles call their name list KEYS


def positional_encoding(Lp, Np):
    """The reference's constant: for i in range(0, N, 2) columns i, i+1 = sin, cos of pos / 10000^((2 i) / (N + 1)) -- the doubled even
    index is the reference's -- rounded to fp32 as torch.zeros holds it; every other column stays 0."""
    pe = np.zeros((Lp, Np), np.float32)
    for pos in range(Lp):
        for i in range(0, Np - 1, 2):
            pe[pos, i] = math.sin(pos / (10000 ** ((2 * i) / Np)))
            pe[pos, i + 1] = math.cos(pos / (10000 ** ((2 * i) / Np)))
    return pe.astype(np.float64)


def keep_masks(bs, cfg, seed, step, p, sample_offset=0):
    """[num_blocks][bs, L+1, N+1] keep masks (1 / 0, unscaled) of the temporal halves' dropout."""
    Lp, Np = cfg["time_length"] + 1, cfg["num_nodes"] + 1
    out = []
    for blk in range(cfg["num_blocks"]):
        ctr = (np.arange(bs * Lp * Np, dtype=np.uint64) + np.uint64(sample_offset * Lp * Np)).astype(np.uint32)
        key = SO.dropout_layer_key(seed, step, blk)
        with np.errstate(over="ignore"):
            keep = SO._lowbias32(ctr ^ np.uint32(key)) >= np.uint32(SO.dropout_threshold(p))
        out.append(keep.reshape(bs, Lp, Np).astype(np.float64))
    return out


# ---- pieces, each with its backward ---------------------------------------------------------------------------------------------------
def _erf(v):
    return np.vectorize(math.erf, otypes=[np.float64])(v)


def gelu(v):
    return 0.5 * v * (1.0 + _erf(v / math.sqrt(2.0)))


def gelu_grad(v):
    return 0.5 * (1.0 + _erf(v / math.sqrt(2.0))) + v * np.exp(-0.5 * v * v) / math.sqrt(2.0 * math.pi)


def softmax(v):
    e = np.exp(v - v.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def softmax_bwd(p, dp):
    return p * (dp - (dp * p).sum(-1, keepdims=True))


def layer_norm(v, g, b):
    mu = v.mean(-1, keepdims=True)
    rs = 1.0 / np.sqrt(((v - mu) ** 2).mean(-1, keepdims=True) + LN_EPS)
    xh = (v - mu) * rs
    return xh * g + b, (xh, rs)


def layer_norm_bwd(dy, g, cache):
    xh, rs = cache
    dxh = dy * g
    dx = (dxh - dxh.mean(-1, keepdims=True) - xh * (dxh * xh).mean(-1, keepdims=True)) * rs
    red = tuple(range(dy.ndim - 1))
    return dx, (dy * xh).sum(red), dy.sum(red)


def pcc(X):
    with np.errstate(invalid="ignore", divide="ignore"):
        c = X - X.mean(-1, keepdims=True)
        n = np.sqrt((c * c).sum(-1, keepdims=True))
        A = (c @ c.swapaxes(-1, -2)) / (n @ n.swapaxes(-1, -2))
    return A, (c, n)


def pcc_bwd(dA, A, cache):
    c, n = cache
    dD = dA / (n @ n.swapaxes(-1, -2))
    w = dA * A
    dn = -(w.sum(-1, keepdims=True) + w.sum(-2)[..., None]) / n
    dc = (dD + dD.swapaxes(-1, -2)) @ c + dn * c / n
    return dc - dc.mean(-1, keepdims=True)


def _half_forward(P, names, X, A, cfg, view, keep, scale):
    H, d, lam = cfg["num_heads"], cfg["d_model"][view], cfg["lambda_param"]
    G = softmax(np.maximum(A, 0.0))
    heads, cache = [], {"X": X, "A": A, "G": G, "h": []}
    for h in range(H):
        Wq, bq, Wk, bk, Wv, bv = (P[names[2 * (t * H + h) + j]] for t in range(3) for j in range(2))
        Q, K, V = X @ Wq.T + bq, X @ Wk.T + bk, X @ Wv.T + bv
        P1 = softmax(Q @ K.swapaxes(-1, -2) / math.sqrt(d))
        Pm = softmax((1.0 - lam) * P1 + lam * G)
        heads.append(Pm @ V)
        cache["h"].append((Q, K, V, P1, Pm))
    WO, bO, g1, b1, g2, b2, W1, c1, W2, c2 = (P[n_] for n_ in names[6 * H:])
    cat = np.concatenate(heads, -1)
    O = cat @ WO.T + bO
    R, ln1 = layer_norm(O, g1, b1)
    R = R + X
    D = R * keep * scale if keep is not None else R
    pre = D @ W1.T + c1
    act = gelu(pre)
    FF = act @ W2.T + c2
    out, ln2 = layer_norm(FF, g2, b2)
    cache.update(cat=cat, ln1=ln1, ln2=ln2, D=D, pre=pre, act=act, keep=keep, scale=scale)
    return out + D, cache


def _half_backward(P, names, dout, cache, cfg, view, grads):
    H, d, lam = cfg["num_heads"], cfg["d_model"][view], cfg["lambda_param"]
    WO, bO, g1, b1, g2, b2, W1, c1, W2, c2 = (P[n_] for n_ in names[6 * H:])
    nWO, nbO, ng1, nb1, ng2, nb2, nW1, nc1, nW2, nc2 = names[6 * H:]
    s2 = lambda a, b: np.einsum("bti,btj->ij", a, b)         # sum over batch and tokens of the outer products
    dFF, grads[ng2], grads[nb2] = layer_norm_bwd(dout, g2, cache["ln2"])
    dD = dout.copy()
    grads[nW2], grads[nc2] = s2(dFF, cache["act"]), dFF.sum(tuple(range(dFF.ndim - 1)))
    dpre = (dFF @ W2) * gelu_grad(cache["pre"])
    grads[nW1], grads[nc1] = s2(dpre, cache["D"]), dpre.sum(tuple(range(dpre.ndim - 1)))
    dD = dD + dpre @ W1
    dR = dD * cache["keep"] * cache["scale"] if cache["keep"] is not None else dD
    dO, grads[ng1], grads[nb1] = layer_norm_bwd(dR, g1, cache["ln1"])
    dX = dR.copy()
    grads[nWO], grads[nbO] = s2(dO, cache["cat"]), dO.sum(tuple(range(dO.ndim - 1)))
    dcat = dO @ WO
    X, G = cache["X"], cache["G"]
    dG = np.zeros_like(G)
    for h in range(H):
        Q, K, V, P1, Pm = cache["h"][h]
        Wq, bq, Wk, bk, Wv, bv = (P[names[2 * (t * H + h) + j]] for t in range(3) for j in range(2))
        dhead = dcat[..., h * d:(h + 1) * d]
        dPm = dhead @ V.swapaxes(-1, -2)
        dV = Pm.swapaxes(-1, -2) @ dhead
        dZ = softmax_bwd(Pm, dPm)
        dG += lam * dZ
        dS = softmax_bwd(P1, (1.0 - lam) * dZ) / math.sqrt(d)
        dQ, dK = dS @ K, dS.swapaxes(-1, -2) @ Q
        for t, dT, W in ((0, dQ, Wq), (1, dK, Wk), (2, dV, Wv)):
            grads[names[2 * (t * H + h)]] = s2(dT, X)
            grads[names[2 * (t * H + h) + 1]] = dT.sum(tuple(range(dT.ndim - 1)))
            dX += dT @ W
    dA = softmax_bwd(G, dG) * (cache["A"] > 0)
    return dX, dA


def forward_backward(P, x, y, cfg, keep=None, dropout_p=0.0, global_batch=None, want_grads=True):
    """P: name -> fp64 array (reference shapes).  keep: ``keep_masks`` (train mode) or None.  Returns a dict with pred [bs], loss,
    taps (x0, enc, a_temp, a_spat) and, with ``want_grads``, grads: name -> array of the parameter's shape."""
    P = {k: np.asarray(v, np.float64) for k, v in P.items()}
    x, N, L, nb, H = np.asarray(x, np.float64), cfg["num_nodes"], cfg["time_length"], cfg["num_blocks"], cfg["num_heads"]
    bs = x.shape[0]
    scale = 1.0 / (1.0 - dropout_p) if keep is not None else 1.0
    X1 = x @ P["linear_t.weight"].T + P["linear_t.bias"]                         # [bs, N, L]
    X2 = X1.swapaxes(1, 2) @ P["linear_x.weight"].T + P["linear_x.bias"]           # [bs, L, N]
    Xc = np.concatenate([X2, np.broadcast_to(P["t_v"].reshape(1, 1, N), (bs, 1, N))], 1)
    Xc = np.concatenate([Xc, np.broadcast_to(P["x_v"].reshape(1, L + 1, 1), (bs, L + 1, 1))], 2)
    At, ct = pcc(Xc)
    As, cs = pcc(Xc.swapaxes(1, 2))
    X = Xc + positional_encoding(L + 1, N + 1)
    out = {"x0": X, "a_temp": At, "a_spat": As}
    caches = []
    for b in range(nb):
        X, c0 = _half_forward(P, half_names(0, b, H), X, At, cfg, 0, keep[b] if keep is not None else None, scale)
        Xs, c1 = _half_forward(P, half_names(1, b, H), X.swapaxes(1, 2), As, cfg, 1, None, 1.0)
        X = Xs.swapaxes(1, 2)
        caches.append((c0, c1))
    out["enc"] = X
    flat = X.reshape(bs, -1)
    hpre = flat @ P["output_layer.0.weight"].T + P["output_layer.0.bias"]
    hact = gelu(hpre)
    pred = (hact @ P["output_layer.2.weight"].T + P["output_layer.2.bias"]).reshape(bs)
    out["pred"] = pred
    if y is None:
        return out
    gb = float(global_batch if global_batch is not None else bs)
    err = pred - np.asarray(y, np.float64).reshape(bs)
    out["loss"] = float((err * err).sum() / gb)
    if not want_grads:
        return out
    g = {}
    dpred = (2.0 * err / gb)[:, None]
    g["output_layer.2.weight"], g["output_layer.2.bias"] = dpred.T @ hact, dpred.sum(0)
    dh = (dpred @ P["output_layer.2.weight"]) * gelu_grad(hpre)
    g["output_layer.0.weight"], g["output_layer.0.bias"] = dh.T @ flat, dh.sum(0)
    dX = (dh @ P["output_layer.0.weight"]).reshape(bs, L + 1, N + 1)
    out["d_enc"] = dX
    dAt, dAs = np.zeros_like(At), np.zeros_like(As)
    for b in reversed(range(nb)):
        c0, c1 = caches[b]
        dXs, dA = _half_backward(P, half_names(1, b, H), dX.swapaxes(1, 2), c1, cfg, 1, g)
        dAs += dA
        dX, dA = _half_backward(P, half_names(0, b, H), dXs.swapaxes(1, 2), c0, cfg, 0, g)
        dAt += dA
    dXc = dX + pcc_bwd(dAt, At, ct) + pcc_bwd(dAs, As, cs).swapaxes(1, 2)
    g["x_v"] = dXc[:, :, N].sum(0).reshape(1, L + 1, 1)
    g["t_v"] = dXc[:, L, :N].sum(0).reshape(1, 1, N)
    dX2 = dXc[:, :L, :N]
    g["linear_x.weight"] = np.einsum("blm,bnl->mn", dX2, X1)
    g["linear_x.bias"] = dX2.sum((0, 1))
    dX1 = (dX2 @ P["linear_x.weight"]).swapaxes(1, 2)                             # [bs, N, L]
    g["linear_t.weight"] = np.einsum("bnk,bnl->kl", dX1, x)
    g["linear_t.bias"] = dX1.sum((0, 1))
    sh = param_shapes(cfg)
    out["grads"] = {k: g[k].reshape(sh[k]) for k in param_names(cfg)}
    return out


# ---- the same model on torch tensors (fp32 noise, the ATen baseline) ------------------------------------------------------------------
def torch_forward(P, x, cfg, keep=None, dropout_p=0.0, torch_dropout=False):
    """P: name -> torch tensor (any dtype / device, requires_grad as the caller likes); returns pred [bs, 1].  ``keep``: the kernels'
    masks (``keep_masks``); ``torch_dropout``: torch's own Bernoulli dropout at ``dropout_p`` instead (the timing baseline)."""
    import torch
    N, L, nb, H, lam = cfg["num_nodes"], cfg["time_length"], cfg["num_blocks"], cfg["num_heads"], cfg["lambda_param"]
    bs = x.shape[0]

    def tpcc(X):
        c = X - X.mean(-1, keepdim=True)
        n = torch.norm(c, dim=-1, keepdim=True)
        return torch.bmm(c, c.transpose(1, 2)) / torch.bmm(n, n.transpose(1, 2))

    def half(X, A, view, b, mask):
        names, d = half_names(view, b, H), cfg["d_model"][view]
        G = torch.softmax(torch.relu(A), -1)
        heads = []
        for h in range(H):
            Wq, bq, Wk, bk, Wv, bv = (P[names[2 * (t * H + h) + j]] for t in range(3) for j in range(2))
            Q, K, V = X @ Wq.T + bq, X @ Wk.T + bk, X @ Wv.T + bv
            P1 = torch.softmax(torch.bmm(Q, K.transpose(1, 2)) / math.sqrt(d), -1)
            heads.append(torch.bmm(torch.softmax((1 - lam) * P1 + lam * G, -1), V))
        WO, bO, g1, b1, g2, b2, W1, c1, W2, c2 = (P[n_] for n_ in names[6 * H:])
        F = X.shape[-1]
        R = torch.nn.functional.layer_norm(torch.cat(heads, -1) @ WO.T + bO, (F,), g1, b1, LN_EPS) + X
        if mask is not None:
            R = R * mask
        elif torch_dropout and view == 0:
            R = torch.nn.functional.dropout(R, dropout_p)
        FF = torch.nn.functional.gelu(R @ W1.T + c1) @ W2.T + c2
        return torch.nn.functional.layer_norm(FF, (F,), g2, b2, LN_EPS) + R

    X = (x @ P["linear_t.weight"].T + P["linear_t.bias"]).transpose(1, 2) @ P["linear_x.weight"].T + P["linear_x.bias"]
    X = torch.cat([X, P["t_v"].reshape(1, 1, N).expand(bs, -1, -1)], 1)
    X = torch.cat([X, P["x_v"].reshape(1, L + 1, 1).expand(bs, -1, -1)], 2)
    At, As = tpcc(X), tpcc(X.transpose(1, 2))
    X = X + torch.as_tensor(positional_encoding(L + 1, N + 1), dtype=X.dtype, device=X.device)
    for b in range(nb):
        mask = None
        if keep is not None:
            mask = torch.as_tensor(keep[b] / (1.0 - dropout_p), dtype=X.dtype, device=X.device)
        X = half(X, At, 0, b, mask)
        X = half(X.transpose(1, 2), As, 1, b, None).transpose(1, 2)
    h = torch.nn.functional.gelu(X.reshape(bs, -1) @ P["output_layer.0.weight"].T + P["output_layer.0.bias"])
    return h @ P["output_layer.2.weight"].T + P["output_layer.2.bias"]


def torch_grads(P_np, x, y, cfg, dtype, keep=None, dropout_p=0.0):
    """pred, loss and name -> gradient of the torch restatement's autograd at ``dtype`` on the CPU."""
    import torch
    P = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in P_np.items()}
    pred = torch_forward(P, torch.tensor(np.asarray(x), dtype=dtype), cfg, keep, dropout_p)
    loss = torch.nn.functional.mse_loss(pred, torch.tensor(np.asarray(y), dtype=dtype).reshape(-1, 1))
    loss.backward()
    return pred.detach().numpy().reshape(-1), float(loss.detach()), {k: v.grad.numpy() for k, v in P.items()}


def torch_step(P, opt, x, y, cfg, dropout_p):
    """One training step of the restatement as a user of the reference runs it: forward (torch dropout), MSE, backward, optimizer."""
    import torch
    loss = torch.nn.functional.mse_loss(torch_forward(P, x, cfg, dropout_p=dropout_p, torch_dropout=True), y.reshape(-1, 1))
    opt.zero_grad()
    loss.backward()
    opt.step()
    return loss
