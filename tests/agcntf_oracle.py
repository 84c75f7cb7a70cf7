"""Independent restatement of AGCN_TF (reference models/AGCN_TF/Model.py:137-189, algorithms/algorithms.py:574-599) in numpy float64,
with a hand-written backward: what the gfx950 kernels of csrc/agcntf.hip are tested against beyond the reference fixtures.

It follows the reference's LITERAL order -- it does form the adjacencies A_t [P, P] and A_s [40, 40] and multiplies them into the
features -- which is what makes it an independent check of the kernels' reassociation A X = U (W2^T X) + 1 (b2^T X)^T.  The features are
oracle.sagcn_oracle.extract_features (the front end is SAGCN's, tie rule included).

`torch_step` is the same step as vectorised ATen calls on whatever device its tensors live on: the yardstick of tools/time_agcntf.py.
"""
from dataclasses import dataclass

import numpy as np

from oracle.sagcn_oracle import extract_features

F = 40
SLOPE = 0.01


def param_names(heads=1):
    names = []
    for m in ("attention_spa_adj.0", "attention_spa_adj.2", "attention_tem_adj.0", "attention_tem_adj.2", "spatial_gnn.theta.0",
              "temporal_gnn.theta.0"):
        names += [m + ".weight", m + ".bias"]
    for i in range(heads):
        for w in ("W_q", "W_k", "W_v"):
            names += [f"self_attention.heads.{i}.{w}.weight", f"self_attention.heads.{i}.{w}.bias"]
    return names + ["fc.weight", "fc.bias"]


def param_shapes(P, Ha, Hg, heads=1):
    s = {"attention_spa_adj.0.weight": (Ha, P), "attention_spa_adj.0.bias": (Ha,), "attention_spa_adj.2.weight": (F, Ha),
         "attention_spa_adj.2.bias": (F,), "attention_tem_adj.0.weight": (Ha, F), "attention_tem_adj.0.bias": (Ha,),
         "attention_tem_adj.2.weight": (P, Ha), "attention_tem_adj.2.bias": (P,), "spatial_gnn.theta.0.weight": (Hg, P),
         "spatial_gnn.theta.0.bias": (Hg,), "temporal_gnn.theta.0.weight": (Hg, F), "temporal_gnn.theta.0.bias": (Hg,)}
    for i in range(heads):
        for w in ("W_q", "W_k", "W_v"):
            s[f"self_attention.heads.{i}.{w}.weight"] = (Hg, Hg)
            s[f"self_attention.heads.{i}.{w}.bias"] = (Hg,)
    s["fc.weight"] = (1, Hg * heads * (P + F))
    s["fc.bias"] = (1,)
    return s


def random_params(P, Ha, Hg, heads=1, seed=0, dtype=np.float64):
    """nn.Linear-like ranges (uniform within 1 / sqrt(fan_in)), except the layers that see the unit-norm features (entries ~ 1 / sqrt(40 P)):
    those are scaled up so that every branch carries signal of order one."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, shape in param_shapes(P, Ha, Hg, heads).items():
        fan = shape[1] if len(shape) > 1 else shape[0]
        v = rng.uniform(-1, 1, size=shape) / np.sqrt(fan)
        if name.startswith(("attention_spa_adj.0", "attention_tem_adj.0", "spatial_gnn", "temporal_gnn")) and name.endswith("weight"):
            v = v * np.sqrt(F * P)
        out[name] = v.astype(dtype)
    return out


def flatten(p, heads=1):
    return np.concatenate([np.asarray(p[k]).reshape(-1) for k in param_names(heads)])


def unflatten(flat, P, Ha, Hg, heads=1):
    out, o = {}, 0
    shapes = param_shapes(P, Ha, Hg, heads)
    for k in param_names(heads):
        n = int(np.prod(shapes[k]))
        out[k] = np.asarray(flat[o:o + n]).reshape(shapes[k])
        o += n
    assert o == len(flat)
    return out


def heads_of(p):
    return sum(1 for k in p if k.endswith("W_q.weight"))


@dataclass
class Forward:
    feat: np.ndarray = None       # [bs, P, 40]
    Ut: np.ndarray = None
    At: np.ndarray = None         # [bs, P, P]
    Mt: np.ndarray = None         # A_t X [bs, P, 40]
    Us: np.ndarray = None
    As: np.ndarray = None         # [bs, 40, 40]
    Ms: np.ndarray = None         # A_s X^T [bs, 40, P]
    H: np.ndarray = None          # [bs, N, Hg], spatial rows first
    Q: list = None
    K: list = None
    V: list = None
    prob: list = None             # per head [bs, N, N]
    O: np.ndarray = None          # [bs, N, heads * Hg]
    pred: np.ndarray = None       # [bs, 1]


def _lrelu(v):
    return np.where(v > 0, v, SLOPE * v)


def forward(p, x, num_patch, patch_size):
    fw = Forward()
    bs = x.shape[0]
    nh = heads_of(p)
    X = fw.feat = extract_features(x.reshape(bs, -1), num_patch, patch_size)
    Xt = X.transpose(0, 2, 1)
    fw.Us = np.tanh(Xt @ p["attention_spa_adj.0.weight"].T + p["attention_spa_adj.0.bias"])
    fw.As = fw.Us @ p["attention_spa_adj.2.weight"].T + p["attention_spa_adj.2.bias"]
    fw.Ut = np.tanh(X @ p["attention_tem_adj.0.weight"].T + p["attention_tem_adj.0.bias"])
    fw.At = fw.Ut @ p["attention_tem_adj.2.weight"].T + p["attention_tem_adj.2.bias"]
    fw.Ms = fw.As @ Xt
    fw.Mt = fw.At @ X
    Hs = _lrelu(fw.Ms @ p["spatial_gnn.theta.0.weight"].T + p["spatial_gnn.theta.0.bias"])
    Ht = _lrelu(fw.Mt @ p["temporal_gnn.theta.0.weight"].T + p["temporal_gnn.theta.0.bias"])
    H = fw.H = np.concatenate([Hs, Ht], 1)
    d = H.shape[2]
    fw.Q, fw.K, fw.V, fw.prob, outs = [], [], [], [], []
    for i in range(nh):
        pre = f"self_attention.heads.{i}."
        Q = H @ p[pre + "W_q.weight"].T + p[pre + "W_q.bias"]
        K = H @ p[pre + "W_k.weight"].T + p[pre + "W_k.bias"]
        V = H @ p[pre + "W_v.weight"].T + p[pre + "W_v.bias"]
        s = Q @ K.transpose(0, 2, 1) / np.sqrt(np.float32(d)).astype(H.dtype)
        e = np.exp(s - s.max(-1, keepdims=True))
        pr = e / e.sum(-1, keepdims=True)
        fw.Q.append(Q), fw.K.append(K), fw.V.append(V), fw.prob.append(pr)
        outs.append(pr @ V)
    fw.O = np.concatenate(outs, -1)
    fw.pred = fw.O.reshape(bs, -1) @ p["fc.weight"].T + p["fc.bias"]
    return fw


def backward(p, fw, dpred):
    bs, N, d = fw.H.shape
    nh = len(fw.Q)
    P = N - F
    X = fw.feat
    Xt = X.transpose(0, 2, 1)
    g = {}
    dpred = dpred.reshape(bs, 1)
    g["fc.weight"] = dpred.T @ fw.O.reshape(bs, -1)
    g["fc.bias"] = dpred.sum(0)
    dO = (dpred @ p["fc.weight"]).reshape(bs, N, nh * d)
    dH = np.zeros_like(fw.H)
    sc = 1.0 / np.sqrt(np.float32(d)).astype(fw.H.dtype)
    for i in range(nh):
        pre = f"self_attention.heads.{i}."
        dOi = dO[:, :, i * d:(i + 1) * d]
        pr = fw.prob[i]
        dV = pr.transpose(0, 2, 1) @ dOi
        dP = dOi @ fw.V[i].transpose(0, 2, 1)
        dS = pr * (dP - (dP * pr).sum(-1, keepdims=True)) * sc
        dQ = dS @ fw.K[i]
        dK = dS.transpose(0, 2, 1) @ fw.Q[i]
        for w, dd in (("W_q", dQ), ("W_k", dK), ("W_v", dV)):
            g[pre + w + ".weight"] = np.einsum("bno,bni->oi", dd, fw.H)
            g[pre + w + ".bias"] = dd.sum((0, 1))
            dH = dH + dd @ p[pre + w + ".weight"]
    dZ = dH * np.where(fw.H > 0, 1.0, SLOPE)
    dZs, dZt = dZ[:, :F], dZ[:, F:]
    # spatial: H_s = lrelu((A_s Xt) Ts^T + bs), A_s = U_s W2s^T + b2s, U_s = tanh(Xt W1s^T + b1s)
    g["spatial_gnn.theta.0.weight"] = np.einsum("bjo,bjp->op", dZs, fw.Ms)
    g["spatial_gnn.theta.0.bias"] = dZs.sum((0, 1))
    dMs = dZs @ p["spatial_gnn.theta.0.weight"]                                 # [bs, 40, P]
    dAs = dMs @ X                                                                 # dA = dM Xt^T   [bs, 40, 40]
    g["attention_spa_adj.2.weight"] = np.einsum("bij,bih->jh", dAs, fw.Us)
    g["attention_spa_adj.2.bias"] = dAs.sum((0, 1))
    dpre = (dAs @ p["attention_spa_adj.2.weight"]) * (1 - fw.Us ** 2)
    g["attention_spa_adj.0.weight"] = np.einsum("bjh,bjp->hp", dpre, Xt)
    g["attention_spa_adj.0.bias"] = dpre.sum((0, 1))
    # temporal
    g["temporal_gnn.theta.0.weight"] = np.einsum("bpo,bpf->of", dZt, fw.Mt)
    g["temporal_gnn.theta.0.bias"] = dZt.sum((0, 1))
    dMt = dZt @ p["temporal_gnn.theta.0.weight"]                                # [bs, P, 40]
    dAt = dMt @ Xt                                                                # [bs, P, P]
    g["attention_tem_adj.2.weight"] = np.einsum("bij,bih->jh", dAt, fw.Ut)
    g["attention_tem_adj.2.bias"] = dAt.sum((0, 1))
    dpre = (dAt @ p["attention_tem_adj.2.weight"]) * (1 - fw.Ut ** 2)
    g["attention_tem_adj.0.weight"] = np.einsum("bph,bpf->hf", dpre, X)
    g["attention_tem_adj.0.bias"] = dpre.sum((0, 1))
    assert P == X.shape[1]
    return g


def loss_and_grads(p, x, y, num_patch, patch_size, global_batch=None):
    fw = forward(p, x, num_patch, patch_size)
    B = x.shape[0] if global_batch is None else global_batch
    diff = fw.pred.reshape(-1) - y.reshape(-1)
    return float((diff * diff).sum() / B), backward(p, fw, (2.0 / B) * diff), fw


# ---- the same step as vectorised torch calls (timing yardstick) ---------------------------------------------------------------------
def torch_features(x, num_patch, patch_size):
    """The reference's extract_features restated with batched torch calls: x [bs, P * n] -> [bs, P, 40] (median bin: stable order)."""
    import torch
    bs = x.shape[0]
    s = x.reshape(bs * num_patch, patch_size)
    n = patch_size
    mean = s.mean(1)
    sm = torch.softmax(s, 1)
    ent = -(sm * torch.log(sm)).sum(1)
    sd, var = s.std(1), s.var(1)
    d = s - mean[:, None]
    clamp = s.clamp(-1 + 1e-7, 1 - 1e-7)
    t = torch.stack([s.max(1).values, s.min(1).values, sd, (s * s).mean(1).sqrt(), mean, s.max(1).values - s.min(1).values, var, ent,
                     torch.asin(clamp).std(1), torch.atan(s).std(1), (d ** 4).mean(1) / var ** 2 - 3, (d ** 3).mean(1) / sd ** 3], 1)
    Fq = torch.fft.fft(s, dim=1)
    freqs = torch.fft.fftfreq(n, d=1.0).to(s.device)
    amp = Fq.abs()
    psd = amp ** 2 / n
    tot = psd.sum(1)
    med = freqs[torch.argsort(psd, dim=1, stable=True)[:, n // 2]]
    f = torch.stack([(freqs * psd).sum(1) / tot, med, tot, psd[:, freqs < 0.5].sum(1) / tot, ((psd ** 2).sum(1) / tot).sqrt(), psd.max(1).values,
                     amp.max(1).values, freqs[amp.argmax(1)]], 1)
    f = torch.cat([t, f], 1).reshape(bs, num_patch, 20)
    cs = torch.cumsum(f, 1)
    f = torch.cat([f, cs / cs.abs().clamp_min(1e-12).sqrt()], 2)
    return f / (f * f).sum((1, 2), keepdim=True).sqrt()


def torch_forward(p, x, num_patch, patch_size, heads=1):
    import torch
    import torch.nn.functional as Fn
    X = torch_features(x, num_patch, patch_size)
    Xt = X.transpose(1, 2)
    As = Fn.linear(torch.tanh(Fn.linear(Xt, p["attention_spa_adj.0.weight"], p["attention_spa_adj.0.bias"])),
                   p["attention_spa_adj.2.weight"], p["attention_spa_adj.2.bias"])
    At = Fn.linear(torch.tanh(Fn.linear(X, p["attention_tem_adj.0.weight"], p["attention_tem_adj.0.bias"])),
                   p["attention_tem_adj.2.weight"], p["attention_tem_adj.2.bias"])
    Hs = Fn.leaky_relu(Fn.linear(torch.bmm(As, Xt), p["spatial_gnn.theta.0.weight"], p["spatial_gnn.theta.0.bias"]))
    Ht = Fn.leaky_relu(Fn.linear(torch.bmm(At, X), p["temporal_gnn.theta.0.weight"], p["temporal_gnn.theta.0.bias"]))
    H = torch.cat((Hs, Ht), 1)
    outs = []
    for i in range(heads):
        pre = f"self_attention.heads.{i}."
        Q = Fn.linear(H, p[pre + "W_q.weight"], p[pre + "W_q.bias"])
        K = Fn.linear(H, p[pre + "W_k.weight"], p[pre + "W_k.bias"])
        V = Fn.linear(H, p[pre + "W_v.weight"], p[pre + "W_v.bias"])
        s = torch.bmm(Q, K.transpose(-1, -2)) / float(np.sqrt(np.float32(H.shape[-1])))
        outs.append(torch.bmm(torch.softmax(s, -1), V))
    return Fn.linear(torch.cat(outs, -1).reshape(x.shape[0], -1), p["fc.weight"], p["fc.bias"])


def torch_step(p, optimizer, x, y, num_patch, patch_size, heads=1):
    """AGCN_TF.update (algorithms.py:589-597) on a dict of torch parameters `p` and a torch optimizer over them."""
    import torch.nn.functional as Fn
    loss = Fn.mse_loss(torch_forward(p, x, num_patch, patch_size, heads), y.reshape(-1, 1))
    optimizer.zero_grad()
    loss.backward()
    optimizer.step()
    return loss
