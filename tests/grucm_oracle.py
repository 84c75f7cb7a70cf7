"""Independent fp64 restatement of GRU_CM (reference models/GRU_CM/Model.py:6-82) in numpy, forward and backward, with the package's
counter-hash dropout -- the yardstick of tests/test_grucm_*.py -- and a small torch restatement of the same model (the CPU tests
cross-check the numpy code against it through autograd; tools/time_grucm.py times it as the ATen baseline).

    x [bs, N, L], h = N // 2
    x0 = Linear(1, h)(x[b, i, t]) . drop0                                   Model.py:61-65
    S_i = sum_j relu(W_e [x0_i ; x0_j] + b_e), all j (j = i included)       Model.py:22-32
    n_i = relu(W_n [x0_i ; S_i] + b_n) . drop1                              Model.py:35-38, 69
    pooled = max_i n_i (first index on ties)                                Model.py:72
    hs = GRU(h, H)(pooled), gates (r, z, n), h0 = 0;  . drop2               Model.py:74-75
    pred = Linear(H L, 1)(hs.reshape(bs, -1))                               Model.py:77-80
"""
import numpy as np

from oracle.stgcn_oracle import _lowbias32, dropout_layer_key, dropout_threshold

PARAM_NAMES = ["input_linear.weight", "input_linear.bias", "gnn.edge_mlp.0.weight", "gnn.edge_mlp.0.bias",
               "gnn.node_mlp.0.weight", "gnn.node_mlp.0.bias",
               "gru.weight_ih_l0", "gru.weight_hh_l0", "gru.bias_ih_l0", "gru.bias_hh_l0",
               "output_linear.weight", "output_linear.bias"]


def param_names():
    return list(PARAM_NAMES)


def flatten(p):
    return np.concatenate([np.asarray(p[k], np.float32).reshape(-1) for k in PARAM_NAMES])


def unflatten(flat, like):
    out, off = {}, 0
    for k in PARAM_NAMES:
        n = like[k].size
        out[k] = np.asarray(flat[off:off + n]).reshape(like[k].shape)
        off += n
    return out


# ---- dropout ---------------------------------------------------------------------------------------------------------------------
def keep_scale(shape_bl, inner, seed, step, site, p, sample_offset=0):
    """Keep-scale (0 or 1 / (1 - p)) of one dropout site.  ``shape_bl`` = (bs, L); ``inner`` = (N, h) for sites 0 / 1, (H,) for site 2.
    counter = (((b + sample_offset) L + t) [N + i]) C + c, mod 2^32; dropped when hash(counter ^ key) < threshold."""
    bs, L = shape_bl
    full = (bs, L) + tuple(inner)
    if p <= 0.0:
        return np.ones(full)
    per = int(np.prod(inner))
    b = np.arange(bs, dtype=np.uint64)[:, None, None] + np.uint64(sample_offset)
    t = np.arange(L, dtype=np.uint64)[None, :, None]
    e = np.arange(per, dtype=np.uint64)[None, None, :]
    ctr = (((b * np.uint64(L) + t) * np.uint64(per) + e) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    with np.errstate(over="ignore"):
        hsh = _lowbias32(ctr ^ np.uint32(dropout_layer_key(seed, step, site)))
    keep = hsh >= np.uint32(dropout_threshold(p))
    return (keep.astype(np.float64) / (1.0 - p)).reshape(full)


def masks(bs, N, L, H, seed, step, p=(0.0, 0.0, 0.0), sample_offset=0):
    h = N // 2
    return (keep_scale((bs, L), (N, h), seed, step, 0, p[0], sample_offset),
            keep_scale((bs, L), (N, h), seed, step, 1, p[1], sample_offset),
            keep_scale((bs, L), (H,), seed, step, 2, p[2], sample_offset))


def _sig(v):
    return 1.0 / (1.0 + np.exp(-v))


# ---- GRU (torch's gate arithmetic: r, z, n; n = tanh(gi_n + r (gh_n + b_hn))) --------------------------------------------------
def gru_forward(x, w_ih, w_hh, b_ih, b_hh):
    S, L, _ = x.shape
    H = w_hh.shape[1]
    out = np.zeros((S, L, H))
    tape = []
    hprev = np.zeros((S, H))
    for t in range(L):
        gi = x[:, t] @ w_ih.T + b_ih
        gh = hprev @ w_hh.T + b_hh
        r = _sig(gi[:, :H] + gh[:, :H])
        z = _sig(gi[:, H:2 * H] + gh[:, H:2 * H])
        n = np.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        hcur = (1.0 - z) * n + z * hprev
        tape.append((hprev, r, z, n, gh[:, 2 * H:]))
        out[:, t] = hcur
        hprev = hcur
    return out, tape


def gru_backward(x, w_ih, w_hh, tape, dout):
    S, L, I = x.shape
    H = w_hh.shape[1]
    dx = np.zeros_like(x)
    dw_ih, dw_hh = np.zeros_like(w_ih), np.zeros_like(w_hh)
    db_ih, db_hh = np.zeros(3 * H), np.zeros(3 * H)
    dh = np.zeros((S, H))
    for t in range(L - 1, -1, -1):
        hprev, r, z, n, ghn = tape[t]
        g = dout[:, t] + dh
        dn = g * (1.0 - z)
        dz = g * (hprev - n)
        dpn = dn * (1.0 - n * n)
        dpr = dpn * ghn * r * (1.0 - r)
        dpz = dz * z * (1.0 - z)
        dgi = np.concatenate([dpr, dpz, dpn], axis=1)
        dgh = np.concatenate([dpr, dpz, dpn * r], axis=1)
        dw_ih += dgi.T @ x[:, t]
        dw_hh += dgh.T @ hprev
        db_ih += dgi.sum(0)
        db_hh += dgh.sum(0)
        dx[:, t] = dgi @ w_ih
        dh = g * z + dgh @ w_hh
    return dx, dw_ih, dw_hh, db_ih, db_hh


# ---- the model -------------------------------------------------------------------------------------------------------------------
def forward_backward(x, y, p, keep=None, global_batch=None, dpred=None, want_grads=True):
    """Returns (loss, grads, pred [bs, 1], cache).  ``keep``: the three keep-scale tensors of ``masks`` (None: eval / p = 0).
    loss = sum (pred - y)^2 / global_batch (the shard's share of the global MSE); ``dpred`` overrides d loss / d pred."""
    x = np.asarray(x, np.float64)
    bs, N, L = x.shape
    h = N // 2
    P64 = {k: np.asarray(v, np.float64) for k, v in p.items()}
    w_in, b_in = P64["input_linear.weight"].reshape(h), P64["input_linear.bias"]
    We, be = P64["gnn.edge_mlp.0.weight"], P64["gnn.edge_mlp.0.bias"]
    Wn, bn = P64["gnn.node_mlp.0.weight"], P64["gnn.node_mlp.0.bias"]
    w_ih, w_hh, b_ih, b_hh = P64["gru.weight_ih_l0"], P64["gru.weight_hh_l0"], P64["gru.bias_ih_l0"], P64["gru.bias_hh_l0"]
    w_out, b_out = P64["output_linear.weight"].reshape(-1), P64["output_linear.bias"]
    H = w_hh.shape[1]
    m0, m1, m2 = keep if keep is not None else (np.ones((bs, L, N, h)), np.ones((bs, L, N, h)), np.ones((bs, L, H)))
    xt = x.transpose(0, 2, 1)                                           # [bs, L, N]
    lin = xt[..., None] * w_in + b_in
    x0 = lin * m0                                                       # [bs, L, N, h]
    Pm = x0 @ We[:, :h].T
    Qm = x0 @ We[:, h:].T + be
    pair = Pm[:, :, :, None, :] + Qm[:, :, None, :, :]                  # [bs, L, i, j, h]  (the oracle may form it; the kernels never do)
    S = np.maximum(pair, 0.0).sum(3)
    u = np.concatenate([x0, S], -1)
    pre = u @ Wn.T + bn
    nd = np.maximum(pre, 0.0) * m1
    arg = nd.argmax(2)                                                  # first index on ties, as torch.max
    pooled = np.take_along_axis(nd, arg[:, :, None, :], 2)[:, :, 0, :]  # [bs, L, h]
    hs, tape = gru_forward(pooled, w_ih, w_hh, b_ih, b_hh)
    hd = hs * m2
    flat = hd.reshape(bs, -1)
    pred = flat @ w_out + b_out                                         # [bs]
    cache = {"pooled": pooled, "hs": hs}
    gb = float(global_batch if global_batch is not None else bs)
    loss = None
    if y is not None:
        err = pred - np.asarray(y, np.float64).reshape(bs)
        loss = float((err * err).sum() / gb)
    if not want_grads:
        return loss, None, pred[:, None], cache
    dp = np.asarray(dpred, np.float64).reshape(bs) if dpred is not None else 2.0 * err / gb
    g = {}
    g["output_linear.weight"] = (dp @ flat).reshape(1, -1)
    g["output_linear.bias"] = np.array([dp.sum()])
    dhs = (dp[:, None] * w_out[None, :]).reshape(bs, L, H) * m2
    dpooled, g["gru.weight_ih_l0"], g["gru.weight_hh_l0"], g["gru.bias_ih_l0"], g["gru.bias_hh_l0"] = gru_backward(pooled, w_ih, w_hh, tape, dhs)
    dnd = np.zeros_like(nd)
    np.put_along_axis(dnd, arg[:, :, None, :], dpooled[:, :, None, :], 2)
    da = dnd * m1 * (pre > 0.0)
    g["gnn.node_mlp.0.weight"] = np.einsum("blnc,blnk->ck", da, u)
    g["gnn.node_mlp.0.bias"] = da.sum((0, 1, 2))
    du = da @ Wn
    dx0, dS = du[..., :h].copy(), du[..., h:]
    sign = pair > 0.0
    dP = dS * sign.sum(3)
    dQ = (dS[:, :, :, None, :] * sign).sum(2)
    g["gnn.edge_mlp.0.weight"] = np.concatenate([np.einsum("blnc,blnk->ck", dP, x0), np.einsum("blnc,blnk->ck", dQ, x0)], 1)
    g["gnn.edge_mlp.0.bias"] = dQ.sum((0, 1, 2))
    dx0 += dP @ We[:, :h] + dQ @ We[:, h:]
    dlin = dx0 * m0
    g["input_linear.weight"] = (dlin * xt[..., None]).sum((0, 1, 2)).reshape(h, 1)
    g["input_linear.bias"] = dlin.sum((0, 1, 2))
    return loss, g, pred[:, None], cache


def forward(x, p, keep=None):
    return forward_backward(x, None, p, keep, want_grads=False)[2]


def adam_step(p, grads, state, lr, wd, betas=(0.9, 0.999), eps=1e-8):
    """torch.optim.Adam (L2 weight decay folded into the gradient), in place on the fp64 parameters."""
    state["t"] = state.get("t", 0) + 1
    t = state["t"]
    for k in PARAM_NAMES:
        gk = np.asarray(grads[k], np.float64).reshape(p[k].shape) + wd * p[k]
        m = state.setdefault("m:" + k, np.zeros_like(p[k]))
        v = state.setdefault("v:" + k, np.zeros_like(p[k]))
        m *= betas[0]; m += (1 - betas[0]) * gk
        v *= betas[1]; v += (1 - betas[1]) * gk * gk
        p[k] = p[k] - lr / (1 - betas[0] ** t) * m / (np.sqrt(v / (1 - betas[1] ** t)) + eps)


# ---- torch restatement ------------------------------------------------------------------------------------------------------------
def torch_model(time_length, num_nodes, gru_hidden_dim, dtype=None):
    """The same function as a torch module (ATen ops + nn.GRU), its parameters under the 12 names of PARAM_NAMES.  ``keep`` (three
    tensors as of ``masks``) replaces the dropout; without it the module applies no dropout."""
    import torch
    import torch.nn as nn

    class _Gnn(nn.Module):
        def __init__(self, h):
            super().__init__()
            self.edge_mlp = nn.Sequential(nn.Linear(2 * h, h), nn.ReLU())
            self.node_mlp = nn.Sequential(nn.Linear(2 * h, h), nn.ReLU())

    class TorchGRUCM(nn.Module):
        def __init__(self):
            super().__init__()
            h = num_nodes // 2
            self.h = h
            self.input_linear = nn.Linear(1, h)
            self.gnn = _Gnn(h)
            self.gru = nn.GRU(h, gru_hidden_dim, batch_first=True)
            self.output_linear = nn.Linear(gru_hidden_dim * time_length, 1)

        def forward(self, x, keep=None):
            bs, h = x.size(0), self.h
            v = self.input_linear(x.transpose(1, 2).unsqueeze(-1))                # [bs, L, N, h]
            if keep is not None:
                v = v * keep[0]
            We = self.gnn.edge_mlp[0]
            pm = v @ We.weight[:, :h].T
            qm = v @ We.weight[:, h:].T + We.bias
            s = torch.relu(pm.unsqueeze(3) + qm.unsqueeze(2)).sum(3)
            nd = self.gnn.node_mlp(torch.cat([v, s], -1))
            if keep is not None:
                nd = nd * keep[1]
            pooled, _ = nd.max(2)
            hs, _ = self.gru(pooled)
            if keep is not None:
                hs = hs * keep[2]
            return self.output_linear(hs.reshape(bs, -1))

    m = TorchGRUCM()
    return m.to(dtype) if dtype is not None else m
