"""Every golden fixture that holds the reference's gradients (``grad:*``), with the fp64 oracle's gradients for the same parameters
and input: what tests/test_grad_gate_cpu.py, tests/test_grad_elementwise_gpu.py and tests/golden/make_grad_noise.py share.

``case(family, name)`` runs the family's oracle once per process (cached; the arrays are shared and must not be written to) and returns
the fp64 gradients ``g64`` and the reference's fp32 autograd ``ref32`` under the reference's parameter names, both in the fixture's
layout.  ``ref32[k] is None`` where the fixture records that the reference produced no gradient (``hasgrad:k`` false).
``maxnorm_failures`` restates each family's existing whole-tensor rule (the ``check_grads`` of its GPU test file) so that the CPU test
can show what that rule lets through.  Nothing here needs a GPU or the extension.

``Case.x`` is the batch: the fixture's ``x``, or, for the ``*_wrap_*`` fixtures of tests/golden/make_golden_wrap.py (batches of
thousands, ``Case.wrap``), the array rebuilt from the fixture's seed and checked against its checksum (tests/golden_io.py).
``Case.pred64`` / ``Case.loss64`` are the oracle's own prediction and loss of the step, ``Case.oracle_seconds`` what the oracle took."""
import functools
import glob
import os
import time

import numpy as np

import grad_gate as GG

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# family -> (fixture glob, rtol).  rtol is the family's existing gradient gate against the oracle, from its GPU test file:
# GTOL of test_train_gpu / test_mpnn_order_gpu / test_fcstgnn_gpu / test_astgcnn_gpu / test_stconv_gpu / test_rgcnu_gpu /
# test_stmsgcn_gpu / test_agcntf_gpu / test_stnet_gpu / test_hagcn_gpu, the literal 5e-4 of test_sagcn_gpu and test_stagnn_gpu,
# GTOL_ORACLE of test_grucm_gpu and the allclose rtol of test_stgnn_gpu (tests/test_grad_elementwise_gpu.py asserts the named ones)
FAMILIES = {
    "ST_GCN": ("stgcn_*_bs*.npz", 5e-4),
    "FC_STGNN": ("fcstgnn_*_bs*.npz", 5e-4),
    "ASTGCNN": ("astgcnn_*_bs*.npz", 5e-4),
    "HAGCN": ("hagcn_*_bs*.npz", 1e-3),
    "STMSGCN": ("stmsgcn_*_bs*.npz", 5e-4),
    "ST_Conv": ("stconv_*_bs*.npz", 5e-4),
    "RGCNU": ("rgcnu_*_bs*.npz", 5e-4),
    "STAGNN": ("stagnn_*_bs*.npz", 5e-4),
    "STGNN": ("stgnn_*_bs*.npz", 2e-3),
    "STNet": ("stnet_*_bs*.npz", 1e-3),
    "SAGCN": ("sagcn_*_bs*.npz", 5e-4),
    "AGCN_TF": ("agcntf_*_bs*.npz", 5e-4),
    "GRU_CM": ("grucm_*_bs*.npz", 2e-4),
}


def _holds_grads(path):
    with np.load(path) as z:
        return any(k.startswith("grad:") for k in z.files)


def fixtures(family):
    pat, _ = FAMILIES[family]
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, pat)) if _holds_grads(p))


def all_cases():
    return [(f, n) for f in FAMILIES for n in fixtures(f)]


def rtol_of(family):
    return FAMILIES[family][1]


class Case:
    def __init__(self, family, name, z, g64, extra=None):
        self.family, self.name, self.z, self.rtol = family, name, z, rtol_of(family)
        self.x = z["x"]                       # the stored array, or the one rebuilt from the fixture's seed (tests/golden/synth.py::Fixture)
        self.wrap = "x_seed" in z.files       # a batch that wraps every clamped grid (tests/golden/make_golden_wrap.py)
        self.ref32, self.g64 = {}, {}
        for k, v in g64.items():
            key = "grad_nodes" if k == "grad_nodes" else "grad:" + k
            has = key in z.files and ("hasgrad:" + k not in z.files or bool(z["hasgrad:" + k]))
            self.ref32[k] = z[key] if has else None
            v = np.array(v, np.float64)
            if key in z.files:
                assert v.size == z[key].size, (name, k, v.shape, z[key].shape)
                v = v.reshape(z[key].shape)
            self.g64[k] = v
        self.zero = GG.zero_in_exact_arithmetic(self.g64, self.ref32)
        self.live = [k for k in self.g64 if k not in self.zero]
        self.extra = extra or {}
        self.pred64 = np.asarray(self.extra["pred"], np.float64).reshape(-1) if "pred" in self.extra else None       # the oracle's own step
        self.loss64 = float(self.extra["loss"]) if "loss" in self.extra else None
        for v in list(self.g64.values()) + [v for v in self.ref32.values() if v is not None]:
            v.setflags(write=False)

    def floor(self, k):
        return GG.floor_for(self.ref32[k], self.g64[k])


def stgcn_dims(name, z):
    """(num_patch, patch_size, num_layers, mpnn order) of an ST_GCN fixture; the layer-count fixtures are 14 x 30 and say only L."""
    N = int(z["num_patch"]) if "num_patch" in z.files else 14
    P = int(z["patch_size"]) if "patch_size" in z.files else 30
    L = int(z["num_layers"]) if "num_layers" in z.files else 2
    K = int(z["k"]) if "k" in z.files else 1
    return N, P, L, K


def _stgcn(name):
    from oracle import stgcn_oracle as O
    from test_oracle_golden import load_case
    z, sd = load_case(name)
    N, P, L, K = stgcn_dims(name, z)
    fc = O.forward(sd, z["x"].astype(np.float64), N, P, L, train=True, dropout=0.0)
    loss, dpred = O.mse_loss_and_grad(fc.pred, z["y"].astype(np.float64))
    g = O.backward(sd, fc, dpred)
    return z, {k: g[k] for k in O.live_param_names(L, K)}, {"sd": sd, "dims": (N, P, L, K), "pred": fc.pred, "loss": loss}


def _fcstgnn(name):
    from oracle import fcstgnn_oracle as O
    from test_fcstgnn_oracle_golden import load_case
    z, cfg, p = load_case(name)
    loss, g, fw = O.loss_and_grads(p, z["x"].astype(np.float64), z["y"].astype(np.float64), cfg)
    return z, {k: g[k] for k in O.param_names(cfg)}, {"pred": fw.pred, "loss": loss, "cfg": cfg, "p": p}


def _astgcnn(name):
    from oracle import astgcnn_oracle as O
    from test_astgcnn_oracle_golden import load_case
    z, p = load_case(name)
    loss, g, fw = O.loss_and_grads(p, z["x"].astype(np.float64), z["y"].astype(np.float64))
    return z, {k: g[k] for k in O.live_param_names()}, {"pred": fw.pred, "loss": loss, "p": p}


def _stconv(name):
    from oracle import stconv_oracle as O
    from test_stconv_oracle_golden import load_case
    z, p = load_case(name)
    loss, g, fw = O.loss_and_grads(p, z["x"].astype(np.float64), z["y"].astype(np.float64))
    return z, {k: g[k] for k in O.live_param_names()}, {"pred": fw.pred, "loss": loss, "p": p}


def _stmsgcn(name):
    from oracle import stmsgcn_oracle as O
    from test_stmsgcn_oracle_golden import load_case
    z, cfg, p = load_case(name)
    loss, g, fw = O.loss_and_grads(p, z["x"].astype(np.float64), z["y"].astype(np.float64), cfg)
    return z, {k: g[k] for k in O.param_names(cfg)}, {"pred": fw.pred, "loss": loss, "cfg": cfg, "p": p}


def _rgcnu(name):
    from oracle import rgcnu_oracle as O
    from test_rgcnu_oracle_golden import load_case
    z, cfg, p = load_case(name)
    loss, g, fw = O.loss_and_grads(p, z["x"].astype(np.float64), z["y"].astype(np.float64), cfg["alpha"])
    return z, {k: g[k] for k in O.param_names()}, {"pred": fw.pred, "loss": loss, "cfg": cfg, "p": p}


def _stagnn(name):
    from oracle import stagnn_oracle as O
    from test_stagnn_oracle_golden import load_case
    z, cfg, p = load_case(name)
    loss, g, fw = O.loss_and_grads(p, z["x"].astype(np.float64), z["y"].astype(np.float64), cfg["num_heads"], cfg["threshold"])
    return z, {k: g[k] for k in O.live_param_names(cfg["num_heads"])}, {"pred": fw.pred, "loss": loss, "cfg": cfg, "p": p}


def _stgnn(name):
    from oracle import stgnn_oracle as O
    from test_stgnn_oracle_golden import load
    z, cfg, p = load(os.path.join(GOLDEN, name + ".npz"))
    loss, g, out, _ = O.forward_backward(z["x"].astype(np.float64), z["y"].astype(np.float64), p, cfg["num_patch"], cfg["patch_size"], cfg["top_k"])
    return z, {k: g[k] for k in O.param_names()}, {"pred": out, "loss": loss, "cfg": cfg, "p": p}


def _stnet(name):
    from oracle import stnet_oracle as O
    from test_stnet_oracle_golden import load_case
    z, cfg, p = load_case(name)
    loss, g, fw = O.loss_and_grads(p, z["x"].astype(np.float64), z["y"].astype(np.float64), cfg["num_patch"], cfg["patch_size"], cfg["nperseg"])
    return z, {k: g[k] for k in O.param_names(len(cfg["Cheb_layers"]))}, {"pred": fw.pred, "loss": loss, "cfg": cfg, "p": p}


def _sagcn(name):
    from oracle import sagcn_oracle as O
    from test_sagcn_oracle_golden import load_case
    z, cfg, p = load_case(name)
    loss, g, fw = O.loss_and_grads(p, z["x"].astype(np.float64), z["y"].astype(np.float64), cfg["num_patch"], cfg["patch_size"])
    return z, {k: g[k] for k in O.param_names()}, {"pred": fw.pred, "loss": loss, "cfg": cfg, "p": p}


def _agcntf(name):
    import agcntf_oracle as O
    from test_agcntf_oracle_golden import load_case
    z, cfg, p = load_case(name)
    loss, g, fw = O.loss_and_grads(p, z["x"].astype(np.float64), z["y"].astype(np.float64), cfg["num_patch"], cfg["patch_size"])
    return z, {k: g[k] for k in O.param_names(cfg.get("num_heads", 1))}, {"pred": fw.pred, "loss": loss, "cfg": cfg, "p": p}


def _grucm(name):
    import grucm_oracle as O
    from test_grucm_oracle_golden import load
    z, cfg, p = load(os.path.join(GOLDEN, name + ".npz"))
    loss, g, out, _ = O.forward_backward(z["x"].astype(np.float64), z["y"].astype(np.float64), p)
    return z, {k: g[k] for k in O.param_names()}, {"pred": out, "loss": loss, "cfg": cfg, "p": p}


def _hagcn(name):
    """The graph stack and the head from the reference's own node features under its own selection (as
    test_hagcn_oracle_golden.py::test_graph_stack_gradients_match_reference does), with the data gradient d loss / d nodes as one
    more tensor; where the fixture holds the LSTM stack's gradients too, those from the reference's own d loss / d nodes
    (test_lstm_stack_backward_matches_reference)."""
    from oracle import hagcn_oracle as O
    from test_hagcn_oracle_golden import load_case
    z, p = load_case(name)
    bs = z["x"].shape[0]
    fw = O.graph_forward(p, z["nodes"].astype(np.float64), forced_topk=[z[f"order{l}"] for l in (1, 2, 3)])
    feats = fw.feats.reshape(bs, -1)
    h_pre = feats @ p["fc.0.weight"].T + p["fc.0.bias"]
    h = np.maximum(h_pre, 0.0)
    pred = h @ p["fc.2.weight"].T + p["fc.2.bias"]
    dpred = 2.0 * (pred - z["y"].astype(np.float64)) / bs
    dh = (dpred @ p["fc.2.weight"]) * (h_pre > 0)
    dfeats = (dh @ p["fc.0.weight"]).reshape(fw.feats.shape)
    g, dx0 = O.graph_backward(p, fw, dfeats, float(z["alpha"]))
    g64 = {k: g[k] for k in O.graph_param_names()}
    g64.update({"fc.0.weight": dh.T @ feats, "fc.0.bias": dh.sum(0), "fc.2.weight": dpred.T @ h, "fc.2.bias": dpred.sum(0)})
    g64["grad_nodes"] = dx0
    td = sorted(k[5:] for k in z.files if k.startswith("grad:TD."))
    if td:
        gt = O.td_backward(p, z["x"].astype(np.float64), int(z["cfg:patch_size"]), int(z["cfg:num_patch"]), z["grad_nodes"].astype(np.float64))
        g64.update({k: gt[k] for k in td})
    return z, g64, {"p": p}


_ORACLES = {"ST_GCN": _stgcn, "FC_STGNN": _fcstgnn, "ASTGCNN": _astgcnn, "HAGCN": _hagcn, "STMSGCN": _stmsgcn, "ST_Conv": _stconv,
            "RGCNU": _rgcnu, "STAGNN": _stagnn, "STGNN": _stgnn, "STNet": _stnet, "SAGCN": _sagcn, "AGCN_TF": _agcntf, "GRU_CM": _grucm}


@functools.lru_cache(maxsize=None)
def case(family, name):
    t0 = time.perf_counter()
    z, g64, extra = _ORACLES[family](name)
    c = Case(family, name, z, g64, extra)
    c.oracle_seconds = time.perf_counter() - t0
    return c


# ---- each family's existing whole-tensor rule, restated -------------------------------------------------------------------------

def _rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


def maxnorm_failures(c, got, names=None):
    """The names among ``names`` (default: the live tensors) on which ``got`` fails the family's existing check against the fixture's
    fp32 gradients: max|got - ref| / max(max|ref|, share * largest gradient of the model) < tol, with
      ST_GCN, FC_STGNN, ASTGCNN, STMSGCN, ST_Conv, SAGCN, AGCN_TF  tol 5e-4, share 0        (rel / rel_err < GTOL)
      GRU_CM   tol 5e-4 (GTOL_REF, the one its fixtures are held to), share 0
      STNet    tol 1e-3, share 0
      RGCNU    tol 5e-4, share 1e-3                                   (test_rgcnu_gpu.check_grads)
      STAGNN   tol 5e-4, share 1e4 * 1e-7                             (test_stagnn_gpu.check_grads with grad_floor)
      HAGCN    tol 1e-3, share 1e-2 over the graph stack's tensors; 0 for fc.*, TD.* and the data gradient (test_hagcn_gpu)
      STGNN    np.allclose(rtol=2e-3, atol=1e-6 + 2e-4 max|ref|)      (test_stgnn_gpu)"""
    fam = c.family
    names = c.live if names is None else names
    tol = {"STNet": 1e-3, "HAGCN": 1e-3}.get(fam, 5e-4)
    share = {"RGCNU": 1e-3, "STAGNN": 1e-3, "HAGCN": 1e-2}.get(fam, 0.0)
    pool = [k for k in c.g64 if c.ref32[k] is not None]
    if fam == "HAGCN":
        pool = [k for k in pool if k.startswith(("gin", "gnn"))]
    gmax = max(np.abs(c.ref32[k]).max() for k in pool)
    bad = []
    for k in names:
        r = np.asarray(c.ref32[k], np.float64)
        if fam == "STGNN":
            ok = np.allclose(got[k], r, rtol=2e-3, atol=1e-6 + 2e-4 * np.abs(r).max())
        else:
            s = share if (fam != "HAGCN" or k in pool) else 0.0
            ok = np.abs(got[k] - r).max() / max(np.abs(r).max(), s * gmax, 1e-30) < tol
        if not ok:
            bad.append(k)
    return bad


# ---- the comparison the GPU test makes, on anything that stands in for the kernels' gradients ---------------------------------------

def _where(mask):
    """Where the elements over the gate sit: their count, and the rows / columns / flat range they span."""
    idx = np.argwhere(mask)
    if mask.ndim < 2:
        return f"{len(idx)} of {mask.size} over, flat {idx.min()}..{idx.max()}"
    m2 = mask.reshape(mask.shape[0], -1)
    r, q = np.nonzero(m2)
    return f"{len(idx)} of {mask.size} over, rows {sorted(set(r.tolist()))[:12]} cols {sorted(set(q.tolist()))[:12]} of {m2.shape}"


def check(c, got, tag, margins=None):
    """Every live tensor of ``got`` (name -> array of the tensor's size in the fixture's element order; ``name@variant`` for a second
    set from another path) under the gate.  Returns (one line per tensor, one message per tensor over the gate).  Raises if ``got``
    does not hold exactly the model's tensors or a size differs."""
    margins = margins or {}
    names = sorted({gk.split("@")[0] for gk in got})
    assert names == sorted(c.g64), (tag, sorted(set(names) ^ set(c.g64)))
    lines, bad = [], []
    for gk in got:
        k = gk.split("@")[0]
        if k in c.zero:
            continue
        g64, ref32 = c.g64[k], c.ref32[k]
        a = np.asarray(got[gk], np.float64)
        assert a.size == g64.size, (tag, gk, a.shape, g64.shape)
        a = a.reshape(g64.shape)
        margin = margins.get((c.family, k), (GG.MARGIN,))[0]
        floor = GG.floor_for(ref32, g64, margin)
        r, at = GG.gate(a, g64, c.rtol, floor)
        gmax = np.abs(g64).max()
        lines.append(f"{tag} {gk}: ratio {r:.3f} at {at}  max-norm {np.abs(a - g64).max() / gmax:.2e}  floor/max {floor / gmax:.1e}")
        if not r <= 1.0:
            bad.append(f"{tag} {gk} at {at}: got {a[at]!r} g64 {g64[at]!r} ref32 {ref32[at]!r} ratio {r:.3f} (margin {margin}); "
                       + _where(GG.over_gate(a, g64, c.rtol, floor)))
    return lines, bad
