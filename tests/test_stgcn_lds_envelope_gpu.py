"""-m gpu: ST_GCN at the edges of the fused row-mapped kernels' LDS budget (160 KB per workgroup).

The C-ABI promises one thing about shapes: a shape the host-side queries accept runs, and a shape they refuse gets
RULGNN_EUNSUPPORTED before anything is launched.  Each shape below is the last window length that one launch form of the fused
kernels holds, or the first one it does not hold (exact eval kernel, wide matrix-core eval + its scanning launch, fp32 phase chain,
the order-k theta phases).  Every call at every shape must be exactly one of

* accepted: the query says so, the call returns 0 and matches the fp64 oracle at the suite's gates (1e-4 on predictions, loss and
  batch statistics, 5e-4 on gradients);
* refused: the call returns -2 and nothing ran -- predictions, loss, gradients, batch statistics, workspace, parameters and
  optimizer state are bit for bit what they were.

"The query accepts the shape and the call fails" is the bug this file is about."""
import ctypes as C

import numpy as np
import pytest
import torch

from gnn_rul_benchmarking_amd import _lib, params as PL
from oracle import stgcn_oracle as O
from test_train_gpu import TOL, GTOL

pytestmark = pytest.mark.gpu

PATTERN = 0xA5           # the workspace's byte pattern: a kernel that ran (the step's prepare launch first of all) leaves it changed

# (num_patch, patch_size, num_layers, mpnn_k, batch): pairs of (last window that fits, first that does not) for one launch form each
SHAPES = [
    # eval, exact row-mapped kernel, order 1
    (33, 207, 2, 1, 5), (33, 208, 2, 1, 3),
    (40, 171, 2, 1, 7), (40, 172, 2, 1, 4),
    (47, 146, 2, 1, 6), (47, 147, 2, 1, 5),
    (48, 143, 2, 1, 3), (48, 144, 2, 1, 4),
    (64, 107, 2, 1, 3), (64, 108, 2, 1, 5),
    # eval at eight layers: row width 32 (batch 9: not a multiple of the two samples per wavefront); row width 16, where the staging
    # limit comes first (the last window it holds)
    (17, 219, 8, 1, 9), (17, 220, 8, 1, 5), (32, 115, 8, 1, 3), (32, 116, 8, 1, 4), (16, 143, 8, 1, 17),
    # training, fp32 phase chain, order 1: at 41 x 131 / 133 num_patch x patch_size is no multiple of 4 (no matrix-core chain);
    # 41 x 132 and 40 x 136 qualify for the wide matrix-core chain, whose guard retry lands on the fp32 chain
    (41, 131, 2, 1, 11), (41, 133, 2, 1, 3), (41, 132, 2, 1, 5), (40, 135, 2, 1, 3), (40, 136, 2, 1, 6),
    (48, 111, 2, 1, 7), (48, 112, 2, 1, 4),
    (64, 83, 2, 1, 9), (64, 84, 2, 1, 3),
    # order 2: eval, then training
    (17, 255, 2, 2, 5), (17, 256, 2, 2, 3),
    (40, 115, 2, 2, 4), (40, 116, 2, 2, 3), (40, 135, 2, 2, 5), (40, 136, 2, 2, 3),
    (64, 71, 2, 2, 3), (64, 72, 2, 2, 4), (64, 83, 2, 2, 3), (64, 84, 2, 2, 5),
    # order 3: training, eval, training at one layer
    (17, 198, 2, 3, 4), (17, 199, 2, 3, 3), (17, 239, 2, 3, 3), (17, 240, 2, 3, 5), (17, 203, 1, 3, 7), (17, 204, 1, 3, 3),
    (40, 63, 2, 3, 5), (40, 64, 2, 3, 3), (40, 83, 2, 3, 4), (40, 84, 2, 3, 3),
    (64, 39, 2, 3, 3), (64, 40, 2, 3, 6), (64, 51, 2, 3, 3), (64, 52, 2, 3, 4),
]
# shapes the wide matrix-core eval kernel (16 <= num_patch <= 47) qualifies for beyond the exact kernel's limit; its scanning launch
# recomputes non-finite predictions with the exact routine, so a constant patch (0/0 statistics) gives it work
WIDE_MX_EVAL = [(40, 200, 2, 1, 37), (47, 190, 2, 1, 13)]


def _sid(s):
    return "N%d_P%d_L%d_k%d_B%d" % s


def _inputs(N, P, L, K, B):
    rng = np.random.default_rng(N * 100003 + P * 101 + L * 7 + K)
    prm = O.random_params(N, L, seed=P + K, k=K)
    flat, bn = PL.pack_numpy(prm, N, L, k=K)
    x = rng.uniform(0, 1, (B, N, P)).astype(np.float32)
    y = rng.uniform(0, 1, (B,)).astype(np.float32)
    return prm, flat, bn, x, y


def eval_accepted(shp):
    """The eval gate as a host-only call: null pointers are EINVAL on a shape the kernels take, EUNSUPPORTED on one they refuse."""
    rc = _lib.load().rulgnn_stgcn_forward_f32(C.byref(shp), None, None, None, None, None, 0, None)
    assert rc in (_lib.EINVAL, _lib.EUNSUPPORTED), rc
    return rc == _lib.EINVAL


def run_eval(x_np, flat, bn_np, N, P, L, K, path):
    import gpu_util as G
    lib = _lib.load()
    dev = torch.device("cuda:0")
    B = x_np.shape[0]
    shp = G.shape_struct(B, N, P, L, K)
    nbytes = lib.rulgnn_stgcn_forward_workspace_bytes(C.byref(shp))
    x = torch.from_numpy(np.ascontiguousarray(x_np.reshape(B, -1))).to(dev)
    prm = torch.from_numpy(flat.copy()).to(dev)
    bn = torch.from_numpy(bn_np.copy()).to(dev)
    out = torch.full((B,), float("nan"), device=dev)
    ws = torch.full((max(nbytes, 1 << 16),), PATTERN, dtype=torch.uint8, device=dev)
    rc = lib.rulgnn_stgcn_forward_path_f32(C.byref(shp), x.data_ptr(), prm.data_ptr(), bn.data_ptr(), out.data_ptr(), ws.data_ptr(),
                                           ws.numel(), path, G.stream_ptr())
    torch.cuda.synchronize()
    untouched = bool((ws == PATTERN).all()) and np.array_equal(prm.cpu().numpy(), flat) and np.array_equal(bn.cpu().numpy(), bn_np)
    return rc, out.cpu().numpy(), untouched


def _check_eval(shape, const_patch=False):
    import gpu_util as G
    N, P, L, K, B = shape
    prm, flat, bn, x, _ = _inputs(N, P, L, K, B)
    if const_patch:
        x[1, N // 2, :] = 0.5
    accepted = eval_accepted(G.shape_struct(B, N, P, L, K))
    with np.errstate(all="ignore"):
        ref = O.forward(prm, x.astype(np.float64), N, P, L, train=False).pred[:, 0]
    nan = np.isnan(ref)
    assert nan.sum() == (1 if const_patch else 0)
    ok = ~nan
    for path in (_lib.EVAL_AUTO, _lib.EVAL_EXACT, _lib.EVAL_MX):
        rc, pred, untouched = run_eval(x, flat, bn, N, P, L, K, path)
        refused = rc == _lib.EUNSUPPORTED and np.isnan(pred).all() and untouched
        if not accepted:
            assert refused, (path, rc)
            continue
        # EVAL_MX names kernels with shape rules of their own: it may decline a shape the gate accepts, but only before any launch
        if path == _lib.EVAL_MX and rc == _lib.EUNSUPPORTED:
            assert refused, "EVAL_MX declined after writing predictions"
            continue
        assert rc == 0, (path, rc)
        assert np.array_equal(np.isnan(pred), nan), path
        assert G.rel_err(pred[ok], ref[ok]) < TOL, path
        assert G.elem_gate(pred[ok], ref[ok]) <= 1, path


@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_eval_at_the_lds_edge_runs_or_is_refused_up_front(shape):
    _check_eval(shape)


@pytest.mark.parametrize("shape", WIDE_MX_EVAL, ids=_sid)
def test_wide_mx_eval_shapes_put_the_nan_where_the_oracle_does(shape):
    _check_eval(shape, const_patch=True)


# (entry, path, fused Adam): the forms a training step reaches the kernels in
TRAIN_FORMS = [("fwdbwd", None, False), ("step", _lib.STEP_AUTO, False), ("step", _lib.STEP_CHAIN, False), ("step", _lib.STEP_AUTO, True)]
LR = 1e-3


def run_train(x_np, y_np, flat, N, P, L, K, entry, path, adam, dropout, seed, step):
    import gpu_util as G
    lib = _lib.load()
    dev = torch.device("cuda:0")
    B = x_np.shape[0]
    shp = G.shape_struct(B, N, P, L, K)
    nbytes = lib.rulgnn_stgcn_train_workspace_bytes(C.byref(shp))
    x = torch.from_numpy(np.ascontiguousarray(x_np.reshape(B, -1))).to(dev)
    y = torch.from_numpy(y_np.copy()).to(dev)
    prm = torch.from_numpy(flat.copy()).to(dev)
    grads = torch.full_like(prm, float("nan"))
    pred = torch.full((B,), float("nan"), device=dev)
    loss = torch.full((1,), float("nan"), device=dev)
    bnb = torch.full((L * 2 * 2 * 10,), float("nan"), device=dev)
    ws = torch.full((nbytes if nbytes else 1 << 20,), PATTERN, dtype=torch.uint8, device=dev)
    a = _lib.StgcnTrainArgs()
    a.x = x.data_ptr(); a.y = y.data_ptr(); a.dpred = None
    a.params = prm.data_ptr(); a.grads = grads.data_ptr(); a.pred = pred.data_ptr(); a.loss = loss.data_ptr()
    a.bn_batch = bnb.data_ptr(); a.workspace = ws.data_ptr(); a.workspace_bytes = ws.numel()
    a.global_batch = B; a.sample_offset = 0
    a.dropout_p = dropout; a.seed = seed; a.step = step
    opt, m, v, run = None, None, None, None
    if adam:
        m, v = torch.zeros_like(prm), torch.zeros_like(prm)
        run = torch.ones(L * 2 * 2 * 10, device=dev)
        opt = C.byref(_lib.AdamArgs(prm.data_ptr(), m.data_ptr(), v.data_ptr(), run.data_ptr(), 1, LR, 0.9, 0.999, 1e-8, 0.0, 0.1, None))
    if entry == "fwdbwd":
        rc = lib.rulgnn_stgcn_train_fwdbwd_f32(C.byref(shp), C.byref(a), G.stream_ptr())
    else:
        rc = lib.rulgnn_stgcn_train_step_path_f32(C.byref(shp), C.byref(a), opt, path, G.stream_ptr())
    torch.cuda.synchronize()
    r = {"pred": pred.cpu().numpy(), "loss": float(loss.item()), "grads": grads.cpu().numpy(), "bn_batch": bnb.cpu().numpy(),
         "params": prm.cpu().numpy(), "ws_untouched": bool((ws == PATTERN).all())}
    r["untouched"] = (r["ws_untouched"] and np.isnan(r["pred"]).all() and np.isnan(r["loss"]) and np.isnan(r["grads"]).all()
                      and np.isnan(r["bn_batch"]).all() and np.array_equal(r["params"], flat)
                      and (not adam or (not bool(m.any()) and not bool(v.any()) and bool((run == 1).all()))))
    return rc, r


def oracle_step(prm, x, y, N, P, L, K, dropout, seed, step):
    keys = [O.dropout_layer_key(seed, step, l) for l in range(L)]
    fc = O.forward(prm, x.astype(np.float64), N, P, L, train=True, dropout=dropout, dropout_keys=keys)
    loss, dp = O.mse_loss_and_grad(fc.pred, y.astype(np.float64))
    g = O.backward(prm, fc, dp, dropout)
    flat = np.zeros(PL.param_count(N, L, K))
    for name, (off, shape) in PL.live_param_layout(N, L, K).items():
        flat[off:off + int(np.prod(shape))] = g[name].reshape(-1)
    bnb = np.zeros(L * 2 * 2 * 10)
    for l in range(L):
        for b in range(2):
            bnb[((l * 2 + b) * 2) * 10:((l * 2 + b) * 2) * 10 + 10] = fc.layers[l].bn_mean[b]
            bnb[((l * 2 + b) * 2 + 1) * 10:((l * 2 + b) * 2 + 1) * 10 + 10] = fc.layers[l].bn_var[b]
    return fc.pred[:, 0], loss, flat, bnb


def check_grads(got, ref, N, L, K):
    import gpu_util as G
    for name, (off, shape) in PL.live_param_layout(N, L, K).items():
        n = int(np.prod(shape))
        e = G.rel_err(got[off:off + n], ref[off:off + n])
        assert e < GTOL, (name, e)


@pytest.mark.parametrize("shape", SHAPES + WIDE_MX_EVAL, ids=_sid)
def test_training_at_the_lds_edge_runs_or_is_refused_up_front(shape):
    import gpu_util as G
    N, P, L, K, B = shape
    prm, flat, _, x, y = _inputs(N, P, L, K, B)
    dropout, seed, step = 0.1, 3, 2
    accepted = _lib.load().rulgnn_stgcn_train_workspace_bytes(C.byref(G.shape_struct(B, N, P, L, K))) > 0
    rpred, rloss, rgrads, rbnb = oracle_step(prm, x, y, N, P, L, K, dropout, seed, step)
    for entry, path, adam in TRAIN_FORMS:
        form = (entry, path, adam)
        rc, r = run_train(x, y, flat, N, P, L, K, entry, path, adam, dropout, seed, step)
        if not accepted:
            assert rc == _lib.EUNSUPPORTED and r["untouched"], (form, rc)
            continue
        assert rc == 0, (form, rc)
        assert G.rel_err(r["pred"], rpred) < TOL, form
        assert abs(r["loss"] - rloss) < TOL * abs(rloss), form
        assert G.rel_err(r["bn_batch"], rbnb) < TOL, form
        if adam:
            # the fused optimizer's gradients are not written back; Adam's first step moves every parameter by lr * sign(g): identical
            # to the oracle's step unless a gradient is ~0
            want = flat.astype(np.float64) - LR * rgrads / (np.abs(rgrads) + 1e-8)
            assert np.mean(np.abs(r["params"] - want) < 1e-6) > 0.99, form
        else:
            check_grads(r["grads"], rgrads, N, L, K)


# ---- the module surface ------------------------------------------------------------------------------------------------------

def _state(model):
    return {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}


@pytest.mark.parametrize("N,P", [(64, 100), (40, 150)])
def test_module_trains_then_evaluates_at_the_edge(N, P):
    """Two ``update()`` calls and an ``eval()`` forward of the Algorithm wrapper, each against the oracle."""
    import gpu_util as G
    from gnn_rul_benchmarking_amd.algorithms import ST_GCN
    dev = torch.device("cuda:0")
    torch.manual_seed(2)
    algo = ST_GCN({"num_patch": N, "patch_size": P, "dropout": 0.2}, {"learning_rate": 1e-3, "weight_decay": 1e-4}, dev)
    algo.to(dev)
    g = torch.Generator(device=dev).manual_seed(9)
    x = torch.rand(13, N, P, device=dev, generator=g)
    y = torch.rand(13, 1, device=dev, generator=g)
    x64, y64 = x.cpu().numpy().astype(np.float64), y.cpu().numpy().astype(np.float64)
    algo.train()
    for _ in range(2):
        sd = _state(algo.model)
        seed, step = algo.model._seed, algo.model._step + 1
        loss = algo.update(x, y, 1)["loss"]
        keys = [O.dropout_layer_key(seed, step, l) for l in range(2)]
        fc = O.forward(sd, x64, N, P, train=True, dropout=0.2, dropout_keys=keys)
        ref_loss, dpred = O.mse_loss_and_grad(fc.pred, y64)
        assert abs(loss - ref_loss) < TOL * abs(ref_loss), (loss, ref_loss)
        ref = O.backward(sd, fc, dpred, 0.2)
        got = algo.model.bucket[:algo.model.num_live].cpu().numpy()
        for name, (off, shape) in PL.live_param_layout(N, 2).items():
            n = int(np.prod(shape))
            assert G.rel_err(got[off:off + n], ref[name].reshape(-1)) < GTOL, name
    algo.eval()
    with torch.no_grad():
        pred = algo.model(x).cpu().numpy()[:, 0]
    ref = O.forward(_state(algo.model), x64, N, P, train=False).pred[:, 0]
    assert G.rel_err(pred, ref) < TOL
    assert G.elem_gate(pred, ref) <= 1


def test_guard_retry_at_a_wide_shape_never_fails_partway():
    """40 x 136 qualifies for the wide matrix-core chain, whose f16 range guard rejects inputs far from O(1); ``update()`` then repeats
    the step after ``retry_on_fp32_chain()``.  Whatever path that lands on must take the step -- same result as a model that ran the
    fp32-chain request from the start."""
    from gnn_rul_benchmarking_amd.algorithms import ST_GCN
    dev = torch.device("cuda:0")
    N, P = 40, 136
    cfg = dict(num_patch=N, patch_size=P, dropout=0.2)
    hp = {"learning_rate": 1e-3, "weight_decay": 1e-4}
    g = torch.Generator(device=dev).manual_seed(5)
    X = torch.rand(24, N, P, device=dev, generator=g) * 3.0e4
    y = torch.rand(24, 1, device=dev, generator=g)
    torch.manual_seed(11)
    a = ST_GCN(cfg, hp, dev); a.to(dev); a.train()
    torch.manual_seed(11)
    b = ST_GCN(cfg, hp, dev); b.to(dev); b.train()
    b.model.step_path = _lib.STEP_CHAIN
    la = [a.update(X, y, 1)["loss"] for _ in range(2)]
    lb = [b.update(X, y, 1)["loss"] for _ in range(2)]
    assert all(np.isfinite(la)) and la == lb
    assert a.model._step == b.model._step == 2 and a.optimizer._steps == 2
    assert torch.equal(a.model.flat_params, b.model.flat_params)
    # and the explicit call, after a step that was taken: the next step still runs
    a.model.retry_on_fp32_chain(a.optimizer)
    assert np.isfinite(a.update(X, y, 1)["loss"])


def test_order3_model_past_the_limit_is_refused_before_any_launch():
    from gnn_rul_benchmarking_amd.stgcn import ST_GCN_model
    dev = torch.device("cuda:0")
    torch.manual_seed(1)
    m = ST_GCN_model(40, 84, num_layers=2, dropout=0.2, k=3).to(dev).train()
    before = m.flat_params.detach().clone()
    x = torch.rand(3, 40, 84, device=dev)
    with pytest.raises(RuntimeError, match="training kernels do not cover"):
        m(x)
    torch.cuda.synchronize()
    assert torch.equal(m.flat_params, before)
