"""-m gpu: the H_l record of the matrix-core training chain (csrc/stgcn_train_mx.hip, MxTrainK::hrec).  F_{2l} (l >= 1)
saves H_l = leaky(theta(A X_l)) of every tile; F_{2l+1}, G_{2l+1} and TOP read it instead of rebuilding it from X_l and the adjacency.
The record lives in a workspace slot that no other part of the step writes, and the last tile of a batch with B % 4 != 0 leaves whatever
an earlier step put there beyond the batch: a step on a workspace filled with NaN must give the same bits as a step on a zeroed one.
(Batches of at most 256 samples: at most 16 workgroups, one per cell replica, so the fp64 cell sums do not depend on atomic order.)"""
import ctypes as C

import numpy as np
import pytest
import torch

from gnn_rul_benchmarking_amd import _lib, params as PL
from oracle import stgcn_oracle as O
from test_train_gpu import oracle_step, check_grads, TOL

pytestmark = pytest.mark.gpu


def ws_step(x_np, y_np, flat_np, N, P, L, path, ws_fill, dropout=0.0, seed=0, step=1):
    """rulgnn_stgcn_train_step_path_f32 on cuda:0 with a workspace whose floats all hold `ws_fill` before the step."""
    import gpu_util as G
    lib = _lib.load()
    dev = torch.device("cuda:0")
    B = x_np.shape[0]
    x = torch.from_numpy(np.ascontiguousarray(x_np.reshape(B, -1), np.float32)).to(dev)
    y = torch.from_numpy(np.ascontiguousarray(y_np.reshape(B), np.float32)).to(dev)
    prm = torch.from_numpy(flat_np.copy()).to(dev)
    grads = torch.full_like(prm, float("nan"))
    pred = torch.full((B,), float("nan"), device=dev)
    loss = torch.full((1,), float("nan"), device=dev)
    bnb = torch.full((L * 2 * 2 * 10,), float("nan"), device=dev)
    shp = G.shape_struct(B, N, P, L)
    nbytes = lib.rulgnn_stgcn_train_workspace_bytes(C.byref(shp))
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=dev).fill_(ws_fill)
    a = _lib.StgcnTrainArgs()
    a.x = x.data_ptr(); a.y = y.data_ptr(); a.dpred = None
    a.params = prm.data_ptr(); a.grads = grads.data_ptr(); a.pred = pred.data_ptr(); a.loss = loss.data_ptr()
    a.bn_batch = bnb.data_ptr(); a.workspace = ws.data_ptr(); a.workspace_bytes = nbytes
    a.global_batch = B; a.sample_offset = 0
    a.dropout_p = dropout; a.seed = seed; a.step = step
    rc = lib.rulgnn_stgcn_train_step_path_f32(C.byref(shp), C.byref(a), None, path, G.stream_ptr())
    torch.cuda.synchronize()
    return rc, {"pred": pred.cpu().numpy(), "loss": loss.cpu().numpy(), "grads": grads.cpu().numpy(), "bn_batch": bnb.cpu().numpy()}


def _inputs(N, P, L, B):
    rng = np.random.default_rng(B * 10 + L)
    prm = O.random_params(N, L, seed=B)
    x = rng.uniform(0, 1, (B, N, P)).astype(np.float32)
    y = rng.uniform(0, 1, (B,)).astype(np.float32)
    flat, _ = PL.pack_numpy(prm, N, L)
    return prm, x, y, flat


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


_MX, _PERSIST = "mx", "mx_persist"


@pytest.mark.parametrize("N,P,B,L,p,path", [(14, 30, 251, 2, 0.2, _MX), (14, 30, 38, 2, 0.0, _MX), (14, 30, 77, 1, 0.2, _MX),
                                            (14, 30, 41, 3, 0.2, _MX), (12, 21, 35, 2, 0.3, _MX), (14, 30, 251, 2, 0.2, _PERSIST),
                                            (14, 30, 38, 2, 0.0, _PERSIST), (12, 21, 35, 2, 0.3, _PERSIST)])
def test_stale_h_records_do_not_reach_the_step(N, P, B, L, p, path):
    step_path = _lib.STEP_MX if path == _MX else _lib.STEP_MX_PERSIST
    prm, x, y, flat = _inputs(N, P, L, B)
    rc0, zero = ws_step(x, y, flat, N, P, L, step_path, 0.0, dropout=p, seed=5, step=2)
    rc1, nan = ws_step(x, y, flat, N, P, L, step_path, float("nan"), dropout=p, seed=5, step=2)
    assert rc0 == 0 and rc1 == 0, (rc0, rc1)
    for k in ("pred", "loss", "grads", "bn_batch"):
        assert np.all(np.isfinite(zero[k])), k
        assert np.array_equal(_bits(zero[k]), _bits(nan[k])), k
    # and still the reference step
    import gpu_util as G
    pred, loss, gref, bnb = oracle_step(prm, x, y, N, P, L, p, 5, 2)
    assert G.rel_err(nan["pred"], pred) < TOL
    assert abs(float(nan["loss"][0]) - loss) < TOL * abs(loss)
    assert G.rel_err(nan["bn_batch"], bnb) < TOL
    check_grads(nan["grads"], gref, N, L)


@pytest.mark.parametrize("B", [100, 101])
def test_single_launch_and_phase_launches_agree_on_a_stale_workspace(B):
    """F_1 .. G_0 as one launch (H_1 stored by F_2, read back by F_3 and G_3 of the same wavefront inside the launch) against the ten
    launches, both on NaN-filled workspaces, at the tolerances of the single-launch tests in test_train_mx_gpu.py."""
    import gpu_util as G
    N, P, L = 14, 30, 2
    prm, x, y, flat = _inputs(N, P, L, B)
    rc0, one = ws_step(x, y, flat, N, P, L, _lib.STEP_MX_PERSIST, float("nan"), dropout=0.2, seed=3, step=4)
    rc1, ten = ws_step(x, y, flat, N, P, L, _lib.STEP_MX, float("nan"), dropout=0.2, seed=3, step=4)
    assert rc0 == 0 and rc1 == 0, (rc0, rc1)
    lo, lt = float(one["loss"][0]), float(ten["loss"][0])
    assert np.isfinite(lo) and abs(lo - lt) <= 1e-6 * abs(lt)
    assert G.rel_err(one["pred"], ten["pred"]) < 1e-6 and G.rel_err(one["bn_batch"], ten["bn_batch"]) < 1e-6
    check_grads(one["grads"], ten["grads"], N, L, 1e-5)
