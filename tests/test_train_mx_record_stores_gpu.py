"""-m gpu: the record stores of the matrix-core training chain (csrc/stgcn_train_mx.hip).  Every full-tile record (X_l, Q_l, H_l,
d(x0 + H), d X_l) leaves a phase through the wavefront's staging tile as whole 16-byte pieces: the last tile of a batch with
B % 4 != 0 writes all four samples, and every reader overwrites the samples beyond the batch of what it loads.  So neither what an
earlier step left in the workspace nor what this step's staged stores put beyond the batch may reach a result: a step on a workspace
filled with NaN gives the bits of a step on a zeroed one, and a step at a smaller batch on a workspace a larger batch has used gives the
bits of that step on a fresh workspace.
(Batches of at most 256 samples: at most 16 workgroups, one per cell replica, so the fp64 cell sums do not depend on atomic order.  The
single launch exists for two layers only: its cases are the L = 2 ones.)"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from gnn_rul_benchmarking_amd import _lib
from test_train_gpu import oracle_step, check_grads, TOL
from test_train_mx_hrec_gpu import ws_step, _inputs, _bits

pytestmark = pytest.mark.gpu

_MX, _PERSIST = "mx", "mx_persist"
_KEYS = ("pred", "loss", "grads", "bn_batch")


def _path(name):
    return _lib.STEP_MX if name == _MX else _lib.STEP_MX_PERSIST


@functools.lru_cache(maxsize=None)
def _case(N, P, L, B, p):
    """The H-record test's inputs and the fp64 oracle's step, computed once per case and shared by the two paths."""
    prm, x, y, flat = _inputs(N, P, L, B)
    return x, y, flat, oracle_step(prm, x, y, N, P, L, p, 5, 2)


def _step_on(ws, x_np, y_np, flat_np, N, P, L, path, dropout, seed, step):
    """ws_step of the H-record test on a workspace the CALLER keeps (ws_step allocates a fresh one per call): the same step, the same
    outputs, for the one test here whose point is a workspace that an earlier step has used."""
    import gpu_util as G
    lib = _lib.load()
    dev = ws.device
    B = x_np.shape[0]
    x = torch.from_numpy(np.ascontiguousarray(x_np.reshape(B, -1), np.float32)).to(dev)
    y = torch.from_numpy(np.ascontiguousarray(y_np.reshape(B), np.float32)).to(dev)
    prm = torch.from_numpy(flat_np.copy()).to(dev)
    out = {"pred": torch.full((B,), float("nan"), device=dev), "loss": torch.full((1,), float("nan"), device=dev),
           "grads": torch.full_like(prm, float("nan")), "bn_batch": torch.full((L * 2 * 2 * 10,), float("nan"), device=dev)}
    shp = G.shape_struct(B, N, P, L)
    nbytes = lib.rulgnn_stgcn_train_workspace_bytes(C.byref(shp))
    assert nbytes <= ws.numel() * 4
    a = _lib.StgcnTrainArgs()
    a.x = x.data_ptr(); a.y = y.data_ptr(); a.dpred = None; a.params = prm.data_ptr()
    a.grads = out["grads"].data_ptr(); a.pred = out["pred"].data_ptr(); a.loss = out["loss"].data_ptr(); a.bn_batch = out["bn_batch"].data_ptr()
    a.workspace = ws.data_ptr(); a.workspace_bytes = nbytes
    a.global_batch = B; a.sample_offset = 0
    a.dropout_p = dropout; a.seed = seed; a.step = step
    rc = lib.rulgnn_stgcn_train_step_path_f32(C.byref(shp), C.byref(a), None, path, G.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return {k: v.cpu().numpy() for k, v in out.items()}


_STALE = [(N, P, B, L, p, path)
          for (N, P) in ((14, 30), (12, 21)) for B in (1, 3, 5, 38, 251) for L in (1, 2, 3) for p in (0.0, 0.2)
          for path in (_MX, _PERSIST) if path == _MX or L == 2]


@pytest.mark.parametrize("N,P,B,L,p,path", _STALE)
def test_stale_workspace_does_not_reach_the_step(N, P, B, L, p, path):
    import gpu_util as G
    x, y, flat, (pred, loss, gref, bnb) = _case(N, P, L, B, p)
    rc0, zero = ws_step(x, y, flat, N, P, L, _path(path), 0.0, dropout=p, seed=5, step=2)
    rc1, nan = ws_step(x, y, flat, N, P, L, _path(path), float("nan"), dropout=p, seed=5, step=2)
    assert rc0 == 0 and rc1 == 0, (rc0, rc1)
    for k in _KEYS:
        assert np.all(np.isfinite(zero[k])), k
        assert np.array_equal(_bits(zero[k]), _bits(nan[k])), k
    assert G.rel_err(nan["pred"], pred) < TOL
    assert abs(float(nan["loss"][0]) - loss) < TOL * abs(loss)
    assert G.rel_err(nan["bn_batch"], bnb) < TOL
    check_grads(nan["grads"], gref, N, L)


@pytest.mark.parametrize("N,P,L,p,path", [(14, 30, 2, 0.2, _MX), (14, 30, 2, 0.2, _PERSIST), (14, 30, 3, 0.2, _MX), (14, 30, 1, 0.0, _MX),
                                          (12, 21, 2, 0.2, _MX), (12, 21, 2, 0.0, _PERSIST)])
def test_shrinking_batch_on_one_workspace(N, P, L, p, path):
    """B = 8 (two full tiles), then B = 5 on the same workspace with the same parameters: tile 1 of every record holds four samples of
    the first step, three of them beyond the second step's batch."""
    import gpu_util as G
    _, x8, y8, flat = _inputs(N, P, L, 8)
    x5, y5 = x8[:5], y8[:5]
    nbytes = _lib.load().rulgnn_stgcn_train_workspace_bytes(C.byref(G.shape_struct(8, N, P, L)))
    used = torch.zeros((nbytes + 3) // 4, dtype=torch.float32, device="cuda:0")
    first = _step_on(used, x8, y8, flat, N, P, L, _path(path), p, 5, 2)
    assert all(np.all(np.isfinite(first[k])) for k in _KEYS)
    second = _step_on(used, x5, y5, flat, N, P, L, _path(path), p, 5, 2)
    rc, fresh = ws_step(x5, y5, flat, N, P, L, _path(path), 0.0, dropout=p, seed=5, step=2)
    assert rc == 0, rc
    for k in _KEYS:
        assert np.all(np.isfinite(fresh[k])), k
        assert np.array_equal(_bits(second[k]), _bits(fresh[k])), k
