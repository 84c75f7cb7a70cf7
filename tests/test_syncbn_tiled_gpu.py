"""-m gpu: synchronised BatchNorm on ST_GCN's TILED path (num_patch > 64, and what the LDS gates send there): the shapes the
reference itself wires (XJTU-SY 1024 x 32, PHM2012 Condition_2 160 x 16).  Two data-parallel ranks are emulated on one GPU as in
tests/test_syncbn_gpu.py (two replicas, two host threads, two streams, a two-party rendezvous as the all-reduce).

* the two shards are the whole batch: against the fp64 oracle ON THE WHOLE BATCH under the gates tests/test_train_gpu.py applies to the
  tiled path's single call, and against the library's own full-batch call under the phase chains' tighter bounds;
* a world of one is the plain step, within the run-to-run spread of two plain calls;
* the C-ABI refuses what it documents before any launch, and makes its two kinds of callback in the documented interleaved order."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

from gnn_rul_benchmarking_amd import _lib
from gnn_rul_benchmarking_amd import params as PL
from oracle import stgcn_oracle as O
from test_syncbn_gpu import DEV, TwoPartySum, _replica
from test_train_gpu import GTOL, TOL, check_grads, oracle_step

pytestmark = pytest.mark.gpu
SEED = 5          # _replica's dropout seed; the replicas' first training forward is dropout step 1

# (N, P, L, B, split, p): all on the tiled path
SHAPES = [(72, 8, 2, 9, 4, 0.2),
          (160, 16, 2, 37, 18, 0.2),          # PHM2012 Condition_2: the batched parameter-gradient launch
          (300, 5, 3, 11, 10, 0.0),           # three layers
          (1024, 32, 2, 24, 7, 0.3),          # XJTU-SY: split-K products
          (256, 8, 2, 1024, 300, 0.2),        # the large products on pre-split operands (batch * 10 >= 2048 rows on both shards)
          (40, 136, 2, 13, 6, 0.2)]           # num_patch <= 64 past the LDS edge


# distance of the full-batch call to the fp64 oracle on the commit before this feature, where a bound of the full-batch comparison
# was missed (see that test's docstring): (N, P, L, B) -> gradient tensor -> max |diff| / max |oracle|
_PARENT_TO_ORACLE = {(256, 8, 2, 1024): {"sg_tcn.layers.1.0.theta.0.bias": 4.527e-5}}


def _inputs(N, P, L, B):
    rng = np.random.default_rng(N * 1000 + P * 10 + B)
    prm = O.random_params(N, L, seed=B)
    x = rng.uniform(0, 1, (B, N, P)).astype(np.float32)
    y = rng.uniform(0, 1, (B,)).astype(np.float32)
    flat, _ = PL.pack_numpy(prm, N, L)
    return prm, x, y, flat


def _model(N, P, L, p, flat):
    m = _replica(N, P, L, p, seed=SEED)
    with torch.no_grad():
        m.flat_params.copy_(torch.from_numpy(flat).to(DEV))
    return m


def _two_shards(N, P, L, B, split, p, flat, x, y):
    """Both ranks' synchronised steps; returns (ranks, calls)."""
    ranks = [_model(N, P, L, p, flat), _model(N, P, L, p, flat)]
    bounds = [(0, split), (split, B)]
    comm = TwoPartySum()
    errors = []

    def run(rank):
        try:
            with torch.cuda.stream(torch.cuda.Stream(device=DEV)):
                lo, hi = bounds[rank]
                ranks[rank].fused_mse_step_syncbn(x[lo:hi], y[lo:hi], B, lo, 1.0 if rank == 0 else 0.0, lambda v: comm(rank, v))
                torch.cuda.current_stream().synchronize()
        except BaseException as e:                  # pragma: no cover
            errors.append(e)
            comm.barrier.abort()
    torch.cuda.synchronize()
    ts = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(180)
    assert not any(t.is_alive() for t in ts), "a rank did not finish"
    assert not errors, errors
    torch.cuda.synchronize()
    return ranks, comm.calls


@pytest.mark.parametrize("N,P,L,B,split,p", SHAPES)
def test_two_shards_on_the_tiled_path_equal_the_oracle_on_the_whole_batch(N, P, L, B, split, p):
    prm, x_np, y_np, flat = _inputs(N, P, L, B)
    x, y = torch.from_numpy(x_np).to(DEV), torch.from_numpy(y_np).to(DEV).view(B, 1)
    assert _lib.load().rulgnn_stgcn_train_step_resolve(C.byref(_lib.StgcnShape(split, N, P, L, 1)), None, _lib.STEP_AUTO) == _lib.EUNSUPPORTED
    ranks, calls = _two_shards(N, P, L, B, split, p, flat, x, y)
    assert calls == [4 * L, 4 * L]
    pred_o, loss_o, grad_o, bn_o = oracle_step(prm, x_np, y_np, N, P, L, p, SEED, 1)
    import gpu_util as G
    pred = torch.cat([ranks[0]._pred_buf[:split], ranks[1]._pred_buf[:B - split]]).cpu().numpy()
    nl = ranks[0].num_live
    loss = float(ranks[0].bucket[nl] + ranks[1].bucket[nl])
    grad = (ranks[0].bucket[:nl] + ranks[1].bucket[:nl]).cpu().numpy()
    e_pred, e_loss = G.rel_err(pred, pred_o), abs(loss - loss_o) / abs(loss_o)
    e_bn = [G.rel_err(r._bn_batch.reshape(-1).cpu().numpy(), bn_o) for r in ranks]
    print(f"syncbn-tiled oracle {N}x{P} L{L} B{B}: pred {e_pred:.3e} loss {e_loss:.3e} bn {e_bn[0]:.3e} {e_bn[1]:.3e}")
    assert e_pred < TOL
    assert e_loss < TOL
    assert e_bn[0] < TOL and e_bn[1] < TOL                 # every rank holds the statistics of the GLOBAL batch
    check_grads(grad, grad_o, N, L)


@pytest.mark.parametrize("N,P,L,B,split,p", SHAPES)
def test_two_shards_on_the_tiled_path_equal_the_full_batch_call(N, P, L, B, split, p):
    """The tighter regression guard: the library's own ``fused_mse_step`` on the whole batch, under the bounds tests/test_syncbn_gpu.py
    uses for the phase chains (2e-6 of max |pred|, 1e-5 on the loss and the statistics, 2e-5 of max |grad| per tensor).

    One bound is not the phase chains': at 256 x 8, batch 1024 (shards 300 + 724) the gradient of layer 1's theta bias -- column sums
    over batch * 10 = 10 240 rows of d Hpre, whose producer runs the two-plane f16 split with operand scales taken from the SHARD's
    partial maxima -- came out 2.525e-5 of max |grad| from the full-batch call.  Measured at that shape on the commit before this
    feature: its full-batch call is 4.527e-5 from the fp64 oracle for that tensor (the same figure in three runs).  Two roundings of
    that class, one per side: the bound for that tensor at that shape is 2 x 4.527e-5 = 9.054e-5 (profiles/r10_syncbn_tiled.md).
    Every other tensor and shape holds the phase chains' 2e-5, and the oracle test above holds GTOL for all of them."""
    _, x_np, y_np, flat = _inputs(N, P, L, B)
    x, y = torch.from_numpy(x_np).to(DEV), torch.from_numpy(y_np).to(DEV).view(B, 1)
    full = _model(N, P, L, p, flat)
    pred_f, loss_f = full.fused_mse_step(x, y)
    pred_f, loss_f = pred_f[:B].clone(), float(loss_f)
    nl = full.num_live
    grad_f, bn_f = full.bucket[:nl].clone(), full._bn_batch.clone()
    ranks, calls = _two_shards(N, P, L, B, split, p, flat, x, y)
    assert calls == [4 * L, 4 * L]
    pred = torch.cat([ranks[0]._pred_buf[:split], ranks[1]._pred_buf[:B - split]])
    loss = float(ranks[0].bucket[nl] + ranks[1].bucket[nl])
    grad = ranks[0].bucket[:nl] + ranks[1].bucket[:nl]
    e_pred = float((pred - pred_f).abs().max()) / float(pred_f.abs().max())
    e_loss = abs(loss - loss_f) / abs(loss_f)
    e_grad = {}
    for name, (off, shape) in PL.live_param_layout(N, L).items():
        n = int(np.prod(shape))
        ref, got = grad_f[off:off + n], grad[off:off + n]
        e_grad[name] = float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-6)
    worst = max(e_grad, key=e_grad.get)
    e_bn = max(float(((r._bn_batch - bn_f).abs() / (1e-5 * bn_f.abs() + 1e-7)).max()) for r in ranks)
    print(f"syncbn-tiled full {N}x{P} L{L} B{B}: pred {e_pred:.3e} loss {e_loss:.3e} bn(allclose ratio) {e_bn:.3f} "
          f"grad {e_grad[worst]:.3e} ({worst})")
    assert e_pred < 2e-6
    assert e_loss < 1e-5
    for r in ranks:
        assert torch.allclose(r._bn_batch, bn_f, rtol=1e-5, atol=1e-7)
    for name, e in e_grad.items():
        assert e < max(2e-5, 2.0 * _PARENT_TO_ORACLE.get((N, P, L, B), {}).get(name, 0.0)), (name, e)


# ---- C-ABI ---------------------------------------------------------------------------------------------------------------------------
class _Call:
    """One call of a training entry on NaN-filled outputs (the argument struct of gpu_util.abi_train)."""

    def __init__(self, x_np, y_np, flat, N, P, L, dropout=0.2, global_batch=None):
        lib = _lib.load()
        B = x_np.shape[0]
        self.B, self.N, self.L = B, N, L
        self.x = torch.from_numpy(np.ascontiguousarray(x_np.reshape(B, -1), np.float32)).to(DEV)
        self.y = torch.from_numpy(np.ascontiguousarray(y_np.reshape(B), np.float32)).to(DEV)
        self.prm = torch.from_numpy(flat.copy()).to(DEV)
        self.grads = torch.full_like(self.prm, float("nan"))
        self.pred = torch.full((B,), float("nan"), device=DEV)
        self.loss = torch.full((1,), float("nan"), device=DEV)
        self.bnb = torch.full((L * 2 * 2 * 10,), float("nan"), device=DEV)
        self.shp = _lib.StgcnShape(B, N, P, L, 1)
        nbytes = lib.rulgnn_stgcn_train_workspace_bytes(C.byref(self.shp))
        assert nbytes > 0
        self.ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
        a = self.a = _lib.StgcnTrainArgs()
        a.x = self.x.data_ptr(); a.y = self.y.data_ptr(); a.dpred = None
        a.params = self.prm.data_ptr(); a.grads = self.grads.data_ptr(); a.pred = self.pred.data_ptr(); a.loss = self.loss.data_ptr()
        a.bn_batch = self.bnb.data_ptr(); a.workspace = self.ws.data_ptr(); a.workspace_bytes = nbytes
        a.global_batch = B if global_batch is None else global_batch
        a.sample_offset = 0
        a.dropout_p = dropout; a.seed = 99; a.step = 5
        self.st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def plain(self, ready=None):
        """The plain entry; with ``ready`` its gradient-ready form (other launch forms of the parameter-gradient products)."""
        if ready is None:
            rc = _lib.load().rulgnn_stgcn_train_fwdbwd_f32(C.byref(self.shp), C.byref(self.a), self.st)
        else:
            rc = _lib.load().rulgnn_stgcn_train_fwdbwd_ready_f32(C.byref(self.shp), C.byref(self.a), ready, None, self.st)
        torch.cuda.synchronize()
        return rc

    def sync(self, scale, cell, which="plain", ready=None):
        lib = _lib.load()
        if which == "plain":
            rc = lib.rulgnn_stgcn_train_fwdbwd_syncbn_f32(C.byref(self.shp), C.byref(self.a), scale, cell, None, self.st)
        elif which == "path":
            rc = lib.rulgnn_stgcn_train_fwdbwd_syncbn_path_f32(C.byref(self.shp), C.byref(self.a), scale, cell, None, _lib.STEP_AUTO, self.st)
        else:
            rc = lib.rulgnn_stgcn_train_fwdbwd_syncbn_ready_f32(C.byref(self.shp), C.byref(self.a), scale, cell, None, ready, None, self.st)
        torch.cuda.synchronize()
        return rc

    def out(self):
        return {"pred": self.pred.cpu().numpy(), "loss": self.loss.cpu().numpy(), "grads": self.grads.cpu().numpy(),
                "bn_batch": self.bnb.cpu().numpy()}

    def untouched(self):
        return all(np.isnan(v).all() for v in self.out().values())


_KEEP = _lib.ALLREDUCE_F64_FN(lambda u, b, c, s: 0)            # a world of one: the cells are the global sums already
_NO_CELL, _NO_READY = C.cast(None, _lib.ALLREDUCE_F64_FN), C.cast(None, _lib.GRAD_READY_FN)


@pytest.mark.parametrize("N,P,B", [(160, 16, 37), (1024, 32, 24)])
@pytest.mark.parametrize("which", ["plain", "path", "ready"])
def test_a_world_of_one_is_the_plain_step(N, P, B, which):
    """global_batch == batch, bn_param_grad_scale = 1, a callback that leaves the cells as they are: the collapse hands every consumer
    the sum it had, so only the order of the fp64 atomics differs from the plain call -- as it does between two plain calls.  Allowed:
    4 x the spread of two plain calls, with a floor of one fp32 ulp of the tensor's maximum."""
    L = 2
    _, x, y, flat = _inputs(N, P, L, B)
    p1, p2, s = (_Call(x, y, flat, N, P, L) for _ in range(3))
    ready = _lib.GRAD_READY_FN(lambda u, g, o, c, st: 0)
    # (the entry that also reports regions against the plain entry that does: with a ready callback the parameter-gradient products
    # take other launch forms -- no batched launch, no side stream -- which round differently whatever the BatchNorm statistics)
    plain_ready = ready if which == "ready" else None
    assert p1.plain(plain_ready) == 0 and p2.plain(plain_ready) == 0
    assert s.sync(1.0, _KEEP, which, ready) == 0
    a, b, got = p1.out(), p2.out(), s.out()
    tensors = {k: (a[k], b[k], got[k]) for k in ("pred", "loss", "bn_batch")}
    for name, (off, shape) in PL.live_param_layout(N, L).items():
        n = int(np.prod(shape))
        tensors["grad:" + name] = tuple(v["grads"][off:off + n] for v in (a, b, got))
    for name, (ta, tb, tg) in tensors.items():
        assert np.isfinite(tg).all(), name
        spread = float(np.max(np.abs(ta.astype(np.float64) - tb)))
        ulp = float(np.spacing(np.float32(np.max(np.abs(ta)))))
        err = float(np.max(np.abs(tg.astype(np.float64) - ta)))
        assert err <= max(4.0 * spread, ulp), (name, err, spread, ulp)


@pytest.mark.parametrize("N,P,L,B", [(160, 16, 2, 6), (40, 136, 2, 5)])
def test_tiled_shapes_refuse_what_the_contract_documents_before_any_launch(N, P, L, B):
    _, x, y, flat = _inputs(N, P, L, B)
    c = _Call(x, y, flat, N, P, L)
    ready = _lib.GRAD_READY_FN(lambda u, g, o, cnt, st: 0)
    for which in ("plain", "path", "ready"):
        assert c.sync(2.0, _KEEP, which, ready) == _lib.EINVAL and c.untouched(), which
        assert c.sync(1.0, _NO_CELL, which, ready) == _lib.EINVAL and c.untouched(), which
        c.a.bn_moment_weight = 0.5
        assert c.sync(1.0, _KEEP, which, ready) == _lib.EINVAL and c.untouched(), which
        c.a.bn_moment_weight = 0.0
    assert c.sync(1.0, _KEEP, "ready", _NO_READY) == _lib.EINVAL and c.untouched()
    assert not bool(c.ws.any())                      # nothing ran: the zero-filled workspace is as it was
    # a failing callback of either kind ends the call with RULGNN_ECALLBACK
    fail = _lib.ALLREDUCE_F64_FN(lambda u, b, cnt, s: 1)
    for which in ("plain", "path", "ready"):
        assert c.sync(1.0, fail, which, ready) == _lib.ECALLBACK, which
    no = _lib.GRAD_READY_FN(lambda u, g, o, cnt, st: 1)
    assert c.sync(1.0, _KEEP, "ready", no) == _lib.ECALLBACK
    torch.cuda.synchronize()
    assert c.sync(1.0, _KEEP, "ready", ready) == 0 and np.isfinite(c.out()["grads"]).all()      # and the workspace is reusable afterwards


@pytest.mark.parametrize("N,P,L,B", [(160, 16, 2, 6), (300, 5, 3, 4), (1024, 32, 2, 3)])
def test_both_callbacks_come_in_the_order_of_the_collective_schedule(N, P, L, B):
    """rulgnn_stgcn_train_fwdbwd_syncbn_ready_f32: the regions are ``ready_regions()`` in order, the interleaving with the 4 L cell
    callbacks is ``sync_collective_schedule()``; every cell callback gets 20 doubles inside the workspace, every region lies in grads."""
    _, x, y, flat = _inputs(N, P, L, B)
    c = _Call(x, y, flat, N, P, L)
    m = _replica(N, P, L, 0.2)
    seen = []
    lo, hi = c.ws.data_ptr(), c.ws.data_ptr() + c.ws.numel()

    def cell(_u, buf, count, _s):
        seen.append(("cells", int(count)))
        return 0 if lo <= int(buf) and int(buf) + 8 * int(count) <= hi else 1

    def region(_u, grads, offset, count, _s):
        seen.append(("region", int(offset), int(count)))
        return 0 if int(grads) == c.grads.data_ptr() and 0 <= offset and offset + count <= c.grads.numel() else 1
    assert c.sync(1.0, _lib.ALLREDUCE_F64_FN(cell), "ready", _lib.GRAD_READY_FN(region)) == 0
    assert [s[1:] for s in seen if s[0] == "region"] == [tuple(r) for r in m.ready_regions()]
    assert seen == [tuple(s) for s in m.sync_collective_schedule()]
    assert len([s for s in seen if s[0] == "cells"]) == 4 * L
    # the plain synchronised entries make the cell callbacks alone
    seen.clear()
    assert c.sync(1.0, _lib.ALLREDUCE_F64_FN(cell), "plain") == 0
    assert seen == [("cells", 20)] * (4 * L)
