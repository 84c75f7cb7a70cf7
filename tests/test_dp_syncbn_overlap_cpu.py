"""world_size-2 gloo tests (CPU, no kernels) of ``DataParallel._sync_bn_step`` in its OVERLAPPED form: a model that takes synchronised
BatchNorm and also reports final gradient regions (ST_GCN's tiled path) keeps both -- the cell all-reduces between its kernels and the
bucket leaving in reported regions, then the complement.  The model is a duck-typed double that issues the collectives of its
``sync_collective_schedule()``; ``torch.distributed.all_reduce`` is wrapped in each worker to record what a rank really issued."""
import os
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from gnn_rul_benchmarking_amd.dp import DataParallel, shard_bounds
from test_dp_cpu import SgdFromBucket, _free_port

JOIN_S = 120
PAIRS = 8            # 4 L at L = 2


class SyncReadyModel:
    """4096 'gradients' + loss + 8 statistics; eight cell pairs of 20 doubles; two reported regions (backward order) between them."""
    reports_ready_gradients = True

    def __init__(self, deviate=False):
        self.num_live = 4096
        self.bucket = torch.zeros(self.num_live + 1 + 8, dtype=torch.float32)
        self.flat_params = torch.zeros(self.num_live)
        self._bn = torch.zeros(8)
        self._bn_batch = torch.zeros(8)
        self._nbt = torch.zeros(2, dtype=torch.int64)
        self._step = 0
        self.deviate = deviate
        self.cells_after = []

    def sync_bn_schedule(self):
        return [20] * PAIRS

    def ready_regions(self):
        return [(3000, 1096), (1000, 500)]

    def sync_collective_schedule(self):
        c, (head, theta) = ("cells", 20), [("region", o, n) for o, n in self.ready_regions()]
        return [c, c, c, c, head, c, c, theta, c, c]

    def fused_mse_step_syncbn(self, X, y, global_batch, sample_offset, bn_param_grad_scale, allreduce, grad_ready=None):
        assert grad_ready is not None
        self._step += 1
        b = X.shape[0]
        self.bucket[:self.num_live] = float(X.sum()) + torch.arange(self.num_live, dtype=torch.float32) * 1e-3
        order = self.sync_collective_schedule()
        if self.deviate:                         # the theta region in front of its layer's cell pairs: not what the schedule says
            order[5], order[7] = order[7], order[5]
        pair = 0
        for item in order:
            if item[0] == "cells":
                pair += 1
                v = torch.full((item[1],), float(pair * b), dtype=torch.float64)       # this rank's sums of pair number `pair`
                allreduce(v)
                self.cells_after.append(v.clone())
            else:
                grad_ready(item[1], item[2])
        self.bucket[self.num_live] = float(b)
        self._bn_batch[:] = 0.5                  # the GLOBAL statistics: the same on every rank that ran
        return None, self.bucket[self.num_live]

    def _after_train_forward(self, batch, from_bucket_moments=False, from_bucket_stats=False):
        assert from_bucket_stats
        self._nbt += 1


def _worker(rank, world, port, B, deviate, out):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        issued, real = [], dist.all_reduce

        def recording(t, *a, **k):
            issued.append((str(t.dtype), int(t.numel())))
            return real(t, *a, **k)
        dist.all_reduce = recording
        x = torch.arange(B * 3, dtype=torch.float32).reshape(B, 3) + 1.0
        y = torch.zeros(B, 1)
        model = SyncReadyModel(deviate)
        dp = DataParallel(sync_bn=True)
        dp.OVERLAP_MIN_BYTES = 1024
        lo, hi = shard_bounds(B, world, rank)
        error = None
        try:
            loss = float(dp.step(model, SgdFromBucket(model), x[lo:hi], y[lo:hi], global_batch=B, sample_offset=lo))
        except RuntimeError as e:
            error, loss = str(e), None
        out[rank] = {"loss": loss, "error": error, "bucket": model.bucket.clone().numpy(), "issued": issued,
                     "regions": list(getattr(dp, "last_overlap_regions", [])), "step": model._step, "shard": hi - lo,
                     "cells": [c.numpy() for c in model.cells_after], "nbt": model._nbt.numpy()}
    finally:
        dist.all_reduce = real
        dist.destroy_process_group()


def _spawn(B, deviate=False):
    """Two workers under a join time-out: a rank left waiting in a collective must fail the test, not hang it."""
    mgr = mp.Manager()
    out = mgr.dict()
    ctx = mp.spawn(_worker, args=(2, _free_port(), B, deviate, out), nprocs=2, join=False)
    deadline = time.monotonic() + JOIN_S
    while not ctx.join(timeout=5):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("the workers did not finish: a rank is waiting in a collective the other never issued")
    return out[0], out[1]


WIRE = [("torch.float64", 20)] * 4 + [("torch.float32", 1096)] + [("torch.float64", 20)] * 2 + [("torch.float32", 500)] + \
    [("torch.float64", 20)] * 2 + [("torch.float32", 1000), ("torch.float32", 1500), ("torch.float32", 9)]


@pytest.mark.parametrize("B", [5, 1])
def test_overlapped_synchronised_step_sums_everything_once_and_issues_one_sequence_world2_gloo(B):
    """Ranks (data, data) at B = 5 and (data, empty) at B = 1: the collectives on the wire are the model's interleaved schedule and
    the complement, identical on both ranks; every bucket element and every cell pair is summed exactly once."""
    r0, r1 = _spawn(B)
    assert r0["error"] is None and r1["error"] is None
    assert r1["shard"] == B // 2 and r0["step"] == r1["step"] == 1
    assert r0["issued"] == r1["issued"] == WIRE
    assert r0["regions"] == r1["regions"] == [(0, 1000), (1000, 1500), (1500, 3000), (3000, 4096), (4096, 4105)]
    assert np.array_equal(r0["bucket"], r1["bucket"])
    # cells: pair k held k * (this rank's shard) on every rank that ran -> k * B after exactly one sum
    for r in (r0, r1):
        assert len(r["cells"]) == (PAIRS if r["shard"] else 0)
        for k, c in enumerate(r["cells"]):
            assert np.array_equal(c, np.full(20, float((k + 1) * B)))
    # bucket: gradients, loss (samples counted once) and the weighted global statistics (0.5 from shard fractions that sum to one)
    x = np.arange(B * 3, dtype=np.float32).reshape(B, 3) + 1.0
    n0 = (B + 1) // 2
    want = sum(float(part.sum()) + np.arange(4096, dtype=np.float32) * 1e-3 for part in (x[:n0], x[n0:]) if part.shape[0] > 0)
    assert np.allclose(r0["bucket"][:4096], want, rtol=1e-6)
    assert r0["loss"] == r1["loss"] == float(B)
    assert np.allclose(r0["bucket"][4097:], 0.5, rtol=1e-6)
    assert np.array_equal(r0["nbt"], [1, 1]) and np.array_equal(r1["nbt"], [1, 1])


def test_a_model_that_leaves_its_schedule_is_reported_on_every_rank_after_the_collectives_world2_gloo():
    """The model reports the theta region in front of its layer's cell pairs (on both ranks alike, so the collectives still pair up):
    both ranks join everything -- the complement included -- and then raise; nobody is left waiting."""
    r0, r1 = _spawn(6, deviate=True)
    for r in (r0, r1):
        assert r["error"] is not None and "differ from the model's schedule" in r["error"]
        assert len(r["issued"]) == len(WIRE) and sorted(r["issued"]) == sorted(WIRE)
        assert r["regions"] == [(0, 1000), (1000, 1500), (1500, 3000), (3000, 4096), (4096, 4105)]

