"""-m gpu: ``DataParallel(sync_bn=True)`` on ST_GCN's tiled path with the real kernels in two processes (both on cuda:0, gloo), against
the single-process ``update`` on the concatenated batch -- the helpers and tolerances of tests/test_dp_2proc_gpu.py.  Blocking form (one
bucket all-reduce behind the step) and overlapped form (the bucket leaves in gradient-ready regions between the cell reductions), unequal
shards and an empty shard, the process group's and the peer mailboxes' cell reductions."""
import pytest
import torch.multiprocessing as mp

from test_dp_2proc_gpu import STGCN_TILED, _check, _free_port, _run, _single_process, _worker

pytestmark = pytest.mark.gpu


def _covers_once(regions, numel):
    pos = 0
    for lo, hi in sorted(regions):
        if lo != pos:
            return False
        pos = hi
    return pos == numel


def _bucket_floats():
    from gnn_rul_benchmarking_amd.stgcn import ST_GCN_model
    return ST_GCN_model(**STGCN_TILED[1]).bucket.numel()          # (host replica: the bucket's size is a function of the shape)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("B", [9, 1])
@pytest.mark.parametrize("overlap_min", [None, 1024], ids=["blocking", "overlapped"])
def test_stgcn_tiled_path_synchronised_batchnorm_two_processes(B, overlap_min):
    r0, r1, ref = _run(STGCN_TILED, B, True, overlap_min=overlap_min)
    assert r1["shard"] == B // 2
    if overlap_min is None:
        assert r0["regions"] is None and r1["regions"] is None
    else:
        assert r0["regions"] is not None and r0["regions"] == r1["regions"] and len(r0["regions"]) >= 3
        assert _covers_once(r0["regions"], _bucket_floats())
    _check(r0, r1, ref, 2e-4)


@pytest.mark.timeout(600)
def test_stgcn_tiled_path_synchronised_batchnorm_over_the_peer_mailboxes():
    """``bn_collective="peer"``: the 4 L cell reductions of a step as device-side one-shot all-reduces (no Python frame between the
    kernels), the bucket in gradient-ready regions through the process group."""
    family, cfg, shape = STGCN_TILED
    B = 9
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(2, _free_port(), family, cfg, shape, B, True, 1024, out, 1.0, True, "peer"), nprocs=2, join=True)
    r0, r1 = out[0], out[1]
    assert r0["peer_collectives"] == r1["peer_collectives"] == 2 * 8          # two steps of 4 L
    assert r0["regions"] is not None and r0["regions"] == r1["regions"] and _covers_once(r0["regions"], _bucket_floats())
    _check(r0, r1, _single_process(family, cfg, shape, B, True), 2e-4)
