"""-m gpu: synchronised BatchNorm on ONE rank is the plain step, bit for bit.

The step every family shares (csrc/optim.hip: sync_cells) sums the 16 replicas of a reduction pair into replica 0 in the readers' own
order and zeroes the others, so every reader's replica sum is what it was before; with a no-op all-reduce, ``bn_param_grad_scale`` 1
and ``global_batch`` = the batch, nothing else separates the two entries.  So ``pred``, the loss, the whole bucket and ``_bn_batch`` must
be EQUAL, not close: a collapse that summed in another order, missed a replica or zeroed the wrong cells shows here as a changed bit.

The batches are small enough that every reducing launch has at most 16 workgroups -- one atomic add per replica, no order to vary --
and each case first shows that: the plain step twice, equal, or the case fails."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _stgcn(N, P, B):
    from gnn_rul_benchmarking_amd import _lib
    from gnn_rul_benchmarking_amd.stgcn import ST_GCN_model
    torch.manual_seed(3)
    m = ST_GCN_model(N, P, num_layers=2, dropout=0.0).to(DEV).train()
    m.step_path = _lib.STEP_CHAIN             # num_patch <= 64: both entries on the fp32 phases (num_patch > 64 has one launch form)
    g = torch.Generator(device=DEV).manual_seed(B)
    x, y = torch.rand(B, N, P, device=DEV, generator=g), torch.rand(B, 1, device=DEV, generator=g)

    def plain():                                # rulgnn_stgcn_train_fwdbwd_f32
        x2d, yv = m._step_inputs(x, y)
        shp = m._shape(B)
        m._call("fwdbwd", shp, m._args(shp, x2d, 1, y=yv))
    return m, x, y, plain


def _astgcnn():
    from test_astgcnn_gpu import build_model, cfg_of, load_case
    z, _ = load_case("astgcnn_small_5x12_bs9")
    m = build_model(cfg_of(z), {k[3:]: z[k] for k in z.files if k.startswith("sd:")}).train()
    x, y = torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(z["y"]).to(DEV)
    return m, x, y, lambda: m.fused_mse_step(x, y, update_running_stats=False)


def _fcstgnn():
    from test_fcstgnn_gpu import build_model, load_case
    z, cfg, _ = load_case("fcstgnn_fd003like_6p_bs2")
    m = build_model(cfg, {k[3:]: z[k] for k in z.files if k.startswith("sd:")}, dropout=0.0).train()
    x, y = torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(z["y"]).to(DEV)
    return m, x, y, lambda: m.fused_mse_step(x, y, update_running_stats=False)


CASES = {"stgcn_14x30_bs8": lambda: _stgcn(14, 30, 8), "stgcn_40x64_bs5": lambda: _stgcn(40, 64, 5),
         "stgcn_tiled_160x16_bs3": lambda: _stgcn(160, 16, 3), "astgcnn_small_5x12_bs9": _astgcnn,
         "fcstgnn_fd003like_6p_bs2": _fcstgnn}


def _results(m, run):
    """pred, the whole bucket [gradient | loss | tail] and _bn_batch of one step, as bit patterns (every buffer poisoned first)."""
    for t in (m.bucket, m._bn_batch):
        t.fill_(float("nan"))
    if m._pred_buf is not None:
        m._pred_buf.fill_(float("nan"))
    run()
    torch.cuda.synchronize()
    return {"pred": m._pred_buf.view(torch.int32).clone(), "bucket": m.bucket.view(torch.int32).clone(),
            "bn_batch": m._bn_batch.view(torch.int32).clone()}


@pytest.mark.parametrize("case", list(CASES))
def test_synchronised_step_on_one_rank_equals_the_plain_step_bit_for_bit(case):
    m, x, y, plain = CASES[case]()
    B = x.size(0)
    first, second = _results(m, plain), _results(m, plain)
    for k in first:
        assert torch.equal(first[k], second[k]), f"{case}: the plain step is not reproducible in {k}: nothing can be pinned on it"
    nl = m.num_live
    assert torch.isfinite(first["bucket"][:nl + 1].view(torch.float32)).all() and torch.isfinite(first["pred"].view(torch.float32)).all()

    seen = []                                    # (byte offset inside the workspace, doubles) of every all-reduce

    def allreduce(view):
        assert view.dtype == torch.float64 and view.is_cuda
        seen.append((view.data_ptr() - m._ws.data_ptr(), view.numel()))
    sync = _results(m, lambda: m.fused_mse_step_syncbn(x, y, B, 0, 1.0, allreduce))
    print(case, "all-reduces (workspace byte offset, doubles):", seen)
    schedule = m.sync_bn_schedule()
    assert [n for _, n in seen] == schedule and len(seen) == len(schedule)
    if case.startswith("stgcn"):
        assert len(seen) == 4 * m.num_layers
    for k in first:
        diff = int((sync[k] != first[k]).sum())
        assert diff == 0, f"{case}: {k} differs from the plain step in {diff} of {first[k].numel()} words"
