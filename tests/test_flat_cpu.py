"""The base class of the model modules (gnn_rul_benchmarking_amd/flat.py): flat parameter views, bucket, workspace cache -- host logic,
no GPU."""
import pytest
import torch
import torch.nn as nn

from gnn_rul_benchmarking_amd import _lib, params as PL
from gnn_rul_benchmarking_amd.flat import FlatModule


class _Toy(FlatModule):
    bucket_tail = 3
    workspace_slots = 2
    bn_modules = ("bn",)

    def __init__(self, order=None):
        super().__init__()
        self.a = nn.Linear(3, 2)
        self.b = nn.Linear(2, 1)
        self.bn = nn.BatchNorm1d(2)
        if order is not None:
            self.flat_order = order
        self._track_batchnorm_counters()
        self._init_flat()


def test_parameters_are_views_of_one_flat_buffer_in_layout_order():
    torch.manual_seed(0)
    ref = [p.detach().clone() for p in nn.Sequential(nn.Linear(3, 2), nn.Linear(2, 1)).parameters()]
    torch.manual_seed(0)
    m = _Toy()
    assert m.num_live == 6 + 2 + 2 + 1 + 2 + 2 and m.flat_params.numel() == m.num_live     # a.w a.b b.w b.b bn.weight bn.bias
    assert m.bucket.numel() == m.num_live + 3 + 4                                          # [gradient | tail | BatchNorm moments]
    off = 0
    for (name, p), (o, n, shape) in zip(m._named_live(), m._slices):
        assert o == off and tuple(p.shape) == shape
        assert p.data_ptr() == m.flat_params.data_ptr() + 4 * o                            # a view, not a copy
        off += n
    for p, r in zip(list(m.parameters())[:4], ref):                                        # same RNG consumption as the plain modules
        assert torch.equal(p.detach(), r)
    m.flat_params.fill_(0.5)
    assert all(float(p.detach().min()) == 0.5 for p in m.parameters())


def test_flat_order_overrides_named_parameters_order():
    m = _Toy(order=["b.weight", "b.bias", "a.weight", "a.bias", "bn.weight", "bn.bias"])
    assert list(m._layout) == ["b.weight", "b.bias", "a.weight", "a.bias", "bn.weight", "bn.bias"]
    assert m.b.weight.data_ptr() == m.flat_params.data_ptr() and m.a.weight.data_ptr() == m.flat_params.data_ptr() + 4 * 3


def test_noop_apply_keeps_the_buffers_and_a_real_conversion_rebuilds_them():
    m = _Toy()
    flat0, hits = m.flat_params, []
    m._reflatten_listeners = [lambda: hits.append(1)]
    m.to(torch.device("cpu")).float()                                                      # the trainers' per-epoch no-op
    assert m.flat_params is flat0 and not hits
    m.double()                                                                             # converts tensor by tensor: views are gone
    assert m.flat_params is not flat0 and m.flat_params.dtype == torch.float32 and hits    # rebuilt (fp32 storage), listeners told
    assert PL.flat_views_intact(m)
    assert m.bn.running_mean.data_ptr() == m._bn.data_ptr()


def test_batchnorm_counter_is_flushed_when_somebody_looks():
    m = _Toy()
    m._nbt_pending = 5
    assert int(m.state_dict()["bn.num_batches_tracked"]) == 5 and m._nbt_pending == 0


def test_batchnorm_state_round_trips_through_the_flat_buffers():
    """running_mean then running_var of every BatchNorm module, module after module, in ``_bn``; one counter per module in ``_nbt``;
    the modules' buffers are views, so state_dict / load_state_dict and a rebuild go through the flat buffers."""
    m = _Toy()
    assert m._bn.numel() == m._bn_batch.numel() == 4 and not bool(m._bn_batch.any()) and m._nbt.numel() == 1
    sd = m.state_dict()
    sd["bn.running_mean"], sd["bn.running_var"], sd["bn.num_batches_tracked"] = (torch.tensor([1.0, 2.0]), torch.tensor([3.0, 4.0]),
                                                                                torch.tensor(7))
    m.load_state_dict(sd)
    assert m._bn.tolist() == [1.0, 2.0, 3.0, 4.0] and m._nbt.tolist() == [7]
    m._nbt_pending = 2
    m.double()                                                                             # rebuilds the flat buffers from the modules'
    assert m._bn.tolist() == [1.0, 2.0, 3.0, 4.0] and m._nbt.tolist() == [9] and m._nbt_pending == 0
    assert m.bn.running_var.data_ptr() == m._bn.data_ptr() + 4 * 2 and m.bn.num_batches_tracked.data_ptr() == m._nbt.data_ptr()
    back = m.state_dict()
    assert back["bn.running_mean"].tolist() == [1.0, 2.0] and back["bn.running_var"].tolist() == [3.0, 4.0]
    assert int(back["bn.num_batches_tracked"]) == 9


def test_batchnorm_fields_of_the_argument_struct():
    m = _Toy()
    m.Args = _lib.AstgcnnArgs
    a = m.Args()
    a.global_batch = 8
    m._bn_args(a, 2)
    assert (a.bn_stats, a.bn_batch, a.bn_moment_weight) == (m._bn.data_ptr(), m._bn_batch.data_ptr(), 0.0)
    m._bn_args(a, 2, moments_to_bucket=True)                                               # behind [gradient | tail], weight B / global
    assert a.bn_batch == m.bucket.data_ptr() + 4 * (m.num_live + 3) == m._bn_source(True) and a.bn_moment_weight == 0.25
    assert m._bn_source(False) == m._bn_batch.data_ptr()
    m.Args = _lib.StgcnTrainArgs                                                           # no bn_stats field: left out
    a = m.Args()
    a.global_batch = 2
    m._bn_args(a, 2, moments_to_bucket=True)
    assert not hasattr(a, "bn_stats") and a.bn_moment_weight == 1.0


def test_stgcn_batchnorm_modules_give_the_kernel_layout():
    from gnn_rul_benchmarking_amd.stgcn import ST_GCN_model
    for L in (1, 2, 3):
        m = ST_GCN_model(14, 30, num_layers=L)
        bufs = dict(m.named_buffers())
        for name, (off, shape) in PL.bn_buffer_layout(L).items():
            assert bufs[name].data_ptr() == m._bn.data_ptr() + 4 * off and tuple(bufs[name].shape) == shape
        assert m._bn.numel() == PL.bn_buffer_count(L) and m._nbt.numel() == 2 * L
        assert m.bucket.numel() == m.num_live + 1 + PL.bn_buffer_count(L)


def test_workspace_cache_evicts_the_oldest_size_unless_pinned():
    m = _Toy()
    sizes = []
    for B in (4, 8, 16):
        ws, pred = m._workspace_entry(B, lambda: 64, "unsupported")
        assert ws.numel() == 64 and pred.numel() == B
        sizes.append(B)
    assert list(m._bufs) == [8, 16]
    m._pin_bufs = True
    m._workspace_entry(32, lambda: 64, "unsupported")
    assert list(m._bufs) == [8, 16, 32]
    with pytest.raises(RuntimeError, match="not covered"):
        m._workspace_entry(64, lambda: 0, "configuration not covered")
    ent = m._workspace_entry(7, lambda: 16, "x", make=lambda dev: (torch.zeros(2), torch.zeros(3)))
    assert len(ent) == 3 and ent[2].numel() == 3


def test_adam_block_and_side_stream_defaults():
    m = _Toy()
    assert m._adam_args(None) is None
    s = PL.SideStream()
    assert s.pointer(torch.device("cpu"), training=False) is None
    s.enabled = False
    assert s.pointer(torch.device("cpu"), training=True) is None


class _AutogradToy(FlatModule):
    """y = lin(x) through the shared autograd Function; the "workspace" of a batch size holds the forward's input, which the backward
    reads -- the same hazard the HIP families have."""

    def __init__(self, consumes_tape=False, gradless_params=0):
        super().__init__()
        self.lin = nn.Linear(3, 1)
        self.consumes_tape, self.gradless_params = consumes_tape, gradless_params
        self._init_flat()

    def _run_forward(self, x):
        self._tape.mark(x.size(0))
        self._bufs[x.size(0)] = (x.clone(),)
        return (x @ self.lin.weight.detach().t() + self.lin.bias.detach(),)

    def _run_backward(self, x, douts):
        saved, d = self._bufs[x.size(0)][0], douts[0].reshape(-1, 1)
        self._grad_flat[:3] = (d * saved).sum(0)
        self._grad_flat[3] = d.sum()
        return self._grad_flat


def test_shared_autograd_function_raises_on_overwritten_activations_and_returns_per_parameter_gradients():
    torch.manual_seed(0)
    m, x = _AutogradToy(), torch.rand(4, 3)
    p1 = m._predict(x, autograd=True)[0]
    with torch.no_grad():
        m._predict(x * 0.5, autograd=False)                   # a second forward of the same batch size before the backward
    with pytest.raises(RuntimeError, match="overwritten"):
        p1.sum().backward()
    p2 = m._predict(x, autograd=True)[0]
    m._predict(torch.rand(5, 3), autograd=False)              # another batch size has its own workspace
    p2.sum().backward()
    assert torch.allclose(m.lin.weight.grad, x.sum(0, keepdim=True)) and float(m.lin.bias.grad) == 4.0
    assert m.lin.weight.grad.data_ptr() != m._grad_flat.data_ptr()                      # clones, not views of the bucket


def test_shared_autograd_function_consumes_the_tape_and_skips_gradless_parameters():
    x = torch.rand(4, 3)
    m = _AutogradToy(consumes_tape=True, gradless_params=1)
    loss = m._predict(x, autograd=True)[0].sum()
    loss.backward(retain_graph=True)
    assert m.lin.weight.grad is None and float(m.lin.bias.grad) == 4.0
    with pytest.raises(RuntimeError, match="ran twice"):
        loss.backward()
