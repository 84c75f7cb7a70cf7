"""-m gpu: the matrix-core training step reads every parameter-derived operand (theta, the convolutions, their transposed forms, the head)
fresh in each phase's prologue.  Whatever changes the parameters between two fused steps -- ``load_state_dict``, an in-place edit of a
``state_dict`` tensor (a view into the flat buffer), a step the f16 range guard rejected and the fp32 chain repeated -- the next step must
be bit for bit the step of a fresh model loaded with the same state: same loss, same gradient bucket."""
import pytest
import torch

from gnn_rul_benchmarking_amd import _lib

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CFG = dict(num_patch=14, patch_size=30, dropout=0.2)
HP = {"learning_rate": 1e-3, "weight_decay": 1e-4}


def _algo(seed):
    from gnn_rul_benchmarking_amd.algorithms import ST_GCN
    torch.manual_seed(seed)
    a = ST_GCN(CFG, HP, DEV)
    a.to(DEV)
    a.train()
    return a


def _batch(seed, n=1000, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.rand(n, 14, 30, device=DEV, generator=g) * scale, torch.rand(n, 1, device=DEV, generator=g)


def _fresh_like(a):
    """A model that never took a step, holding a's parameters and BatchNorm buffers, at a's dropout stream position."""
    c = _algo(99)
    c.model.load_state_dict({k: v.clone() for k, v in a.model.state_dict().items()})
    c.model._seed, c.model._step = a.model._seed, a.model._step
    return c


def _same_next_step(a, c, X, y):
    la, lc = a.update(X, y, 1)["loss"], c.update(X, y, 1)["loss"]
    assert a.model._last_chain == c.model._last_chain == _lib.STEP_MX
    assert la == lc
    n = a.model.num_live
    assert torch.equal(a.model.bucket[:n], c.model.bucket[:n])


def test_step_after_load_state_dict_equals_a_fresh_model():
    a, b = _algo(11), _algo(12)
    X, y = _batch(1)
    for _ in range(2):
        a.update(X, y, 1)
    a.model.load_state_dict(b.model.state_dict())
    _same_next_step(a, _fresh_like(a), *_batch(2))


def test_step_after_an_in_place_parameter_edit_equals_a_fresh_model():
    a = _algo(13)
    X, y = _batch(3)
    a.update(X, y, 1)
    with torch.no_grad():
        for k, v in a.model.state_dict().items():
            if v.dtype.is_floating_point and "running" not in k:
                v.mul_(0.75)
    _same_next_step(a, _fresh_like(a), *_batch(4))


def test_step_after_a_guard_retry_on_the_fp32_chain_equals_a_fresh_model():
    a = _algo(14)
    X, y = _batch(5, scale=3.0e4)
    a.update(X, y, 1)                                  # rejected by the f16 range guard, repeated on the fp32 chain
    assert a.model.step_path == _lib.STEP_CHAIN
    a.model.step_path = _lib.STEP_AUTO
    _same_next_step(a, _fresh_like(a), *_batch(6))
