"""The stale-workspace checker of tests/family_kit.py (section 9) without a GPU: a module whose "kernels" are numpy on a host workspace
passes every fill at every call, and each planted fault -- a word read before it is written, a tile row beyond the batch folded into a
sum, an accumulator added into without being cleared, an index slot used before it is set -- makes at least one fill fail.  The table
of tests/test_stale_workspace_gpu.py must name every family of the package."""
import numpy as np
import pytest
import torch

import family_kit as K
import test_stale_workspace_gpu as T

F, TILE = 6, 4
FAULTS = ("read-before-write", "row-beyond-batch", "accumulator", "index")


class _Step(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, x, w):
        ctx.model, ctx.x = model, x
        return torch.from_numpy(model._forward(x.numpy(), True)).reshape(-1, 1)

    @staticmethod
    def backward(ctx, dpred):
        g = torch.from_numpy(ctx.model._backward(ctx.x.numpy(), dpred.reshape(-1).numpy().astype(np.float32)))
        ctx.model.bucket[:F + 1] = g
        return None, None, g.clone()


class Fake:
    """pred_b = h_b + bias + 0.01 sum_b h_b^2 + 0.1 h_j, h = x w, j = the arg-max of h; the workspace of a batch holds, in fp32 words,
    h and dpred (a tile of 4 samples each: the rows beyond the batch are never written), the accumulator, the index slot and a scratch
    word that only the backward writes."""

    def __init__(self, fault=None):
        rng = np.random.default_rng(3)
        self.fault = fault
        self._w = torch.nn.Parameter(torch.from_numpy(rng.standard_normal(F + 1).astype(np.float32)))
        self.flat_params = self._w.data
        self.bucket = torch.zeros(F + 2)
        self.num_live = F + 1
        self.running = torch.zeros(1)
        self._bufs, self._pin_bufs, self._step, self._seed, self.training = {}, False, 0, 7, True

    # ---- what the checker touches of a FlatModule ----
    def train(self):
        self.training = True
        return self

    def eval(self):
        self.training = False
        return self

    def _named(self):
        return [self._w]

    def state_dict(self):
        return {"w": self.flat_params.clone(), "running_mean": self.running.clone()}

    def load_state_dict(self, sd, strict=True):
        assert sorted(sd) == ["running_mean", "w"]
        self.flat_params.copy_(sd["w"])
        self.running.copy_(sd["running_mean"])

    def __call__(self, x):
        if self.training:
            self._step += 1
        if self.training and torch.is_grad_enabled():
            self._w.grad = None
            return _Step.apply(self, x, self._w)
        return torch.from_numpy(self._forward(x.numpy(), self.training)).reshape(-1, 1)

    def fused_mse_step(self, x, y, optimizer=None):
        self._step += 1
        B = x.shape[0]
        pred = self._forward(x.numpy(), True)
        diff = pred - y.numpy()
        self.bucket[:F + 1] = torch.from_numpy(self._backward(x.numpy(), (2.0 / B * diff).astype(np.float32)))
        with np.errstate(over="ignore"):                               # (a planted fault may have let garbage through)
            self.bucket[F + 1] = float(np.mean(diff * diff))
        if optimizer is not None:
            optimizer.apply(self.bucket[:F + 1].numpy())
        return torch.from_numpy(pred), self.bucket[F + 1].clone()

    # ---- the "kernels" ----
    def _carve(self, B):
        T_ = TILE * ((B + TILE - 1) // TILE)
        if B not in self._bufs:
            assert self._pin_bufs or len(self._bufs) < 2
            self._bufs[B] = (torch.empty(256 * ((4 * (2 * T_ + 3) + 255) // 256), dtype=torch.uint8).fill_(0x55),)
        ws = self._bufs[B][0].numpy()
        f, i = ws.view(np.float32), ws.view(np.int32)
        return T_, f[:T_], f[T_:2 * T_], f[2 * T_:2 * T_ + 1], i[2 * T_ + 1:2 * T_ + 2], f[2 * T_ + 2:2 * T_ + 3]

    def _forward(self, x, training):
        B = x.shape[0]
        T_, h, _, acc, idx, scratch = self._carve(B)
        w, bias = self.flat_params.numpy()[:F], self.flat_params.numpy()[F]
        h[:B] = x @ w
        rows = T_ if self.fault == "row-beyond-batch" else B
        if self.fault != "accumulator":
            acc[0] = 0.0
        for r in range(rows):
            acc[0] += h[r] * h[r]
        j = int(idx[0]) % B if self.fault == "index" else int(np.argmax(h[:B]))
        idx[0] = int(np.argmax(h[:B]))
        extra = scratch[0] if self.fault == "read-before-write" else np.float32(0)
        if training:
            self.running.mul_(0.9).add_(0.1 * float(h[:B].mean()))
        return (h[:B] + bias + np.float32(0.01) * acc[0] + np.float32(0.1) * h[j] + extra).astype(np.float32)

    def _backward(self, x, dpred):
        B = x.shape[0]
        _, h, d, _, idx, scratch = self._carve(B)                       # h and the index are the forward's tape
        d[:B] = dpred + np.float32(0.02) * dpred.sum() * h[:B]
        d[int(idx[0])] += np.float32(0.1) * dpred.sum()
        scratch[0] = dpred.sum()
        return np.concatenate([x.T @ d[:B], [dpred.sum()]]).astype(np.float32)


class FakeAdam:
    def __init__(self, m):
        self.m, self._exp_avg, self._exp_avg_sq, self._steps = m, torch.zeros(F + 1), torch.zeros(F + 1), 0

    def state_dict(self):
        return {"step": self._steps, "exp_avg": self._exp_avg.clone(), "exp_avg_sq": self._exp_avg_sq.clone()}

    def apply(self, g):
        self._steps += 1
        g = torch.from_numpy(g.copy())
        self._exp_avg.mul_(0.9).add_(0.1 * g)
        self._exp_avg_sq.mul_(0.999).add_(0.001 * g * g)
        self.m.flat_params.sub_(1e-2 * self._exp_avg / (self._exp_avg_sq.sqrt() + 1e-8))


def _draw(B, seed):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.standard_normal((B, F)).astype(np.float32)), torch.from_numpy(rng.uniform(0, 1, B).astype(np.float32))


def case(fault=None, bar=None):
    return K.StaleCase(lambda: Fake(fault), FakeAdam, _draw, lambda m: {k: v + 0.1 for k, v in m.state_dict().items()}, {}, bar)


def failures(fault, B, call):
    """The fills under which the checker raises."""
    base = K.stale_run(case(fault), B, "zero", call)
    K.stale_baseline_ok(base, call)
    bad = []
    for fill in K.STALE_FILLS[1:]:
        try:
            K.stale_compare(base, K.stale_run(case(fault), B, fill, call), fill, None)
        except AssertionError:
            bad.append(fill)
    return bad


@pytest.mark.parametrize("call", K.STALE_CALLS)
@pytest.mark.parametrize("B", [1, 3, 5])
def test_the_faultless_module_passes_every_fill(B, call):
    assert failures(None, B, call) == []


@pytest.mark.parametrize("fault", FAULTS)
def test_each_planted_fault_fails_under_at_least_one_fill(fault):
    caught = {(B, call): failures(fault, B, call) for B in (3, 5) for call in K.STALE_CALLS}
    print(fault, caught)
    assert all(caught[B, "step"] for B in (3, 5)), caught              # the fused step shows every one of them
    assert "nan" in caught[3, "step"] or "same-batch" in caught[3, "step"]


def test_the_zero_fill_alone_would_not_have_shown_them():
    """On a zeroed workspace the faults that read a float compute what the faultless module computes: what the suite had before.  (A
    zeroed index slot names sample 0, not the arg-max: that one a zeroed workspace does show.)"""
    want = K.stale_run(case(None), 3, "zero", "step")
    for fault in FAULTS[:3]:
        got = K.stale_run(case(fault), 3, "zero", "step")
        assert all(got[k].tobytes() == want[k].tobytes() for k in want), fault


def test_compare_refuses_a_fill_that_did_not_take_one_ulp_a_signed_zero_and_a_nan():
    base = {"filled:1": np.asarray(0), "step1:pred": np.array([1.0, 0.0, -2.0], np.float32), "step1:_step": np.asarray(1)}
    good = dict(base, **{"filled:1": np.asarray(12)})
    K.stale_compare(base, good, "nan", None)
    with pytest.raises(AssertionError, match="left the workspace as the baseline's"):
        K.stale_compare(base, dict(base), "nan", None)
    ulp = dict(good, **{"step1:pred": np.array([np.nextafter(np.float32(1), np.float32(2)), 0.0, -2.0], np.float32)})
    with pytest.raises(AssertionError, match="1 of 3 elements differ"):
        K.stale_compare(base, ulp, "nan", None)
    with pytest.raises(AssertionError):
        K.stale_compare(base, dict(good, **{"step1:pred": np.array([1.0, -0.0, -2.0], np.float32)}), "nan", None)
    with pytest.raises(AssertionError):
        K.stale_compare(base, dict(good, **{"step1:_step": np.asarray(2)}), "nan", None)
    with pytest.raises(AssertionError):
        K.stale_compare(base, {k: v for k, v in good.items() if k != "step1:_step"}, "nan", None)
    # a relative bar: of the tensor's largest magnitude; finite; integers still equal
    K.stale_compare(base, ulp, "nan", 1e-6)
    off = dict(good, **{"step1:pred": np.array([1.0, 3e-6, -2.0], np.float32)})
    with pytest.raises(AssertionError, match="the bar is"):
        K.stale_compare(base, off, "nan", 1e-6)
    K.stale_compare(base, off, "nan", 2e-6)
    with pytest.raises(AssertionError, match="not finite"):
        K.stale_compare(base, dict(good, **{"step1:pred": np.array([1.0, np.nan, -2.0], np.float32)}), "nan", 1e-6)
    with pytest.raises(AssertionError):
        K.stale_compare(base, dict(good, **{"step1:_step": np.asarray(2)}), "nan", 1e-6)


def test_the_baseline_must_be_finite_on_zeros_and_have_a_gradient():
    ok = {"filled:1": np.asarray(0), "step1:bucket": np.array([0.0, 1.0], np.float32), "step1:pred": np.ones(2, np.float32)}
    K.stale_baseline_ok(ok, "step")
    with pytest.raises(AssertionError):
        K.stale_baseline_ok(dict(ok, **{"filled:1": np.asarray(3)}), "step")
    with pytest.raises(AssertionError):
        K.stale_baseline_ok(dict(ok, **{"step1:pred": np.array([1.0, np.inf], np.float32)}), "step")
    with pytest.raises(AssertionError, match="all zero"):
        K.stale_baseline_ok(dict(ok, **{"step1:bucket": np.zeros(2, np.float32)}), "step")


def test_the_table_names_every_family_of_the_package():
    T.check_table_is_complete()
    assert "ST_GCN" not in T.TABLE and len(T.package_families()) >= 19
