"""tests/adam_reference.py checked without a GPU: the fp64 reference IS torch.optim.Adam, and its error bounds hold (with room) for an
independent fp32 implementation -- torch.optim.Adam in fp32 on the CPU -- on the very inputs the GPU tests feed the HIP kernels.

torch gets the hyper-parameters as the C ABI's ``float`` sees them (``adam_reference.f32``): the kernels are handed fp32(0.9), not 0.9,
and 1 - fp32(0.999) differs from 1 - 0.999 by 1.3e-5 relative, far above any rounding bound."""
import numpy as np
import pytest
import torch

import adam_reference as R

HP = R.DEFAULT


def _torch_adam(p0, m0, v0, k0, wd, dtype):
    """A torch.optim.Adam over one tensor with moments (m0, v0) after k0 steps."""
    p = torch.nn.Parameter(torch.from_numpy(np.asarray(p0)).to(dtype).clone())
    opt = torch.optim.Adam([p], lr=R.f32(HP["lr"]), betas=(R.f32(HP["beta1"]), R.f32(HP["beta2"])), eps=R.f32(HP["eps"]),
                           weight_decay=R.f32(wd), foreach=False)
    opt.state[p] = {"step": torch.tensor(float(k0)), "exp_avg": torch.from_numpy(np.asarray(m0)).to(dtype).clone(),
                    "exp_avg_sq": torch.from_numpy(np.asarray(v0)).to(dtype).clone()}
    return p, opt


def _torch_step(p, opt, g):
    p.grad = torch.from_numpy(np.asarray(g)).to(p.dtype).clone()
    opt.step()
    s = opt.state[p]
    return tuple(t.detach().numpy().copy() for t in (p, s["exp_avg"], s["exp_avg_sq"]))


def _same_to_1e14(got, want, prev, g, k):
    """Element by element to 1e-14 of the operands' magnitudes (m and p are sums that may cancel: an element's own value is no scale)."""
    for name, a, w, before in zip("pmv", got, want, prev):
        scale = np.abs(w) + np.abs(before) + (np.abs(g) + np.abs(prev[0]) if name == "m" else 0.0)
        assert (np.abs(a - w) <= 1e-14 * scale).all(), (name, k)


@pytest.mark.parametrize("wd", [0.0, 1e-4, 0.1])
def test_reference_is_torch_adam_in_fp64_over_five_steps(wd):
    p0, g, m0, v0 = R.inputs(1025, 11)
    rng = np.random.default_rng(12)
    p, opt = _torch_adam(p0, m0, v0, 6, wd, torch.float64)
    cur = tuple(a.astype(np.float64) for a in (p0, m0, v0))
    for k in range(7, 12):
        gk = R.gradient(1025, rng)
        got = _torch_step(p, opt, gk.astype(np.float64))
        prev = cur
        cur = R.reference(cur[0], gk, cur[1], cur[2], k, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], wd, 1.0)
        _same_to_1e14(got, cur, prev, gk, k)


def test_reference_from_zero_moments_is_torch_adam_in_fp64():
    p0, _, _, _ = R.inputs(257, 13)
    rng = np.random.default_rng(14)
    p = torch.nn.Parameter(torch.from_numpy(p0.astype(np.float64)))
    opt = torch.optim.Adam([p], lr=R.f32(HP["lr"]), betas=(R.f32(HP["beta1"]), R.f32(HP["beta2"])), eps=R.f32(HP["eps"]),
                           weight_decay=R.f32(1e-4), foreach=False)
    cur = (p0.astype(np.float64), np.zeros(257), np.zeros(257))
    for k in range(1, 6):
        gk = R.gradient(257, rng)
        got = _torch_step(p, opt, gk.astype(np.float64))
        prev = cur
        cur = R.reference(cur[0], gk, cur[1], cur[2], k, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], 1e-4, 1.0)
        _same_to_1e14(got, cur, prev, gk, k)


def test_fp32_torch_adam_stays_within_half_the_bounds_on_the_gpu_tests_inputs():
    """Every size x step x (weight decay, gradient scale) case of tests/test_adam_kernels_gpu.py, plus the zero-moment trajectory.
    The gradient scale is a power of two, so handing torch g * gscale changes no rounding.

    Within the bounds on every element, and with 2x room on m, v and the accumulated part of bound_p.  That is one quantity fewer than
    asked for ("at least 2x room" on p, m and v): p as a whole cannot have it.  bound_p itself is reached
    (measured 0.997): its u |p| term is the one rounding of the result, which is sharp for a p just above a power of two -- any
    correct fp32 Adam gets there, so room is asked of what the derivation budgets with a factor, not of that term."""
    worst = dict(p=0.0, m=0.0, v=0.0, p_acc=0.0)
    sizes = R.SIZES + (262144 + 777,)
    for i, n in enumerate(sizes):
        p0, g, m0, v0 = R.inputs(n, 100 + i)
        for k in R.STEPS:
            for wd, gscale in R.WD_GSCALE:
                p, opt = _torch_adam(p0, m0, v0, k - 1, wd, torch.float32)
                got = _torch_step(p, opt, (g.astype(np.float64) * gscale).astype(np.float32))
                r = R.check(got, p0, g, m0, v0, k, wd, gscale, what=f"torch fp32, n={n}")
                a = (p0, g, m0, v0, k, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], wd, gscale)
                r["p_acc"] = R.accumulated_p_ratio(got[0], R.reference(*a)[0], R.bounds(*a)[0])
                worst = {q: max(worst[q], r[q]) for q in worst}
    # five steps from zero moments, a fresh gradient each, each step against the reference on the fp32 state before it
    p0, _, _, _ = R.inputs(1025, 7)
    rng = np.random.default_rng(8)
    p, opt = _torch_adam(p0, np.zeros(1025, np.float32), np.zeros(1025, np.float32), 0, 1e-4, torch.float32)
    cur = (p0, np.zeros(1025, np.float32), np.zeros(1025, np.float32))
    for k in range(1, 6):
        gk = R.gradient(1025, rng)
        got = _torch_step(p, opt, gk)
        r = R.check(got, cur[0], gk, cur[1], cur[2], k, 1e-4, 1.0, what="torch fp32 trajectory")
        a = (cur[0], gk, cur[1], cur[2], k, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], 1e-4, 1.0)
        r["p_acc"] = R.accumulated_p_ratio(got[0], R.reference(*a)[0], R.bounds(*a)[0])
        worst = {q: max(worst[q], r[q]) for q in worst}
        cur = got
    print("fp32 torch.optim.Adam vs fp64 reference, largest error/bound: " + ", ".join(f"{q} {worst[q]:.3f}" for q in worst))
    for q in ("m", "v", "p_acc"):
        assert worst[q] <= 0.5, f"{q}: fp32 torch uses {worst[q]:.3f} of the bound, less than 2x room: the derivation is wrong"


def test_bounds_notice_the_mutations_the_gpu_tests_must_catch():
    """No GPU needed to see that the bounds are tight enough: a step without the weight-decay term, with the bias corrections of step 1,
    or applied twice moves p by far more than bound_p on moments of the gradient's scale (step 7, weight decay 1e-4), and an element
    never stepped is far outside all three bounds."""
    p0, g, m0, v0 = R.inputs(1025, 21)
    g = (g * 1e-3).astype(np.float32)        # a family's gradients are small against its weights: that is where wd shows
    m0, v0 = R.moments_like(g, np.random.default_rng(22))
    a = (p0, g, m0, v0, 7, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], 1e-4, 1.0)
    want, bnd = R.reference(*a), R.bounds(*a)
    no_wd = R.reference(p0, g, m0, v0, 7, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], 0.0, 1.0)
    step1 = R.reference(p0, g, m0, v0, 1, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], 1e-4, 1.0)
    twice = R.reference(want[0], g, want[1], want[2], 7, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], 1e-4, 1.0)
    for name, mut in (("no weight decay", no_wd), ("bias corrections of step 1", step1), ("stepped twice", twice)):
        r = R.ratios(mut, want, bnd)
        frac = float(np.mean(np.abs(mut[0] - want[0]) > bnd[0]))
        print(f"{name}: p off by up to {r['p']:.3g} x bound, {100 * frac:.1f} % of the elements beyond it")
        assert r["p"] > 100.0, name          # one element beyond its bound turns a GPU test red: they assert every element
    never = R.ratios((p0, m0, v0), want, bnd)
    assert never["p"] > 1e3 and never["m"] > 1e3 and never["v"] > 1e3
