"""torch.optim.Adam's element update in numpy fp64, the rounding-error bounds an fp32 implementation of it must meet, and the input
generators of the optimizer tests (tests/test_adam_reference_cpu.py, test_adam_kernels_gpu.py, test_fused_adam_families_gpu.py).

The update (csrc/adam_device.hpp: adam_value; L2 weight decay folded into the gradient, bias-corrected, no amsgrad):

    gt = wd * p0 + g * gscale
    m  = b1 * m0 + (1 - b1) * gt
    v  = b2 * v0 + (1 - b2) * gt^2
    p  = p0 - lr / (1 - b1^k) * m / (sqrt(v) / sqrt(1 - b2^k) + eps)

The C ABI takes the hyper-parameters as ``float``: the reference rounds them to fp32 first and computes in fp64 from there, so that
``1 - beta`` is exact in both (Sterbenz: beta in [0.5, 1]) and the comparison sees the kernels' arithmetic, not the fp32 image of 0.9.

Error bounds
------------
``bounds`` returns, per element, the largest absolute error of m, v and p that fp32 arithmetic with correctly rounded + - * / sqrt can
leave, from the operation count of ``adam_value``; u = 2^-24 is the unit roundoff, A = |wd * p0| + |g * gscale| the magnitude sum behind
gt (so a cancelling gt is covered: its error is relative to A, not to gt).

  gt:  one product and one fma                                   2 roundings, each <= u A
  m:   (1 - b1) * gt rounds once more, the fma once (u |m|, and |m| <= |b1 m0| + (1 - b1) A)
         -> |error| <= u (|b1 m0| + (1 - b1) A) + 3 u (1 - b1) A            <= 4 u (|b1 m0| + (1 - b1) A)
  v:   gt^2 carries 2 * 2u A^2, the two products of (1 - b2) * gt * gt one rounding each, the fma one (u v)
         -> |error| <= 6 u (1 - b2) A^2 + u (b2 v0 + (1 - b2) A^2)            <= 7 u (b2 v0 + (1 - b2) A^2)
  delta = lr/bc1 * m / (sqrt(v) / sqrt(bc2) + eps):  the two bias-correction constants are rounded to fp32 (2), sqrt, its product with
       1/sqrt(bc2), the sum with eps, the quotient and the product with lr/bc1 round once each (5): 7 roundings relative to delta;
       the error of m enters divided by the denominator, the relative error of v halved (sqrt) and never amplified (eps >= 0)
  p:   the subtraction rounds once, u |p|

The worst-case counts are therefore 4u for m, 7u for v and 7u for delta, each relative to the magnitudes above.  The bounds use the one
constant 8u for all three: a factor 2 over the count for m, 8/7 for v and for delta.  Contraction to fma only removes roundings, and
the counts add every rounding at its full size with the same sign and charge gt's two roundings even where they vanish (wd = 0 and a
power-of-two gscale make gt exact), so an implementation stays well inside them: see the measured use below.

    bound_m = 8u (|b1 m0| + (1 - b1) A)
    bound_v = 8u (b2 v0 + (1 - b2) A^2)
    bound_p = (lr/bc1) / denom * bound_m + |delta| (bound_v / (2 v) + 8u) + u |p|

with denom, delta, v and p the reference's.  The constants are derived, not measured; tests/test_adam_reference_cpu.py shows that an
independent fp32 implementation (torch.optim.Adam on the CPU) uses less than half of bound_m, of bound_v and of the accumulated part of
bound_p (``accumulated_p_ratio``) -- 0.31, 0.47 and 0.19; the HIP kernels use 0.33 and 0.57 of the first two.  bound_p as a whole has no
such room and cannot have: its last term, the single rounding of the result, is sharp and is reached by any implementation (0.997).
Second-order terms (u^2) are dropped: they are 2^-24 of the bound.

Below the normal range (|x| < 2^-126) a result is rounded to a multiple of 2^-149: each operation then adds at most 2^-150 in absolute
terms instead of u |x|.  With the 8 operations budgeted above that is 8 * 2^-150 = 5.6e-45 on bound_m and bound_v, and through bound_v's
term on bound_p.  The generators below keep every input, and with them every intermediate, above 1e-30 in magnitude or exactly zero, so
the term is idle in the kernel tests; a model's own gradient (tests/test_fused_adam_families_gpu.py) may hold an element whose square
underflows.
"""
import numpy as np

U = 2.0 ** -24
UNDERFLOW = 8 * 2.0 ** -150       # see "Below the normal range" in the module docstring
DEFAULT = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)


def f32(x):
    """A hyper-parameter as the C ABI's ``float`` sees it (a Python float again)."""
    return float(np.float32(x))


def _terms(p0, g, m0, v0, k, lr, beta1, beta2, eps, wd, gscale):
    p0, g, m0, v0 = (np.asarray(a, dtype=np.float64) for a in (p0, g, m0, v0))
    lr, b1, b2, eps, wd, gscale = (f32(a) for a in (lr, beta1, beta2, eps, wd, gscale))
    k = int(k)
    bc1, bc2 = 1.0 - b1 ** k, 1.0 - b2 ** k
    gt = wd * p0 + g * gscale
    m = b1 * m0 + (1.0 - b1) * gt
    v = b2 * v0 + (1.0 - b2) * gt * gt
    denom = np.sqrt(v) / np.sqrt(bc2) + eps
    delta = lr / bc1 * m / denom
    return dict(p0=p0, g=g, m0=m0, v0=v0, b1=b1, b2=b2, wd=wd, gscale=gscale, step=lr / bc1, m=m, v=v, denom=denom, delta=delta,
                p=p0 - delta)


def reference(p0, g, m0, v0, k, lr, beta1, beta2, eps, wd, gscale):
    """(p, m, v) after Adam step ``k`` (1-based) in fp64."""
    t = _terms(p0, g, m0, v0, k, lr, beta1, beta2, eps, wd, gscale)
    return t["p"], t["m"], t["v"]


def bounds(p0, g, m0, v0, k, lr, beta1, beta2, eps, wd, gscale):
    """(bound_p, bound_m, bound_v): per-element absolute error bounds of an fp32 step against ``reference`` (derivation: module
    docstring).  An element whose reference is not finite (a NaN / Inf gradient) gets NaN bounds: the caller checks those separately."""
    t = _terms(p0, g, m0, v0, k, lr, beta1, beta2, eps, wd, gscale)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        A = np.abs(t["wd"] * t["p0"]) + np.abs(t["g"] * t["gscale"])
        bound_m = 8 * U * (np.abs(t["b1"] * t["m0"]) + (1.0 - t["b1"]) * A)
        bound_v = 8 * U * (t["b2"] * t["v0"] + (1.0 - t["b2"]) * A * A)
        # all operands zero: v is exactly zero and sqrt exact; v == 0 < bound_v (gt cancelled exactly) bounds nothing (inf)
        rel_v = np.where(bound_v == 0.0, 0.0, (bound_v + UNDERFLOW) / (2.0 * t["v"]))
        bound_m, bound_v = np.where(bound_m == 0.0, 0.0, bound_m + UNDERFLOW), np.where(bound_v == 0.0, 0.0, bound_v + UNDERFLOW)
        bound_p = t["step"] / t["denom"] * bound_m + np.abs(t["delta"]) * (rel_v + 8 * U) + U * np.abs(t["p"])
    return bound_p, bound_m, bound_v


def ratios(got, want, bnd):
    """max |got - want| / bound over the elements with a finite reference, for (p, m, v): {'p': .., 'm': .., 'v': ..}.  0 / 0 counts as
    0, an error over a zero bound as inf, a non-finite result where the reference is finite as inf."""
    out = {}
    for name, a, w, b in zip("pmv", got, want, bnd):
        a, w, b = (np.asarray(t, dtype=np.float64) for t in (a, w, b))
        ok = np.isfinite(w)
        with np.errstate(invalid="ignore", divide="ignore"):
            err = np.abs(a[ok] - w[ok])
            r = np.where(err == 0.0, 0.0, err / b[ok])
        r = np.where(np.isfinite(a[ok]), r, np.inf)
        out[name] = float(r.max()) if r.size else 0.0
    return out


def accumulated_p_ratio(got_p, want_p, bound_p):
    """The share of bound_p's ACCUMULATED part that p's error uses: max (|error| - u |p|)+ / (bound_p - u |p|).  The last term of
    bound_p is one rounding of the result, which is sharp -- a p just above a power of two that lands midway between two floats is
    off by u |p| however it was computed -- so "room" against bound_p can only be asked of the rest."""
    got_p, want_p, bound_p = (np.asarray(t, dtype=np.float64) for t in (got_p, want_p, bound_p))
    last = U * np.abs(want_p)
    over = np.maximum(np.abs(got_p - want_p) - last, 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(over == 0.0, 0.0, over / (bound_p - last))
    return float(r.max()) if r.size else 0.0


def check(got, p0, g, m0, v0, k, wd=0.0, gscale=1.0, what="", hp=DEFAULT):
    """Assert (p, m, v) ``got`` within ``bounds`` of ``reference`` on every element; returns the error/bound ratios."""
    args = (p0, g, m0, v0, k, hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], wd, gscale)
    r = ratios(got, reference(*args), bounds(*args))
    for name in "pmv":
        assert r[name] <= 1.0, f"{what}: {name} is {r[name]:.3g} x its error bound (step {k}, wd {wd}, gscale {gscale})"
    return r


# ---- inputs ------------------------------------------------------------------------------------------
TINY = 1e-12        # smallest non-zero |gradient| the generators emit: g^2 (1 - b2) >= 1e-27 stays normal in fp32


def moments_like(g, rng):
    """Moments on the gradient's own scale, which is what makes beta, the bias corrections and weight decay visible in the update:
    exp_avg = (a permutation of g) * U(-1, 1), exp_avg_sq = (that permutation)^2 * U(0.5, 2), as fp32.  |U(-1, 1)| is kept above
    1e-3 so that no moment leaves the normal range."""
    g = np.asarray(g, dtype=np.float32).astype(np.float64)
    gp = g[rng.permutation(g.size)]
    s = rng.uniform(-1.0, 1.0, g.size)
    s = np.where(np.abs(s) < 1e-3, np.copysign(1e-3, s), s)
    m0 = (gp * s).astype(np.float32)
    v0 = (gp * gp * rng.uniform(0.5, 2.0, g.size)).astype(np.float32)
    return m0, v0


def gradient(n, rng):
    """N(0, 1) * 10^U(-9, 3) per element, 1 % exact zeros, fp32; non-zero magnitudes floored at TINY."""
    g = rng.standard_normal(n) * 10.0 ** rng.uniform(-9.0, 3.0, n)
    g = np.where(np.abs(g) < TINY, np.copysign(TINY, g), g)
    g[rng.uniform(size=n) < 0.01] = 0.0
    return g.astype(np.float32)


def inputs(n, seed):
    """(p, g, m0, v0) as fp32 arrays of length n."""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n).astype(np.float32)
    g = gradient(n, rng)
    m0, v0 = moments_like(g, rng)
    for a in (p, g, m0, v0):
        nz = np.abs(a[a != 0])
        assert np.isfinite(a).all() and (nz.size == 0 or nz.min() > 1e-30)
    return p, g, m0, v0


# the cases both the CPU self-check and the GPU kernel tests run: sizes, steps and (weight decay, gradient scale) pairs
SIZES = (1, 2, 3, 4, 5, 7, 8, 255, 256, 257, 1023, 1024, 1025)
STEPS = (1, 2, 10, 1000, 100000)
WD_GSCALE = ((0.0, 1.0), (1e-4, 1.0), (0.1, 0.125))
