"""A per-element gate for gradients against an fp64 reference (pure numpy; imports nothing from the package).

The GPU tests compare gradients in the max-norm of a whole tensor, max|got - ref| / max|ref| < GTOL with GTOL = 5e-4..2e-3.  Under
that form an element smaller than GTOL times the tensor's largest element may be 100 % wrong, and in these models most elements of
most tensors are that small (tests/golden/grad_noise.json and tests/test_grad_gate_cpu.py hold the shares).  The gate here holds
every element to

    |got_e - g64_e| <= rtol * |g64_e| + floor_abs

where ``rtol`` is the family's existing gate, now applied to the element's own magnitude, and ``floor_abs`` is measured on the
REFERENCE, never on the code under test: ``floor_for`` takes the error of the reference's own fp32 autograd on this tensor and this
input (the fixture's ``grad:`` entry against the fp64 oracle) times a margin of 16.  The margin: the kernels sum in other orders than
torch (split-K, tree and fp64-atomic reductions), some products run on split operands of the 2^-22-per-operand class (4 fp32 ulps),
and another 4x is headroom.  A tensor on which the reference happened to be exact is floored at one fp32 ulp of its largest element,
so that nothing is held to better than fp32."""
import numpy as np

MARGIN = 16
ZERO_REL = 1e-9          # a tensor whose fp64 gradient is below this share of the model's largest gradient is zero in exact arithmetic


def _pair(a, g64):
    a, b = np.asarray(a, np.float64), np.asarray(g64, np.float64)
    if a.shape != b.shape:
        raise ValueError(f"shape mismatch: {a.shape} against the fp64 gradient's {b.shape}")
    return a, b


def noise(ref32, g64):
    """max_e |ref32_e - g64_e|: what the reference's own fp32 autograd does to this tensor on this input."""
    a, b = _pair(ref32, g64)
    return float(np.abs(a - b).max()) if b.size else 0.0


def gate(got, g64, rtol, floor_abs):
    """The largest |got_e - g64_e| / (rtol |g64_e| + floor_abs) and the index (a tuple into g64's shape) where it occurs.  <= 1 passes.
    A non-finite element of ``got`` gives inf at its index."""
    a, b = _pair(got, g64)
    if not floor_abs > 0:
        raise ValueError("floor_abs must be positive")
    r = np.abs(a - b) / (rtol * np.abs(b) + floor_abs)
    r = np.where(np.isfinite(a), r, np.inf)
    i = int(np.argmax(r.reshape(-1)))
    return float(r.reshape(-1)[i]), tuple(int(v) for v in np.unravel_index(i, b.shape))


def floor_for(ref32, g64, margin=MARGIN):
    """margin * max(noise of the reference's fp32 gradient, one fp32 ulp (2^-23) of the tensor's largest element)."""
    b = np.asarray(g64, np.float64)
    return float(margin * max(noise(ref32, g64), 2.0 ** -23 * np.abs(b).max()))


def zero_in_exact_arithmetic(g64, ref32):
    """Names of the tensors whose gradient is zero in exact arithmetic, detected, not listed: the fp64 gradient is at most 1e-9 of the
    model's largest, or the fixture holds no reference gradient for the name (``ref32`` lacks it or maps it to None).  The reference
    and the kernels hold rounding residue there, which has no magnitude of its own to be relative to; those tensors stay under each
    family's existing rule."""
    gmax = max(float(np.abs(np.asarray(v, np.float64)).max()) for v in g64.values())
    return sorted(k for k, v in g64.items()
                  if ref32.get(k) is None or float(np.abs(np.asarray(v, np.float64)).max()) <= ZERO_REL * gmax)


def over_gate(got, g64, rtol, floor_abs):
    """Boolean mask of the elements over the gate: for telling a row, a column or a trailing range from a spread."""
    a, b = _pair(got, g64)
    return ~(np.abs(a - b) <= rtol * np.abs(b) + floor_abs)
