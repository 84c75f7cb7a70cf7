"""The optimizer entries of include/rulgnn.h alone, element by element against fp64 Adam (tests/adam_reference.py: the reference, its
derived error bounds, the input generator): rulgnn_adam_step_f32, rulgnn_adam_step_guarded_f32, rulgnn_adam_bn_step_f32 and
rulgnn_adam_step_dev_f32 with rulgnn_step_state_set (csrc/optim.hip; reference: torch.optim.Adam as algorithms/algorithms.py:474-478
configures it).

Moments on the gradient's own scale, gradients over twelve decades, steps 1 .. 100 000 and weight decay with a gradient scale: every
term of the update is visible in the result, and every element is held to its own bound.  Sizes and pointer offsets reach every loop
shape of ``adam_range``: the float4 loop with its scalar tail, the scalar loop a misaligned buffer falls back to, a second grid-stride
sweep of each at the 1024 x 256 grid cap, and adam_bn_step's stride of (grid - 1) workgroups.  Each buffer sits between sentinel
floats that must survive the call.

Every test prints the largest error/bound ratio it saw (``pytest -s``), tagged with the path that served it."""
import ctypes as C

import numpy as np
import pytest

import adam_reference as R

pytestmark = pytest.mark.gpu
HP = R.DEFAULT
PAD, SENTINEL = 4, 12345.0        # 16 bytes in front of each buffer: the padding keeps the allocation's alignment
ENTRIES = ("plain", "guarded", "bn", "dev")
BN_L, BN_COUNT, BN_MOM = 1, 1400, 0.1


def _dev():
    import torch
    return torch.device("cuda:0")


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class _Buffers:
    """p, g, m, v on the device, buffer i starting ``offs[i]`` floats behind a 16-byte-aligned address, sentinels around each."""

    def __init__(self, arrays, offs):
        import torch
        self.n, self.offs, self.base, self.view = len(arrays[0]), offs, [], []
        for a, off in zip(arrays, offs):
            base = torch.full((self.n + 2 * PAD + 4,), SENTINEL, dtype=torch.float32, device=_dev())
            assert base.data_ptr() % 16 == 0
            view = base[PAD + off:PAD + off + self.n]
            view.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))
            assert view.data_ptr() % 16 == (4 * off) % 16
            self.base.append(base)
            self.view.append(view)
        self.g0 = np.ascontiguousarray(arrays[1], dtype=np.float32)

    def ptrs(self):
        return [v.data_ptr() for v in self.view]

    def result(self):
        """(p, m, v) as numpy after a device sync; the sentinels and the gradient must be as they were."""
        import torch
        torch.cuda.synchronize()
        for base, off, name in zip(self.base, self.offs, "pgmv"):
            host = base.cpu().numpy()
            outside = np.concatenate([host[:PAD + off], host[PAD + off + self.n:]])
            assert (outside == np.float32(SENTINEL)).all(), f"the call wrote outside {name}[0, n)"
        assert np.array_equal(self.view[1].cpu().numpy().view(np.uint32), self.g0.view(np.uint32)), "the call changed the gradient"
        return tuple(self.view[i].cpu().numpy() for i in (0, 2, 3))


def _bn_block(L=BN_L, seed=3, from_moments=0):
    """(running, batch) in bn_running_entry's layout [2 L modules][mean, var][10]; with ``from_moments`` the second rows hold E[z^2],
    below E[z]^2 on every seventh entry (rounding can leave moments so: the kernel clamps the variance at zero)."""
    rng = np.random.default_rng(seed)
    run = rng.standard_normal((2 * L, 2, 10))
    run[:, 1] = np.abs(run[:, 1]) + 0.1
    bat = rng.standard_normal((2 * L, 2, 10))
    var = rng.uniform(0.01, 2.0, (2 * L, 10))
    if from_moments:
        e2 = bat[:, 0] ** 2 + var
        low = (np.arange(2 * L * 10).reshape(2 * L, 10) % 7) == 3
        e2[low] = 0.5 * bat[:, 0][low] ** 2
        bat[:, 1] = e2
    else:
        bat[:, 1] = var
    return run.astype(np.float32).reshape(-1), bat.astype(np.float32).reshape(-1)


def _bn_reference(run, bat, L, count, mom, from_moments):
    """(want, bound) of the running statistics in fp64: (1 - mom) r + mom b, b the batch mean or count / (count - 1) times the batch
    variance (from moments: max(E[z^2] - E[z]^2, 0)).  Bound from the operations of bn_running_entry, u = 2^-24: ``1 - mom`` (0.1 is
    below 1/2, the difference rounds), its product with r and the sum are 3 roundings on |(1 - mom) r|; m * m, the subtraction, the
    rounded unbias factor, its product, the product with mom and the sum are 6 on mom * unbias * (|E[z^2]| + E[z]^2); 8u on both."""
    mom = R.f32(mom)
    r = run.astype(np.float64).reshape(2 * L, 2, 10)
    b = bat.astype(np.float64).reshape(2 * L, 2, 10).copy()
    mag = np.abs(b)
    unbias = count / (count - 1.0) if count > 1 else 1.0
    if from_moments:
        mag[:, 1] = np.abs(b[:, 1]) + b[:, 0] ** 2
        b[:, 1] = np.maximum(b[:, 1] - b[:, 0] ** 2, 0.0)
    b[:, 1] *= unbias
    mag[:, 1] *= unbias
    want = (1.0 - mom) * r + mom * b
    bound = 8 * R.U * ((1.0 - mom) * np.abs(r) + mom * mag)
    return want.reshape(-1), bound.reshape(-1)


def _launch(entry, arrays, k, wd=0.0, gscale=1.0, offs=(0, 0, 0, 0), guard=0.25, state=None, bn=None, from_moments=0, L=BN_L):
    """One call of ``entry`` as step ``k``; returns (p, m, v) -- for "bn" also the running statistics behind them.  ``state``: a
    device step state to advance ("dev"; None: a fresh one set to k - 1)."""
    import torch
    from gnn_rul_benchmarking_amd import _lib
    lib = _lib.load()
    b = _Buffers(arrays, offs)
    n = b.n
    hp = (HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], wd, gscale)
    keep = []
    if entry == "plain":
        _lib.check(lib.rulgnn_adam_step_f32(*b.ptrs(), n, k, *hp, _stream()), entry)
    elif entry == "guarded":
        gd = torch.tensor([guard], dtype=torch.float32, device=_dev())
        _lib.check(lib.rulgnn_adam_step_guarded_f32(*b.ptrs(), n, k, *hp, gd.data_ptr(), _stream()), entry)
    elif entry == "bn":
        run, bat = bn if bn is not None else _bn_block(L, from_moments=from_moments)
        rd, bd = torch.from_numpy(run.copy()).to(_dev()), torch.from_numpy(bat.copy()).to(_dev())
        gd = None if guard is None else torch.tensor([guard], dtype=torch.float32, device=_dev())
        _lib.check(lib.rulgnn_adam_bn_step_f32(*b.ptrs(), n, k, *hp, rd.data_ptr(), bd.data_ptr(), L, BN_COUNT, BN_MOM, from_moments,
                                               None if gd is None else gd.data_ptr(), _stream()), entry)
        torch.cuda.synchronize()
        assert np.array_equal(bd.cpu().numpy().view(np.uint32), bat.view(np.uint32))
        keep = [rd.cpu().numpy()]
    elif entry == "dev":
        if state is None:
            state = _new_state(k - 1)
        _lib.check(lib.rulgnn_adam_step_dev_f32(*b.ptrs(), n, state.data_ptr(), *hp, _stream()), entry)
    else:
        raise ValueError(entry)
    return b.result() + tuple(keep)


def _new_state(adam_step):
    import torch
    from gnn_rul_benchmarking_amd import _lib
    state = torch.zeros(_lib.STEP_STATE_BYTES, dtype=torch.uint8, device=_dev())
    _lib.check(_lib.load().rulgnn_step_state_set(state.data_ptr(), 0, adam_step, _stream()), "rulgnn_step_state_set")
    return state


def _path(entry, n, offs):
    if entry == "bn":
        return "adam_bn"
    if entry == "dev":
        return "dev-state"
    return "float4" if n >= 4 and not any(offs) else "scalar"


def _report(path, worst):
    print(f"ADAM-RATIO {path}: " + " ".join(f"{q}={worst[q]:.3f}" for q in "pmv"))


def _check_bn(got_bn, from_moments, L=BN_L, bn=None):
    run, bat = bn if bn is not None else _bn_block(L, from_moments=from_moments)
    want, bound = _bn_reference(run, bat, L, BN_COUNT, BN_MOM, from_moments)
    err = np.abs(got_bn.astype(np.float64) - want)
    assert (err <= bound).all(), f"BatchNorm running statistics: {float((err / bound).max()):.3g} x the bound"
    if from_moments:            # the clamped entries: the batch term is exactly zero, what is left is (1 - mom) r, two roundings
        b = bat.astype(np.float64).reshape(2 * L, 2, 10)
        clamped = np.zeros((2 * L, 2, 10), bool)
        clamped[:, 1] = b[:, 1] < b[:, 0] ** 2
        clamped = clamped.reshape(-1)
        assert clamped.sum() >= 2
        kept = (1.0 - R.f32(BN_MOM)) * run.astype(np.float64)[clamped]
        assert (np.abs(got_bn[clamped] - kept) <= 3 * R.U * np.abs(kept)).all(), "a variance below zero was not clamped to zero"
    return float((err / bound).max())


# ---- every entry x every small size x every step and (wd, gscale) --------------------------------------------------------
@pytest.mark.parametrize("n", R.SIZES)
@pytest.mark.parametrize("entry", ENTRIES)
def test_every_entry_is_adam_within_the_rounding_bounds(entry, n):
    arrays = R.inputs(n, 100 + R.SIZES.index(n))
    worst = dict(p=0.0, m=0.0, v=0.0)
    for k in R.STEPS:
        for wd, gscale in R.WD_GSCALE:
            got = _launch(entry, arrays, k, wd, gscale)
            r = R.check(got[:3], *arrays, k, wd, gscale, what=f"{entry}, n={n}")
            worst = {q: max(worst[q], r[q]) for q in worst}
            if entry == "bn":
                _check_bn(got[3], 0)
    _report(_path(entry, n, (0,) * 4), worst)


# ---- the second sweep of each grid-stride loop ------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,n,off", [
    ("plain", 1048576 + 4096 + 3, 0),        # float4 loop: 262 144 threads, 263 168 float4 -> a partly filled second sweep, tail of 3
    ("plain", 262144 + 777, 1),              # scalar loop (misaligned): a partly filled second sweep
    ("guarded", 262144 + 777, 3),
    ("bn", 300000, 0),                       # adam_bn_step, stride (grid - 1) * 256 = 262 144: the float4 loop in ONE sweep (75 000 float4)
    ("bn", 300000, 1),                       # ... misaligned: the scalar loop, a partly filled second sweep
    ("bn", 1048576 + 4096 + 3, 0),           # ... the float4 loop's second sweep at that stride, and the scalar tail
    ("dev", 262144 + 777, 0),
])
def test_second_grid_stride_sweep(entry, n, off):
    arrays = R.inputs(n, 7 + off)
    offs = (off,) * 4
    got = _launch(entry, arrays, 10, 1e-4, 1.0, offs=offs)
    r = R.check(got[:3], *arrays, 10, 1e-4, 1.0, what=f"{entry}, n={n}, offset {off}")
    _report(_path(entry, n, offs), r)


# ---- alignment: the float4 path and the scalar path are one function ----------------------------------------------------------
@pytest.mark.parametrize("offs", [(0, 0, 0, 0), (1, 1, 1, 1), (2, 2, 2, 2), (3, 3, 3, 3), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0),
                                  (0, 0, 0, 1)], ids=lambda o: "".join(map(str, o)))
@pytest.mark.parametrize("entry", ["plain", "bn"])
def test_alignment_changes_the_path_not_the_result(entry, offs):
    """All four buffers offset together (3 floats: STNet's optimized range), and each of p, g, m, v alone: within the bounds, and
    bit for bit what the aligned call gives (optim.hip: "the same arithmetic per element either way")."""
    worst = dict(p=0.0, m=0.0, v=0.0)
    for n in (5, 257, 1025):
        arrays = R.inputs(n, 40 + n)
        got = _launch(entry, arrays, 10, 0.1, 0.125, offs=offs)
        r = R.check(got[:3], *arrays, 10, 0.1, 0.125, what=f"{entry}, n={n}, offsets {offs}")
        worst = {q: max(worst[q], r[q]) for q in worst}
        aligned = _launch(entry, arrays, 10, 0.1, 0.125)
        for a, b, name in zip(got[:3], aligned[:3], "pmv"):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{name} differs between offsets {offs} and an aligned call"
    _report(_path(entry, 1025, offs), worst)


# ---- five steps from zero moments, a fresh gradient each ------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_five_steps_from_zero_moments(entry):
    n = 1027
    p0, _, _, _ = R.inputs(n, 7)
    rng = np.random.default_rng(8)
    cur = (p0, np.zeros(n, np.float32), np.zeros(n, np.float32))
    state = _new_state(0) if entry == "dev" else None
    worst = dict(p=0.0, m=0.0, v=0.0)
    for k in range(1, 6):
        g = R.gradient(n, rng)
        got = _launch(entry, (cur[0], g, cur[1], cur[2]), k, 1e-4, 1.0, state=state)
        r = R.check(got[:3], cur[0], g, cur[1], cur[2], k, 1e-4, 1.0, what=f"{entry}, step {k} from zero moments")
        worst = {q: max(worst[q], r[q]) for q in worst}
        cur = got[:3]
    _report(_path(entry, n, (0,) * 4), worst)


# ---- the device step state ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k0", [0, 9, 999])
def test_device_step_state_counts_the_steps(k0):
    """rulgnn_step_state_set(state, 0, k0), then three rulgnn_adam_step_dev_f32 calls: steps k0 + 1 .. k0 + 3, the bias corrections
    computed on the device (step_prepare_adam_kernel)."""
    n = 1025
    p, g, m, v = R.inputs(n, 60 + k0)
    rng = np.random.default_rng(61 + k0)
    state = _new_state(k0)
    worst = dict(p=0.0, m=0.0, v=0.0)
    for k in (k0 + 1, k0 + 2, k0 + 3):
        got = _launch("dev", (p, g, m, v), k, 1e-4, 1.0, state=state)
        r = R.check(got, p, g, m, v, k, 1e-4, 1.0, what=f"device step state set to {k0}, step {k}")
        worst = {q: max(worst[q], r[q]) for q in worst}
        p, m, v = got
        g = R.gradient(n, rng)
    _report("dev-state", worst)


# ---- exact cases ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_zero_gradient_and_moments_without_decay_change_nothing(entry):
    for n, offs in ((1025, (0,) * 4), (259, (1,) * 4)):
        p0 = R.inputs(n, 5)[0]
        z = np.zeros(n, np.float32)
        p, m, v = _launch(entry, (p0, z, z, z), 3, 0.0, 1.0, offs=offs)[:3]
        assert np.array_equal(p.view(np.uint32), p0.view(np.uint32))
        assert np.array_equal(m.view(np.uint32), z.view(np.uint32)) and np.array_equal(v.view(np.uint32), z.view(np.uint32))


@pytest.mark.parametrize("guard", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "-inf"])
@pytest.mark.parametrize("entry", ["guarded", "bn"])
def test_a_non_finite_guard_leaves_everything_bit_unchanged(entry, guard):
    for n, offs in ((1025, (0,) * 4), (259, (3,) * 4)):
        arrays = R.inputs(n, 9)
        bn = _bn_block(from_moments=1)
        got = _launch(entry, arrays, 4, 1e-4, 1.0, offs=offs, guard=guard, bn=bn, from_moments=1)
        for a, b, name in zip(got[:3], (arrays[0], arrays[2], arrays[3]), "pmv"):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
        if entry == "bn":
            assert np.array_equal(got[3].view(np.uint32), bn[0].view(np.uint32))


@pytest.mark.parametrize("entry,guard", [("guarded", 0.0), ("guarded", -1.0), ("guarded", 1e30), ("bn", 0.0), ("bn", -1.0), ("bn", 1e30),
                                         ("bn", None)])
def test_a_finite_guard_applies_the_step(entry, guard):
    """(``None``: adam_bn_step's guard pointer is optional.)"""
    arrays = R.inputs(1025, 9)
    got = _launch(entry, arrays, 4, 1e-4, 1.0, guard=guard, from_moments=1)
    r = R.check(got[:3], *arrays, 4, 1e-4, 1.0, what=f"{entry}, guard {guard}")
    if entry == "bn":
        _check_bn(got[3], 1)
    _report(_path(entry, 1025, (0,) * 4), r)


# ---- the BatchNorm half of adam_bn_step ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("from_moments", [0, 1])
@pytest.mark.parametrize("L", [1, 2, 8])
def test_adam_bn_step_running_statistics(L, from_moments):
    """The last workgroup's work against fp64: (1 - mom) r + mom b, b = var * count / (count - 1) for variances, the variance from
    moments clamped at zero; the Adam elements beside it within their bounds (n = 1083: float4 loop plus a tail of 3)."""
    arrays = R.inputs(1083, 70 + L)
    bn = _bn_block(L, seed=10 + L, from_moments=from_moments)
    got = _launch("bn", arrays, 3, 1e-4, 1.0, bn=bn, from_moments=from_moments, L=L, guard=None)
    r = R.check(got[:3], *arrays, 3, 1e-4, 1.0, what=f"adam_bn, L={L}")
    worst = _check_bn(got[3], from_moments, L=L, bn=bn)
    _report("adam_bn", r)
    print(f"BN-RATIO adam_bn L={L} from_moments={from_moments}: {worst:.3f}")


# ---- a NaN or Inf gradient element stays where it is ---------------------------------------------------------------------------
@pytest.mark.parametrize("offs", [(0,) * 4, (1,) * 4], ids=["float4", "scalar"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_a_non_finite_gradient_element_poisons_only_itself(entry, offs):
    n = 259                                            # 64 float4 and a scalar tail of 3
    p, g, m, v = R.inputs(n, 31)
    g = g.copy()
    nan_at = [8, 13, 18, 23, 256]                      # lanes x, y, z, w of a float4, and the tail
    inf_at = [32, 37, 42, 47, 258]
    g[nan_at], g[inf_at] = np.nan, np.inf
    bad = np.zeros(n, bool)
    bad[nan_at + inf_at] = True
    got = _launch(entry, (p, g, m, v), 10, 1e-4, 1.0, offs=offs)[:3]
    for a, name in zip(got, "pmv"):
        assert not np.isfinite(a[bad]).any(), f"{name} of a NaN / Inf gradient element came out finite"
        assert np.isfinite(a[~bad]).all(), f"a NaN / Inf gradient element reached another element's {name}"
    with np.errstate(invalid="ignore", over="ignore"):
        r = R.check(got, p, g, m, v, 10, 1e-4, 1.0, what=f"{entry}, NaN / Inf gradient elements")      # the finite-reference elements
    _report(_path(entry, n, offs), r)
