"""Deterministic synthetic datasets shared by make_golden.py (reference side) and the tests."""
import numpy as np


def synthetic_phm2012(seed, n_train, n_test):
    """Deterministic PHM2012-shaped vibration snapshots [n, 2560] with a learnable degradation target.
    The tests regenerate exactly this from the seed instead of storing megabytes of noise."""
    rng = np.random.default_rng(seed)
    def make(n):
        life = rng.uniform(0.05, 1.0, n)                               # label: RUL / max_rul
        t = np.arange(2560)[None, :] / 2560.0
        x = (1.2 - life)[:, None] * np.sin(2 * np.pi * (40 + 25 * (1 - life))[:, None] * t) \
            + 0.4 * rng.standard_normal((n, 2560)) * (1.3 - life)[:, None]
        return x.astype(np.float32), life.astype(np.float32)
    return make(n_train), make(n_test)


def uniform_windows(seed, shape, lo=0.0, hi=1.0):
    """Uniform values in [lo, hi): what the makers of the C-MAPSS-shaped families draw with torch.rand."""
    rng = np.random.default_rng(seed)
    return (rng.random(shape) * (hi - lo) + lo).astype(np.float32)


def vibration_signal(seed, bs, n):
    """The three-tone-plus-noise snapshots of make_golden_sagcn.py::signal / tests/test_sagcn_gpu.py::signal (SAGCN, AGCN_TF)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)[None, :]
    x = np.zeros((bs, n))
    for _ in range(3):
        fr = rng.uniform(0.02, 0.45, (bs, 1))
        x += rng.uniform(0.1, 0.5, (bs, 1)) * np.sin(2 * np.pi * fr * t + rng.uniform(0, 6.28, (bs, 1)))
    return (x + 0.2 * rng.standard_normal((bs, n))).astype(np.float32)


def modulated_signal(seed, bs, n):
    """The four amplitude-modulated tones plus noise of make_golden_stnet.py::signal (STNet: node weights on both sides of 0.7)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)[None, :]
    x = np.zeros((bs, n))
    for _ in range(4):
        fr = rng.uniform(0.02, 0.45, (bs, 1))
        amp = rng.uniform(0.0, 1.2, (bs, 1)) * (0.4 + 0.6 * np.sin(2 * np.pi * t / n * rng.integers(1, 6)) ** 2)
        x += amp * np.sin(2 * np.pi * fr * t + rng.uniform(0, 6.28, (bs, 1)))
    return (x + 0.3 * rng.standard_normal((bs, n))).astype(np.float32)


def drifting_windows(seed, bs, N, L):
    """The drifting sensors in [0, 1] of make_golden_stagnn.py::windows (STAGNN: a mixed-sign adjacency)."""
    rng = np.random.default_rng(seed)
    t = np.linspace(0, 1, L)[None, None, :]
    slope = rng.uniform(-0.5, 0.5, (bs, N, 1))
    x = 0.5 + slope * (t - 0.5) + 0.08 * rng.standard_normal((bs, N, L))
    return np.clip(x, 0, 1).astype(np.float32)


def seeded_input(kind, seed, shape, lo=0.0, hi=1.0):
    """The input of a fixture that stores ``x_seed`` / ``x_kind`` / ``x_shape`` (/ ``x_lo``, ``x_hi``) instead of ``x``."""
    shape = tuple(int(v) for v in shape)
    if kind == "uniform":
        return uniform_windows(seed, shape, lo, hi)
    if kind == "vibration":
        return vibration_signal(seed, shape[0], int(np.prod(shape[1:]))).reshape(shape)
    if kind == "modulated":
        return modulated_signal(seed, shape[0], int(np.prod(shape[1:]))).reshape(shape)
    if kind == "drifting":
        return drifting_windows(seed, *shape)
    raise ValueError(kind)


class Fixture:
    """A golden .npz as np.load gives it (``files``, ``[key]``, ``in``), with ``"x"`` filled in where the file holds a seed instead of
    the array: regenerated once by seeded_input and held to the stored fp64 sum ``x_checksum`` to 1e-6."""

    def __init__(self, path):
        self._z = np.load(path)
        self.seeded = "x_seed" in self._z.files
        self.files = list(self._z.files) + (["x"] if self.seeded else [])
        self._x = None

    def __contains__(self, k):
        return k in self.files

    def __getitem__(self, k):
        if k != "x" or not self.seeded:
            return self._z[k]
        if self._x is None:
            z = self._z
            x = seeded_input(str(z["x_kind"]), int(z["x_seed"]), z["x_shape"], float(z["x_lo"]), float(z["x_hi"]))
            assert abs(x.astype(np.float64).sum() - float(z["x_checksum"])) < 1e-6, "the regenerated input is not the one the reference ran on"
            x.setflags(write=False)
            self._x = x
        return self._x



def synthetic_cmapss(seed, n_train, n_test, window=50, sensors=14):
    """Deterministic C-MAPSS-shaped windows in the reference's on-disk layout [n, window, sensors], values in [0, 1]
    (min-max scaled sensors), label RUL / max_rul in [0, 1]: sensors drift with degradation plus noise."""
    rng = np.random.default_rng(seed)
    slope = rng.uniform(-0.4, 0.4, sensors)

    def make(n):
        life = rng.uniform(0.0, 1.0, n)
        t = np.linspace(0.0, 1.0, window)[None, :, None]
        base = 0.5 + slope[None, None, :] * (1.0 - life)[:, None, None] * (0.7 + 0.3 * t)
        x = np.clip(base + 0.05 * rng.standard_normal((n, window, sensors)), 0.0, 1.0)
        return x.astype(np.float32), life.astype(np.float32)
    return make(n_train), make(n_test)
