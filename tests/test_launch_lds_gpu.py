"""The opt-in to more than 48 KB of dynamic LDS is per kernel (csrc/launch.hpp: allow_dynamic_lds), not per pointer type (GPU).

Kernels that differ only in template arguments share their pointer type: sgemm_planes_kernel<4> / <5>, the four operand layouts of
sgemm_f16x2v_kernel.  Each of them must work whichever kernel of its group a process launches first, so every case below runs in a fresh
child process (the state under test is per process) and the groups are walked in both orders."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def planes_products(order):
    """rulgnn_sgemm_scaled_ws_f32 at 800 x 8192 x 32 (800 = 5 x 160, no multiple of 128: sgemm_planes_kernel<5>, 160 tiles, 156 KB of LDS)
    and at 512 x 8192 x 32 (<4>, 128 tiles, 144 KB); `used_planes` == 1 says that the pre-split kernel ran, not a fallback."""
    from test_sgemm_gpu import run_scaled_ws
    shapes = [(800, 8192, 32), (512, 8192, 32)]
    for M, N, K in (shapes if order == "forward" else shapes[::-1]):
        rng = np.random.default_rng(M + N + K)
        A = rng.standard_normal((M, K)).astype(np.float32)
        B = rng.standard_normal((N, K)).astype(np.float32)
        ref = A.astype(np.float64) @ B.astype(np.float64).T
        got, used = run_scaled_ws(A, B, M, N, K, "k", "k")
        err, bound = np.abs(got - ref).max(), 2e-6 * np.sqrt(K) * np.abs(ref).max() + 1e-6    # test_presplit_product_tile_forms_and_short_k
        print(f"planes M={M} used_planes={used} err={err:.3e} bound={bound:.3e}", flush=True)
        assert used == 1
        assert err < bound


def wide_scaled_products(order):
    """rulgnn_sgemm_scaled_f32 at 2560 x 4096 x 64, the smallest product of 160 tiles of 256 x 256 (sgemm_wide_ok), in the default GEMM
    mode: sgemm_f16x2v_kernel in each of its four (A, B) operand layouts, 96 KB of LDS."""
    from test_sgemm_gpu import run_scaled
    M, N, K = 2560, 4096, 64
    rng = np.random.default_rng(M + N + K)
    A = rng.standard_normal((M, K)).astype(np.float32)
    B = rng.standard_normal((N, K)).astype(np.float32)
    ref = A.astype(np.float64) @ B.astype(np.float64).T
    layouts = [("k", "k"), ("k", "r"), ("r", "k"), ("r", "r")]
    for a_layout, b_layout in (layouts if order == "forward" else layouts[::-1]):
        got, pa, pb = run_scaled(A, B, M, N, K, a_layout, b_layout)
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print(f"wide {a_layout}{b_layout} err={err:.3e}", flush=True)
        assert pa.max() == np.abs(A).max() and pb.max() == np.abs(B).max()
        assert err < 4e-6                                            # test_two_plane_f16_split_with_operand_scales
        assert np.isfinite(got).all()


CASES = {"planes": planes_products, "wide": wide_scaled_products}


@pytest.mark.parametrize("order", ["forward", "reverse"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_each_kernel_of_a_pointer_type_group_gets_its_lds(case, order):
    res = subprocess.run([sys.executable, os.path.abspath(__file__), case, order], capture_output=True, text=True, timeout=180)
    print(res.stdout)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]


if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(HERE), HERE]
    CASES[sys.argv[1]](sys.argv[2])
