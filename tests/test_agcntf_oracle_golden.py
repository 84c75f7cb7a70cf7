"""The AGCN_TF oracle (tests/agcntf_oracle.py) against outputs of the reference itself (tests/golden/agcntf_*.npz, written by
tests/golden/make_golden_agcntf.py running the reference on the CPU): the 40 normalised statistics, H (the concatenation in front of the
attention), the attention output, the prediction, the loss and every parameter gradient.  The fixtures with patches longer than 16
points were produced with the reference's unstable argsort pinned to the stable order (make_golden_sagcn.stable_argsort)."""
import os

import numpy as np
import pytest

import agcntf_oracle as O
from test_sagcn_oracle_golden import rel
from golden_io import load_npz

GOLD = os.path.join(os.path.dirname(__file__), "golden")
CASES = ["agcntf_phm_40x64_bs4", "agcntf_small_5x7_bs6", "agcntf_xjtu_like_20x256_bs3"]


def load_case(name):
    z = load_npz(os.path.join(GOLD, name + ".npz"))
    cfg = {k[4:]: int(z[k]) for k in z.files if k.startswith("cfg:")}
    p = {k[3:]: z[k].astype(np.float64) for k in z.files if k.startswith("sd:")}
    return z, cfg, p


@pytest.mark.parametrize("name", CASES)
def test_forward_and_gradients_match_reference(name):
    z, cfg, p = load_case(name)
    P, n, heads = cfg["num_patch"], cfg["patch_size"], cfg.get("num_heads", 1)
    assert bool(z["argsort_pinned_stable"]) == (n > 16)
    assert list(p) == O.param_names(heads) and O.heads_of(p) == heads
    assert {k: v.shape for k, v in p.items()} == O.param_shapes(P, cfg["hidden_adj_dim"], cfg["hidden_gnn_dim"], heads)
    x, y = z["x"].astype(np.float64), z["y"].astype(np.float64)
    loss, g, fw = O.loss_and_grads(p, x, y, P, n)
    assert fw.At.shape == (x.shape[0], P, P) and fw.As.shape == (x.shape[0], 40, 40)      # the oracle does form the adjacencies
    assert rel(fw.feat, z["feat"]) < 1e-4
    assert rel(fw.H, z["H"]) < 1e-4
    assert rel(fw.O, z["attn_out"]) < 1e-4
    assert rel(fw.pred, z["pred"]) < 1e-5
    assert abs(loss - float(z["loss"])) < 1e-5 * abs(float(z["loss"]))
    for k in O.param_names(heads):
        ref = z["grad:" + k]
        assert g[k].shape == ref.shape, k
        if k.endswith("W_k.bias"):
            # analytically zero (the rows of a softmax gradient sum to zero): rounding noise on both sides
            scale = np.abs(z["grad:" + k.replace("W_k", "W_q")]).max()
            assert np.abs(g[k]).max() <= 1e-4 * scale and np.abs(ref).max() <= 1e-4 * scale, k
            continue
        assert rel(g[k], ref) < 1e-4, k


def test_flatten_round_trip():
    p = O.random_params(5, 6, 7, heads=2, seed=3)
    flat = O.flatten(p, 2)
    q = O.unflatten(flat, 5, 6, 7, 2)
    assert list(q) == O.param_names(2) and all(np.array_equal(p[k], q[k]) for k in p)


def test_backward_finite_difference():
    rng = np.random.default_rng(0)
    P, n, Ha, Hg, heads = 4, 10, 6, 5, 2
    p = O.random_params(P, Ha, Hg, heads, seed=1)
    x, y = rng.normal(0, 0.6, (3, P * n)), rng.uniform(0, 1, 3)
    loss, g, fw = O.loss_and_grads(p, x, y, P, n)
    for k in O.param_names(heads):
        if k.endswith("W_k.bias"):
            assert np.abs(g[k]).max() < 1e-12 * max(np.abs(g[k.replace("W_k", "W_q")]).max(), 1e-30) + 1e-15
            continue
        idx = tuple(rng.integers(0, s) for s in p[k].shape)
        eps = 1e-6
        q = {m: v.copy() for m, v in p.items()}
        q[k][idx] += eps
        lp = O.loss_and_grads(q, x, y, P, n)[0]
        q[k][idx] -= 2 * eps
        lm = O.loss_and_grads(q, x, y, P, n)[0]
        fd = (lp - lm) / (2 * eps)
        assert abs(fd - g[k][idx]) < 1e-5 * max(abs(fd), 1e-3) + 1e-9, (k, fd, g[k][idx])


def test_reassociated_aggregation_equals_the_literal_one():
    """A X = U (W2^T X) + 1 (b2^T X)^T -- the identity the kernels rest on -- in float64."""
    p = O.random_params(9, 6, 7, seed=2)
    x = np.random.default_rng(5).normal(0, 0.6, (3, 9 * 8))
    fw = O.forward(p, x, 9, 8)
    X = fw.feat
    Gt = np.einsum("ph,bpf->bhf", p["attention_tem_adj.2.weight"], X)
    Mt = fw.Ut @ Gt + np.einsum("p,bpf->bf", p["attention_tem_adj.2.bias"], X)[:, None, :]
    assert rel(Mt, fw.Mt) < 1e-13
    Gs = np.einsum("jh,bpj->bhp", p["attention_spa_adj.2.weight"], X)
    Ms = fw.Us @ Gs + np.einsum("j,bpj->bp", p["attention_spa_adj.2.bias"], X)[:, None, :]
    assert rel(Ms, fw.Ms) < 1e-13


def test_torch_restatement_equals_the_oracle():
    import torch
    rng = np.random.default_rng(4)
    P, n, Ha, Hg, heads = 6, 12, 5, 8, 2
    p = O.random_params(P, Ha, Hg, heads, seed=7)
    x = rng.normal(0, 0.6, (3, P * n))
    fw = O.forward(p, x, P, n)
    pt = {k: torch.from_numpy(v) for k, v in p.items()}
    got = O.torch_forward(pt, torch.from_numpy(x), P, n, heads).numpy()
    # float64 on both sides; the cumulative columns c / sqrt|c| amplify the last-bit differences of two ways to write a statistic by up
    # to 1 / sqrt|c| near a zero crossing of a running sum (|c| is clamped at 1e-12), so far less than eps^-1/2 ~ 1e8 of headroom is used
    assert rel(got, fw.pred) < 1e-6
