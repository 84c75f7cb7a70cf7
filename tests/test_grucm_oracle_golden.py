"""The GRU_CM oracle (tests/grucm_oracle.py) against fixtures produced by running the reference (tests/golden/make_golden_grucm.py):
eval prediction, train prediction, loss, every gradient, the reference's own GRU_CM.update for 12 steps; the numpy code against its
torch restatement through autograd; and the hash dropout masks.  Tolerances: those of tests/test_stgnn_oracle_golden.py."""
import glob
import os

import numpy as np
import pytest
import torch

import grucm_oracle as O
from golden_io import load_npz

GOLD = os.path.join(os.path.dirname(__file__), "golden")
CASES = sorted(p for p in glob.glob(os.path.join(GOLD, "grucm_*x*_bs*.npz")) if "curve" not in p)


def load(path):
    z = load_npz(path)
    cfg = {k[4:]: int(z[k]) for k in z.files if k.startswith("cfg:")}
    p = {k[3:]: z[k].astype(np.float64) for k in z.files if k.startswith("sd:")}
    return z, cfg, p


def test_fixtures_cover_the_wirings_and_an_odd_shape():
    shapes = {(load(p)[1]["num_nodes"], load(p)[1]["time_length"], load(p)[1]["gru_hidden_dim"]) for p in CASES}
    assert {(14, 50, 64), (20, 50, 64)} <= shapes and len(shapes) >= 3


@pytest.mark.parametrize("path", CASES, ids=[os.path.basename(p)[:-4] for p in CASES])
def test_oracle_matches_reference_forward_and_gradients(path):
    z, cfg, p = load(path)
    x, y = z["x"].astype(np.float64), z["y"].astype(np.float64)
    assert np.allclose(O.forward(x, p), z["eval_pred"], rtol=1e-4, atol=1e-6)
    loss, grads, out, _ = O.forward_backward(x, y, p)
    assert np.allclose(out, z["pred"], rtol=1e-4, atol=1e-6)
    assert abs(loss - float(z["loss"])) <= 1e-5 * abs(float(z["loss"]))
    for k in O.param_names():
        g = z["grad:" + k]
        assert np.allclose(grads[k].reshape(g.shape), g, rtol=2e-3, atol=1e-6 + 1e-4 * np.abs(g).max()), k


def test_oracle_follows_the_reference_training_curve():
    z = np.load(os.path.join(GOLD, "grucm_train_curve_14x50_bs16.npz"))
    p = {k[len("sd0:model."):]: z[k].astype(np.float64) for k in z.files if k.startswith("sd0:model.")}
    state, losses = {}, []
    for s in range(z["xs"].shape[0]):
        loss, grads, _, _ = O.forward_backward(z["xs"][s].astype(np.float64), z["ys"][s].astype(np.float64), p)
        losses.append(loss)
        O.adam_step(p, grads, state, float(z["lr"]), float(z["wd"]))
    assert np.allclose(losses, z["losses"], rtol=2e-3)
    for k in O.param_names():
        assert np.allclose(p[k], z["sd_end:model." + k], rtol=1e-3, atol=2e-4), k
    assert np.allclose(O.forward(z["xs"][0].astype(np.float64), p), z["eval_pred_end"], rtol=1e-3, atol=1e-4)


@pytest.mark.parametrize("rates", [(0.0, 0.0, 0.0), (0.2, 0.2, 0.2), (0.1, 0.3, 0.5)])
def test_numpy_oracle_matches_its_torch_restatement_through_autograd(rates):
    z, cfg, p = load(os.path.join(GOLD, "grucm_odd_9x21_bs6.npz"))
    x, y = z["x"].astype(np.float64), z["y"].astype(np.float64)
    N, L, H = cfg["num_nodes"], cfg["time_length"], cfg["gru_hidden_dim"]
    keep = O.masks(x.shape[0], N, L, H, 31, 4, rates, sample_offset=3)
    loss, grads, out, _ = O.forward_backward(x, y, p, keep)
    m = O.torch_model(L, N, H, torch.float64)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()})
    pred = m(torch.from_numpy(x), [torch.from_numpy(k) for k in keep])
    tl = torch.nn.functional.mse_loss(pred, torch.from_numpy(y))
    tl.backward()
    assert np.allclose(out, pred.detach().numpy(), rtol=1e-10, atol=1e-12)
    assert abs(loss - tl.item()) <= 1e-10 * abs(tl.item())
    tg = {k: v.grad.numpy() for k, v in m.named_parameters()}
    for k in O.param_names():
        assert np.allclose(grads[k].reshape(tg[k].shape), tg[k], rtol=1e-8, atol=1e-12 + 1e-9 * np.abs(tg[k]).max()), k


def test_dropout_masks_are_deterministic_shard_consistent_and_keep_the_rate():
    bs, N, L, H, p = 100, 14, 50, 64, 0.2                     # the FD004 tensor sizes at the reference protocol's batch
    a = O.masks(bs, N, L, H, 9, 3, (p, p, p))
    b = O.masks(bs, N, L, H, 9, 3, (p, p, p))
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    for other in (O.masks(bs, N, L, H, 10, 3, (p, p, p)), O.masks(bs, N, L, H, 9, 4, (p, p, p))):
        assert all(not np.array_equal(u, v) for u, v in zip(a, other))
    assert not np.array_equal(a[0], a[1])                     # the sites draw from different keys
    tail = O.masks(bs - 40, N, L, H, 9, 3, (p, p, p), sample_offset=40)
    assert all(np.array_equal(u[40:], v) for u, v in zip(a, tail))
    for m in a:
        assert set(np.unique(m)) == {0.0, 1.0 / (1.0 - p)}
        n = m.size
        assert abs((m > 0).mean() - (1.0 - p)) < 3.0 * np.sqrt(p * (1.0 - p) / n)
    assert all((m == 1.0).all() for m in O.masks(4, N, L, H, 9, 3))
