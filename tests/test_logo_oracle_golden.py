"""The LOGO oracle (tests/logo_oracle.py) against outputs of the reference itself (tests/golden/logo_*.npz, written by
tests/golden/make_golden_logo.py running the reference on the CPU, dropouts 0): the graph stage's output, the temporal stack's output,
the prediction in train and eval mode, L_GL, the loss, every parameter gradient element by element (tests/grad_gate.py), a
finite-difference check of the hand-written backward including the theta * L_GL term, the torch restatement, and the reference's own
twelve-step training curve with the oracle's gradients and fp64 Adam (tests/adam_reference.py)."""
import numpy as np
import pytest

import adam_reference as AR
import grad_gate as GG
import logo_oracle as O
from family_kit import load_case, rel_same_shape as rel

CASES = ["logo_small_3x2x2_h1_bs4", "logo_fd001geom_bs5", "logo_fd002geom_bs4", "logo_ncmapssgeom_bs3"]
CURVE = "logo_train_curve_3x2x2_h1_bs8"
RTOL = 5e-4          # the family's gradient gate (tests/test_logo_gpu.py); the oracle stays far inside


@pytest.mark.parametrize("name", CASES)
def test_forward_and_gradients_match_reference(name):
    z, cfg, sd = load_case(name)
    assert list(sd) == O.state_keys() and len(sd) == 46
    assert {k: tuple(v.shape) for k, v in sd.items()} == O.param_shapes(cfg)
    bs = z["x"].shape[0]
    assert 2 * int(((z["fc1_pre"] > 0).any(1) & (z["fc2_pre"] > 0).any(1)).sum()) >= bs           # the maker's condition
    theta = float(z["theta"])
    loss, g, fw = O.loss_and_grads(sd, z["x"], z["y"], cfg, theta)
    for tap in ("mpnn", "lstm"):
        assert rel(fw[tap], z[tap]) < 1e-6, (tap, rel(fw[tap], z[tap]))
    assert rel(fw["pred"], z["pred"]) < 1e-6 and rel(fw["pred"], z["pred_eval"]) < 1e-6          # dropouts are off: train = eval
    assert abs(fw["gl"] - float(z["loss_gl"])) < 1e-6 * abs(float(z["loss_gl"]))
    assert abs(loss - float(z["loss"])) < 1e-6 * abs(float(z["loss"]))
    ref32 = {k: z["refgrad:" + k] for k in O.param_names()}
    assert GG.zero_in_exact_arithmetic(g, ref32) == []                                          # all 46 tensors receive a gradient
    for k in O.param_names():
        assert g[k].shape == ref32[k].shape, k
        # the reference's fp32 gradient against the fp64 oracle under the gate the kernels face; the floor is grad_gate's for a reference
        # without noise of its own: MARGIN fp32 ulps of the tensor's largest element
        ratio, where = GG.gate(ref32[k], g[k], RTOL, GG.floor_for(g[k], g[k]))
        assert ratio <= 1.0, (k, ratio, where)
        assert rel(ref32[k], g[k]) < 1e-4, k


@pytest.mark.parametrize("theta", [0.0, 0.01, 1.0])
def test_backward_finite_difference(theta):
    """Every tensor, the graph stage's in particular, with and without the theta * L_GL term."""
    z, cfg, sd = load_case(CASES[0])
    sd = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    rng = np.random.default_rng(0)
    loss, g, _ = O.loss_and_grads(sd, z["x"], z["y"], cfg, theta)
    for k in O.param_names():
        for _ in range(2):
            idx = tuple(rng.integers(0, s) for s in sd[k].shape)
            eps = 1e-6
            q = {m: v.copy() for m, v in sd.items()}
            q[k][idx] += eps
            lp = O.loss_and_grads(q, z["x"], z["y"], cfg, theta)[0]
            q[k][idx] -= 2 * eps
            lm = O.loss_and_grads(q, z["x"], z["y"], cfg, theta)[0]
            fd = (lp - lm) / (2 * eps)
            assert abs(fd - g[k][idx]) < 1e-5 * max(abs(fd), 1e-4) + 1e-9, (k, idx, fd, g[k][idx])


def test_graph_stage_gradient_of_the_gl_term_alone():
    """theta * L_GL reaches only the graph stage: its gradient is the difference of two oracle gradients, checked against autograd."""
    import torch
    z, cfg, sd = load_case(CASES[1])
    _, g1, _ = O.loss_and_grads(sd, z["x"], z["y"], cfg, 1.0)
    _, g0, _ = O.loss_and_grads(sd, z["x"], z["y"], cfg, 0.0)
    pt = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in sd.items()}
    _, gl = O.torch_forward(pt, torch.tensor(z["x"].astype(np.float64)), cfg)
    names = [k for k in O.param_names() if k.startswith(("nonlin_map", "graph_attn_blk"))]
    auto = torch.autograd.grad(gl, [pt[k] for k in names])
    for k, a in zip(names, auto):
        assert rel(g1[k] - g0[k], a.numpy()) < 1e-8, k
    for k in O.param_names():
        if k not in names:
            assert np.array_equal(g1[k], g0[k]) or rel(g1[k], g0[k]) < 1e-12, k


def test_dropout_masks_enter_forward_and_backward_and_torch_restatement_equals_the_oracle():
    import torch
    z, cfg, sd = load_case(CASES[0])
    bs, Q, h = z["x"].shape[0], cfg["num_patch"] * cfg["num_nodes"], cfg["hidden_dim"]
    rng = np.random.default_rng(1)
    keep = tuple((rng.uniform(size=(Q, bs, W)) >= 0.2).astype(np.float64) for W in (6 * h, 3 * h))
    loss, g, fw = O.loss_and_grads(sd, z["x"], z["y"], cfg, 0.01, keep_mask=keep)
    assert rel(fw["pred"], O.forward(sd, z["x"], cfg)["pred"]) > 1e-3
    pred, loss_t, gt = O.torch_grads(sd, z["x"], z["y"], cfg, 0.01, torch.float64, keep_scale=tuple(k / 0.8 for k in keep))
    assert rel(fw["pred"], pred) < 1e-10 and abs(loss - loss_t) < 1e-10 * loss
    for k in O.param_names():
        assert rel(g[k], gt[k]) < 1e-8, k
    m = O.keep_masks(bs, cfg, 1234, 1)
    assert m[0].shape == (Q, bs, 6 * h) and m[1].shape == (Q, bs, 3 * h) and not np.array_equal(m[0][..., :3 * h], m[1])
    assert np.array_equal(m[0], O.keep_masks(bs, cfg, 1234, 1)[0]) and not np.array_equal(m[0], O.keep_masks(bs, cfg, 1234, 2)[0])


def test_constant_sensor_gives_nan_everywhere_in_the_batch():
    z, cfg, sd = load_case(CASES[0])
    x = z["x"].copy()
    x[1, 0, :] = 0.25
    fw = O.forward(sd, x, cfg)
    assert np.isnan(fw["pred"]).all() and np.isnan(fw["gl"])


def test_batch_coupling():
    """The recurrence runs along the batch: the halves of a batch do not reproduce the whole batch's predictions."""
    z, cfg, sd = load_case(CASES[1])
    x = z["x"][:4]
    whole = O.forward(sd, x, cfg)["pred"]
    halves = np.concatenate([O.forward(sd, x[:2], cfg)["pred"], O.forward(sd, x[2:], cfg)["pred"]])
    assert rel(halves, whole) > 1e-5


def test_training_curve_matches_reference():
    """Twelve steps of the oracle's gradients + fp64 Adam against the reference's own LOGO.update (no scheduler step)."""
    z, cfg, sd = load_case(CURVE, "sd0:")
    sd = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    names = O.param_names()
    m = {k: np.zeros_like(sd[k]) for k in names}
    v = {k: np.zeros_like(sd[k]) for k in names}
    losses = []
    for s in range(len(z["losses"])):
        loss, g, _ = O.loss_and_grads(sd, z["xs"][s], z["ys"][s], cfg, float(z["theta"]))
        losses.append(loss)
        for k in names:
            sd[k], m[k], v[k] = AR.reference(sd[k], g[k], m[k], v[k], s + 1, float(z["lr"]), 0.9, 0.999, 1e-8, float(z["wd"]), 1.0)
    assert len(losses) == 12 and np.abs(np.asarray(losses) / z["losses"] - 1).max() < 1e-5
    for k in names:
        assert rel(sd[k], z["sd_end:" + k]) < 2e-4, k
    assert rel(O.forward(sd, z["xs"][0], cfg)["pred"], z["eval_pred_end"]) < 1e-4
