"""The HierCorrPool oracle (tests/hiercorrpool_oracle.py) against outputs of the reference itself (tests/golden/hiercorrpool_*.npz,
written by tests/golden/make_golden_hiercorrpool.py running the reference on the CPU, dropout 0): the encoder output, X', A', H, the
prediction, the loss, the BatchNorm buffers after the forward, every parameter gradient element by element (tests/grad_gate.py), and
the reference's own twelve-step training curve with the oracle's gradients and fp64 Adam (tests/adam_reference.py)."""
import numpy as np
import pytest

import adam_reference as AR
import grad_gate as GG
import hiercorrpool_oracle as O
from family_kit import load_case, rel_same_shape as rel

CASES = ["hiercorrpool_small_7x3_n5_bs6", "hiercorrpool_fd001geom_bs4", "hiercorrpool_fd004geom_bs4", "hiercorrpool_ncmapssgeom_bs3"]
CURVE = "hiercorrpool_train_curve_7x3_n5_bs8"
RTOL = 5e-4          # the family's gradient gate (tests/test_hiercorrpool_gpu.py); the oracle stays far inside


@pytest.mark.parametrize("name", CASES)
def test_forward_and_gradients_match_reference(name):
    z, cfg, sd = load_case(name)
    assert list(sd) == O.state_keys()
    bs = z["x"].shape[0]
    assert 2 * int((z["fc1_pre"] > 0).sum()) >= bs           # the maker's condition: the final leaky ReLU is open on half the samples
    loss, g, fw = O.loss_and_grads(sd, z["x"], z["y"], cfg)
    assert fw["encoder"].shape[1] == O.lengths(cfg["num_patch"])[-1]
    for tap in ("encoder", "pooled_x", "pooled_adj", "H"):
        assert rel(fw[tap], z[tap]) < 1e-6, tap
    assert rel(fw["pred"], z["pred"]) < 1e-6
    assert abs(loss - float(z["loss"])) < 1e-6 * abs(float(z["loss"]))
    after = O.running_after(sd, fw)
    for k, v in after.items():
        assert rel(v, z["bn_after:" + k]) < 1e-6, k
    for l in (1, 2, 3):
        assert int(z["bn_after:" + O.ENC.format(l) + "1.num_batches_tracked"]) == 1
    ref32 = {k: z["refgrad:" + k] for k in O.param_names()}
    assert GG.zero_in_exact_arithmetic(g, ref32) == [O.ZERO_GRAD]
    gmax = max(np.abs(v).max() for v in g.values())
    assert np.abs(g[O.ZERO_GRAD]).max() <= 1e-12 * gmax and np.abs(ref32[O.ZERO_GRAD]).max() <= 1e-5 * gmax
    for k in O.param_names():
        if k == O.ZERO_GRAD:
            continue
        assert g[k].shape == ref32[k].shape, k
        # the reference's fp32 gradient against the fp64 oracle under the gate the kernels face; the floor is grad_gate's for a reference
        # without noise of its own: MARGIN fp32 ulps of the tensor's largest element
        ratio, where = GG.gate(ref32[k], g[k], RTOL, GG.floor_for(g[k], g[k]))
        assert ratio <= 1.0, (k, ratio, where)
        assert rel(ref32[k], g[k]) < 1e-4, k


def test_backward_finite_difference():
    z, cfg, sd = load_case(CASES[0])
    sd = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    rng = np.random.default_rng(0)
    loss, g, _ = O.loss_and_grads(sd, z["x"], z["y"], cfg)
    for k in O.param_names():
        if k == O.ZERO_GRAD:
            continue
        idx = tuple(rng.integers(0, s) for s in sd[k].shape)
        eps = 1e-6
        q = {m: v.copy() for m, v in sd.items()}
        q[k][idx] += eps
        lp = O.loss_and_grads(q, z["x"], z["y"], cfg)[0]
        q[k][idx] -= 2 * eps
        lm = O.loss_and_grads(q, z["x"], z["y"], cfg)[0]
        fd = (lp - lm) / (2 * eps)
        assert abs(fd - g[k][idx]) < 1e-5 * max(abs(fd), 1e-4) + 1e-9, (k, fd, g[k][idx])


def test_dropout_mask_enters_forward_and_backward():
    z, cfg, sd = load_case(CASES[0])
    bs, C1, L1 = z["x"].shape[0], cfg["hidden_dim"] * cfg["num_nodes"], O.lengths(cfg["num_patch"])[0]
    keep = (np.random.default_rng(1).uniform(size=(bs, C1, L1)) >= 0.35).astype(np.float64)
    loss, g, fw = O.loss_and_grads(sd, z["x"], z["y"], cfg, keep_mask=keep)
    pred32, loss32, g32 = O.torch_grads(sd, z["x"], z["y"], cfg, __import__("torch").float64, keep_scale=keep / 0.65)
    assert rel(fw["pred"], pred32) < 1e-10 and abs(loss - loss32) < 1e-10 * loss
    for k in O.param_names():
        if k != O.ZERO_GRAD:
            assert rel(g[k], g32[k]) < 1e-8, k


def test_torch_restatement_equals_the_oracle_in_eval_mode():
    import torch
    z, cfg, sd = load_case(CURVE, "sd_end:")
    fw = O.forward(sd, z["xs"][0], cfg, training=False)
    pt = {k: torch.tensor(np.asarray(v, np.float64)) if v.dtype.kind == "f" else torch.tensor(v) for k, v in sd.items()}
    got = O.torch_forward(pt, torch.tensor(z["xs"][0].astype(np.float64)), cfg, training=False).numpy()
    assert rel(got, fw["pred"]) < 1e-10
    assert rel(fw["pred"], z["eval_pred_end"]) < 1e-5


def test_training_curve_matches_reference():
    """Twelve steps of the oracle's gradients + fp64 Adam against the reference's own HierCorrPool.update."""
    z, cfg, sd = load_case(CURVE, "sd0:")
    sd = {k: np.asarray(v, np.float64) if v.dtype.kind == "f" else v.copy() for k, v in sd.items()}
    names = O.param_names()
    m = {k: np.zeros_like(sd[k]) for k in names}
    v = {k: np.zeros_like(sd[k]) for k in names}
    losses = []
    for s in range(len(z["losses"])):
        loss, g, fw = O.loss_and_grads(sd, z["xs"][s], z["ys"][s], cfg)
        losses.append(loss)
        sd.update(O.running_after(sd, fw))
        for k in names:
            sd[k], m[k], v[k] = AR.reference(sd[k], g[k], m[k], v[k], s + 1, float(z["lr"]), 0.9, 0.999, 1e-8, float(z["wd"]), 1.0)
    assert np.abs(np.asarray(losses) / z["losses"] - 1).max() < 1e-5
    for k in O.state_keys():
        if k.endswith("num_batches_tracked"):
            assert int(z["sd_end:" + k]) == len(losses)
        else:
            assert rel(sd[k], z["sd_end:" + k]) < 2e-4, k
    assert rel(O.forward(sd, z["xs"][0], cfg, training=False)["pred"], z["eval_pred_end"]) < 1e-4
