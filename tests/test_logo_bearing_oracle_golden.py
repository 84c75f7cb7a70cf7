"""The LOGO_bearing oracle (tests/logo_bearing_oracle.py: an fp64 STFT magnitude in front of tests/logo_oracle.py) against outputs of the
reference itself (tests/golden/logob_*.npz, written by tests/golden/make_golden_logo_bearing.py running the reference on the CPU,
dropouts 0), at the bars of tests/test_logo_oracle_golden.py: the spectrogram ``torch.stft`` returned inside the reference's forward,
the graph stage's and the temporal stack's outputs, the prediction in train and eval mode, L_GL, the loss, every parameter gradient
element by element, the torch restatement, and the reference's own 28-step training curve -- whose MultiStepLR steps once per update --
with the oracle's gradients and fp64 Adam at the recorded learning rates."""
import functools
import glob
import os

import numpy as np
import pytest

import adam_reference as AR
import grad_gate as GG
import family_kit as K
import logo_bearing_oracle as O
from family_kit import GOLD, rel_same_shape as rel
from test_logo_oracle_golden import RTOL

SMALL = ["logob_tiny_ns4_p8_t2_h1_bs3", "logob_ns2_p6_t3_h1_bs2", "logob_ragged_ns4_p10_t3_h2_bs2", "logob_onepatch_ns4_p8_t1_h1_bs2"]
FULL = ["logob_phm2012_full_bs2", "logob_xjtu_full_bs2"]
CASES = SMALL + FULL
CURVE = "logob_train_curve_ns4_p8_t2_h1_bs4"


def seeded_state(cfg, seed):
    from gnn_rul_benchmarking_amd.logo_bearing import LOGO_bearing_model
    return K.seeded_state(LOGO_bearing_model, cfg, seed, O.KEYS)


@functools.lru_cache(maxsize=None)
def load_case(name, prefix="sd:"):
    """(arrays of every part of the fixture, cfg, weights); the full-width cases store no weights: rebuilt from the recorded seed.
    Cached and never modified."""
    z = {}
    for path in [os.path.join(GOLD, name + ".npz")] + sorted(glob.glob(os.path.join(GOLD, name + ".p*.npz"))):
        with np.load(path) as part:
            z.update({k: part[k] for k in part.files})
    cfg = {k[4:]: int(z[k]) for k in z if k.startswith("cfg:")}
    sd = {k[len(prefix):]: z[k] for k in z if k.startswith(prefix)}
    return z, cfg, sd or seeded_state(cfg, int(z["seed"]))


def fusion_is_constant(cfg):
    """At two nodes a row of A_T and of C has one entry off the diagonal, and a softmax over one live entry is 1 whatever the logit: C is
    a constant, L_GL is exactly 1 and the twelve fusion tensors have a zero gradient in exact arithmetic."""
    return sorted(k for k in O.param_names() if k.startswith("graph_attn_blk.")) if cfg["num_nodes"] == 2 else []


@functools.lru_cache(maxsize=None)
def fixture_oracle(name):
    z, cfg, sd = load_case(name)
    loss, g, fw = O.loss_and_grads(sd, z["x"], z["y"], cfg, float(z["theta"]))
    return z, cfg, sd, loss, g, fw


@pytest.mark.parametrize("name", CASES)
def test_stft_restatement_matches_the_reference_spectrogram(name):
    z, cfg, _ = load_case(name)
    N, f = O.stft_shape(cfg)
    assert (N, f) == (cfg["num_nodes"], cfg["input_dim"]) and z["spec"].shape == (z["x"].shape[0], cfg["num_patch"], N, f)
    mag = O.stft_mag(z["x"], cfg)
    assert rel(mag, z["spec"]) < 1e-6, rel(mag, z["spec"])
    import torch
    w = O.torch_window(torch.tensor(z["x"], dtype=torch.float64), cfg).numpy()
    assert rel(O.window(z["x"], cfg), w) < 1e-12 and w.shape == (z["x"].shape[0], N, cfg["num_patch"] * f)


@pytest.mark.parametrize("name", CASES)
def test_forward_and_gradients_match_reference(name):
    z, cfg, sd, loss, g, fw = fixture_oracle(name)
    assert list(sd) == O.state_keys() and len(sd) == 46
    assert {k: tuple(v.shape) for k, v in sd.items()} == O.param_shapes(cfg)
    bs = z["x"].shape[0]
    assert 2 * int(((z["fc1_pre"] > 0).any(1) & (z["fc2_pre"] > 0).any(1)).sum()) >= bs           # the maker's condition
    for tap in ("mpnn", "lstm"):
        assert rel(fw[tap], z[tap]) < 1e-6, (tap, rel(fw[tap], z[tap]))
    assert rel(fw["pred"], z["pred"]) < 1e-6 and rel(fw["pred"], z["pred_eval"]) < 1e-6          # dropouts are off: train = eval
    assert abs(fw["gl"] - float(z["loss_gl"])) < 1e-6 * abs(float(z["loss_gl"]))
    assert abs(loss - float(z["loss"])) < 1e-6 * abs(float(z["loss"]))
    ref32 = {k: z["refgrad:" + k] for k in O.param_names()}
    zero = GG.zero_in_exact_arithmetic(g, ref32)
    assert zero == fusion_is_constant(cfg)                                                      # every other tensor receives a gradient
    for k in O.param_names():
        assert g[k].shape == ref32[k].shape, k
        if k in zero:
            continue
        ratio, where = GG.gate(ref32[k], g[k], RTOL, GG.floor_for(g[k], g[k]))
        assert ratio <= 1.0, (k, ratio, where)
        assert rel(ref32[k], g[k]) < 1e-4, k


def test_torch_restatement_equals_the_oracle():
    import torch
    z, cfg, sd, loss, g, fw = fixture_oracle(SMALL[2])
    pred, loss_t, gt = O.torch_grads(sd, z["x"], z["y"], cfg, float(z["theta"]), torch.float64)
    assert rel(fw["pred"], pred) < 1e-10 and abs(loss - loss_t) < 1e-10 * loss
    for k in O.param_names():
        assert rel(g[k], gt[k]) < 1e-8, k


def test_training_curve_matches_reference_with_the_scheduler_stepped_per_update():
    """28 steps of the oracle's gradients + fp64 Adam at the rate MultiStepLR([5, 10, 20, 25], 0.5) gives when stepped once per update,
    against the reference's own LOGO_bearing.update; the recorded rates are those."""
    z, cfg, sd = load_case(CURVE, "sd0:")
    sd = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    names = O.param_names()
    lr0 = float(z["lr"])
    want_lrs = [lr0 * 0.5 ** sum(s + 1 >= ms for ms in (5, 10, 20, 25)) for s in range(28)]        # behind update s + 1
    assert np.allclose(z["lrs"], want_lrs, rtol=1e-12, atol=0) and z["lrs"][-1] == lr0 / 16
    m = {k: np.zeros_like(sd[k]) for k in names}
    v = {k: np.zeros_like(sd[k]) for k in names}
    losses = []
    for s in range(len(z["losses"])):
        loss, g, _ = O.loss_and_grads(sd, z["xs"][s], z["ys"][s], cfg, float(z["theta"]))
        losses.append(loss)
        lr = lr0 if s == 0 else float(z["lrs"][s - 1])                 # update s + 1 runs at the rate the previous updates left
        for k in names:
            sd[k], m[k], v[k] = AR.reference(sd[k], g[k], m[k], v[k], s + 1, lr, 0.9, 0.999, 1e-8, float(z["wd"]), 1.0)
    assert len(losses) == 28 and np.abs(np.asarray(losses) / z["losses"] - 1).max() < 1e-5
    for k in names:
        assert rel(sd[k], z["sd_end:" + k]) < 2e-4, k
    assert rel(O.forward(sd, z["xs"][0], cfg)["pred"], z["eval_pred_end"]) < 1e-4
