"""The DVGTformer oracle (tests/dvgtformer_oracle.py) against outputs of the reference itself (tests/golden/dvgtformer_*.npz, written by
tests/golden/make_golden_dvgtformer.py running the reference on the CPU, dropout 0): X behind the input stage, both Pearson graphs, the
encoder output, the prediction in train and eval mode, the loss, every parameter gradient, the positional-encoding constant, a
finite-difference check of the hand-written backward, the torch restatement, the dropout masks and the reference's own training curve
with the oracle's gradients and fp64 Adam (tests/adam_reference.py)."""
import functools
import json
import os

import numpy as np
import pytest

import adam_reference as AR
import grad_gate as GG
import dvgtformer_oracle as O
import family_kit as K
from family_kit import GOLD, rel_same_shape as rel

SMALL = ["dvgtformer_small_3x4_h1_b1_bs3", "dvgtformer_small_5x7_h2_b2_bs4"]
FULL = ["dvgtformer_fdgeom_bs3", "dvgtformer_ncmapssgeom_bs3"]
CURVE = "dvgtformer_train_curve_5x7_bs8"
RTOL = 5e-4          # the family's starting gradient gate (AGCN_TF's, tests/test_agcntf_gpu.py); the oracle stays far inside
TAPS = ("x0", "enc", "a_temp", "a_spat")


def seeded_state(cfg, seed):
    from gnn_rul_benchmarking_amd.dvgtformer import DVGTformer_model
    return K.seeded_state(DVGTformer_model, cfg, seed)


@functools.lru_cache(maxsize=None)
def load_case(name, prefix="sd:"):
    """(fixture, cfg, state dict): the stored one, or -- full geometry -- rebuilt from the seed and held to the stored checksum."""
    z = np.load(os.path.join(GOLD, name + ".npz"))
    cfg = json.loads(str(z["cfg_json"]))
    sd = {k[len(prefix):]: z[k] for k in z.files if k.startswith(prefix)}
    if not sd:
        sd = seeded_state(cfg, int(z["seed"]))
        flat = np.concatenate([sd[k].astype(np.float64).ravel() for k in O.param_names(cfg)])
        assert np.allclose([flat.sum(), (flat * flat).sum()], z["checksum"], rtol=1e-12, atol=0), "rebuilt weights differ from the fixture's"
    return z, cfg, sd


@functools.lru_cache(maxsize=None)
def oracle_of(name):
    z, cfg, sd = load_case(name)
    return O.forward_backward(sd, z["x"], z["y"], cfg)


@pytest.mark.parametrize("name", SMALL + FULL)
def test_forward_taps_and_loss_match_reference(name):
    z, cfg, sd = load_case(name)
    assert list(sd) == O.param_names(cfg) and {k: tuple(v.shape) for k, v in sd.items()} == O.param_shapes(cfg)
    o = oracle_of(name)
    for tap in TAPS:
        assert rel(o[tap], z["tap:" + tap]) < 1e-6, (tap, rel(o[tap], z["tap:" + tap]))
    assert rel(o["pred"], z["pred"].reshape(-1)) < 1e-6 and rel(o["pred"], z["pred_eval"].reshape(-1)) < 1e-6     # dropout off: train = eval
    assert abs(o["loss"] - float(z["loss"])) < 1e-6 * abs(float(z["loss"]))
    assert np.isfinite(z["tap:a_temp"]).all() and np.isfinite(z["tap:a_spat"]).all()


@pytest.mark.parametrize("name", SMALL)
def test_gradients_match_reference(name):
    z, cfg, sd = load_case(name)
    g = oracle_of(name)["grads"]
    ref32 = {k: z["refgrad:" + k] for k in O.param_names(cfg)}
    zero = GG.zero_in_exact_arithmetic(g, ref32)
    assert zero == sorted(k for k in O.param_names(cfg) if "linears_K_" in k and k.endswith(".bias"))
    assert len(zero) == 2 * cfg["num_blocks"] * cfg["num_heads"]
    gmax = max(np.abs(v).max() for v in g.values())
    for k in O.param_names(cfg):
        assert g[k].shape == ref32[k].shape, k
        if k in zero:
            assert np.abs(ref32[k]).max() < 1e-6 * gmax, k
            continue
        ratio, where = GG.gate(ref32[k], g[k], RTOL, GG.floor_for(g[k], g[k]))
        assert ratio <= 1.0, (k, ratio, where)
        assert rel(ref32[k], g[k]) < 1e-4, k


@pytest.mark.parametrize("name", SMALL + FULL)
def test_positional_encoding_constant(name):
    z, cfg, _ = load_case(name)
    pe = O.positional_encoding(cfg["time_length"] + 1, cfg["num_nodes"] + 1)
    assert np.array_equal(pe.astype(np.float32), z["pe"])
    if cfg["num_nodes"] % 2 == 0:                       # an even N leaves the last column untouched
        assert not pe[:, -1].any()
    assert pe[:, 0].any() and np.array_equal(pe[0, 1::2][:cfg["num_nodes"] // 2], np.ones(cfg["num_nodes"] // 2))


@pytest.mark.parametrize("lam", [0.0, 0.5, 1.0])
def test_backward_finite_difference(lam):
    z, cfg, sd = load_case(SMALL[1])
    cfg = dict(cfg, lambda_param=lam)
    sd = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    rng = np.random.default_rng(0)
    g = O.forward_backward(sd, z["x"], z["y"], cfg)["grads"]
    gmax = max(np.abs(v).max() for v in g.values())
    for k in O.param_names(cfg):
        idx = tuple(rng.integers(0, s) for s in sd[k].shape)
        eps = 1e-6
        q = {m: v.copy() for m, v in sd.items()}
        q[k][idx] += eps
        lp = O.forward_backward(q, z["x"], z["y"], cfg, want_grads=False)["loss"]
        q[k][idx] -= 2 * eps
        lm = O.forward_backward(q, z["x"], z["y"], cfg, want_grads=False)["loss"]
        fd = (lp - lm) / (2 * eps)
        assert abs(fd - g[k][idx]) < 1e-5 * abs(fd) + 1e-8 * gmax, (k, idx, fd, g[k][idx])


def test_dropout_masks_enter_forward_and_backward_and_torch_restatement_equals_the_oracle():
    import torch
    z, cfg, sd = load_case(SMALL[1])
    bs = z["x"].shape[0]
    keep = O.keep_masks(bs, cfg, 1234, 1, 0.3)
    assert len(keep) == cfg["num_blocks"] and keep[0].shape == (bs, cfg["time_length"] + 1, cfg["num_nodes"] + 1)
    assert not np.array_equal(keep[0], keep[1]) and all(0.5 < k.mean() < 0.9 for k in keep)
    assert np.array_equal(keep[0], O.keep_masks(bs, cfg, 1234, 1, 0.3)[0]) and not np.array_equal(keep[0], O.keep_masks(bs, cfg, 1234, 2, 0.3)[0])
    assert np.array_equal(O.keep_masks(2, cfg, 1234, 1, 0.3, sample_offset=2)[1], keep[1][2:])           # masks go by global sample index
    o = O.forward_backward(sd, z["x"], z["y"], cfg, keep=keep, dropout_p=0.3)
    assert rel(o["pred"], oracle_of(SMALL[1])["pred"]) > 1e-3
    pred, loss_t, gt = O.torch_grads(sd, z["x"], z["y"], cfg, torch.float64, keep, 0.3)
    assert rel(o["pred"], pred) < 1e-10 and abs(o["loss"] - loss_t) < 1e-10 * o["loss"]
    gmax = max(np.abs(v).max() for v in gt.values())
    for k in O.param_names(cfg):
        assert np.abs(o["grads"][k] - gt[k]).max() < 1e-9 * max(np.abs(gt[k]).max(), 1e-6 * gmax), k


def test_constant_input_row_gives_nan():
    z, cfg, sd = load_case(SMALL[0])
    sd = dict(sd)
    sd["t_v"] = np.full_like(sd["t_v"], 0.25)                               # the appended row [t_v | x_v[L]] becomes constant: 0 / 0
    sd["x_v"] = sd["x_v"].copy()
    sd["x_v"][0, -1, 0] = 0.25
    assert np.isnan(O.forward_backward(sd, z["x"], None, cfg)["pred"]).all()


def test_training_curve_matches_reference():
    """Twenty steps of the oracle's gradients + fp64 Adam against the reference's own DVGTformer.update."""
    z, cfg, sd = load_case(CURVE, "sd0:")
    sd = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    names = O.param_names(cfg)
    m = {k: np.zeros_like(sd[k]) for k in names}
    v = {k: np.zeros_like(sd[k]) for k in names}
    losses = []
    for s in range(len(z["losses"])):
        o = O.forward_backward(sd, z["xs"][s], z["ys"][s], cfg)
        losses.append(o["loss"])
        for k in names:
            sd[k], m[k], v[k] = AR.reference(sd[k], o["grads"][k], m[k], v[k], s + 1, float(z["lr"]), 0.9, 0.999, 1e-8, float(z["wd"]), 1.0)
    assert len(losses) == 20 and np.abs(np.asarray(losses) / z["losses"] - 1).max() < 1e-4
    assert rel(O.forward_backward(sd, z["xs"][0], None, cfg)["pred"], z["eval_pred_end"].reshape(-1)) < 1e-3
