"""The fp64 GDAGDL oracle (tests/gdagdl_oracle.py) against what the reference itself produced on the CPU
(tests/golden/make_golden_gdagdl.py): forward, taps and both loss terms at 1e-6, the hand-written backward against the reference's fp32
autograd within that autograd's own noise, the torch restatement against both, and the dropout masks' kept share."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import gdagdl_oracle as O
from family_kit import rel, seeded_state

SMALL = ["gdagdl_small_n3_t3_bs4", "gdagdl_small_n5_t2_bs3"]
FULL = ["gdagdl_phmc1geom_bs2", "gdagdl_phmc3geom_bs2", "gdagdl_xjtugeom_bs2"]
CURVE = "gdagdl_train_curve_n5_t2_bs8"
FWD_TOL = 1e-6            # the bar the other oracles are pinned at (relative to the largest element)

_cache = {}


def seeded_weights(cfg, seed):
    """The maker's weights: the constructor's under the seed (the package's module draws in the reference's order), moved by the
    recorded perturbation."""
    from gnn_rul_benchmarking_amd.gdagdl import GDAGDL_model
    return seeded_state(GDAGDL_model, cfg, seed)


def load_case(name):
    """(npz, cfg, weights name -> fp32 array); cached and never modified."""
    if name not in _cache:
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        cfg = json.loads(str(z["cfg_json"]))
        if name in SMALL:
            P = {k: z["sd:" + k] for k in O.param_names(cfg)}
        else:
            P = seeded_weights(cfg, int(z["seed"]))
            flat = np.concatenate([P[k].astype(np.float64).ravel() for k in O.param_names(cfg)])
            assert np.allclose([flat.sum(), (flat * flat).sum()], z["checksum"], rtol=1e-12, atol=0)
        _cache[name] = (z, cfg, P)
    return _cache[name]


def oracle_run(name):
    """The fp64 oracle's forward + backward of a fixture (train mode, dropout off), computed once."""
    key = ("run", name)
    if key not in _cache:
        z, cfg, P = load_case(name)
        _cache[key] = O.forward_backward(P, z["x"], z["y"], cfg)
    return _cache[key]


@pytest.mark.parametrize("name", SMALL + FULL)
def test_forward_taps_and_losses(name):
    z, cfg, P = load_case(name)
    o = oracle_run(name)
    assert rel(o["pred"], z["pred"]) < FWD_TOL and rel(o["pred"], z["pred_eval"]) < FWD_TOL      # dropout off: train == eval
    assert abs(o["mse"] - float(z["mse"])) < FWD_TOL * max(1.0, float(z["mse"]))
    assert abs(o["recon"] - float(z["recon"])) < FWD_TOL * max(1.0, float(z["recon"]))
    assert abs(o["loss"] - float(z["loss"])) < FWD_TOL * max(1.0, float(z["loss"]))
    assert np.array_equal(o["mask"], z["tap:mask"])                                   # every node: the maker's margin makes it so
    nan = np.isnan(z["tap:ni"])
    assert np.array_equal(np.isnan(o["ni"]), nan) and nan.reshape(-1, cfg["num_nodes"])[3].all() and nan.sum() == cfg["num_nodes"]
    assert rel(o["ni"][~nan], z["tap:ni"][~nan]) < 1e-5                               # a quotient of fp32 norms: the reference's own rounding
    for k in ("mag", "yo", "H"):
        if "tap:" + k in z.files:
            assert rel(o[k], z["tap:" + k]) < FWD_TOL, k


@pytest.mark.parametrize("name", SMALL + FULL)
def test_graph_kinds_and_mask_margin(name):
    """What the maker asserts, read back from the fixture: graphs 0..3 are all-live, one-live, some-live and the zero patch; every node of
    every other graph holds the mask margin on the oracle's own dot product."""
    z, cfg, P = load_case(name)
    N = cfg["num_nodes"]
    live = z["tap:mask"].reshape(-1, N).sum(-1)
    assert live[0] == N and live[1] == 1 and 1 < live[2] < N and live[3] == 0
    assert not z["x"].reshape(-1, cfg["patch_size"])[3].any()
    mag = O.stft_mag(z["x"], cfg)
    ni, m, pcc, lin = O.graph_mask(mag, P["node_importance_linear.weight"].astype(np.float64), P["node_importance_linear.bias"].astype(np.float64))
    ok = np.abs(ni) >= float(z["margin"]) * (np.abs(pcc) * np.abs(lin)[:, None, :]).sum(-1)
    assert ok[~np.isnan(ni)].all()
    assert np.isfinite(z["pred"]).all()


@pytest.mark.parametrize("name", SMALL + FULL)
def test_backward_against_the_reference_within_its_own_noise(name):
    """Every reference gradient the fixture holds (all 34 on the small cases, the small tensors on the full ones) against the
    hand-written fp64 backward: the error is the reference's fp32 autograd noise, measured by the torch restatement in fp32 against
    itself in fp64 (margin 16, floored at one fp32 ulp of the tensor's largest element)."""
    z, cfg, P = load_case(name)
    g64 = oracle_run(name)["grads"]
    assert sorted(g64) == sorted(n for n in O.param_names(cfg) if n not in O.GRADLESS) and len(g64) == len(O.param_names(cfg)) - 2
    _, _, _, t64 = O.torch_grads(P, z["x"], z["y"], cfg, torch.float64)
    _, _, _, t32 = O.torch_grads(P, z["x"], z["y"], cfg, torch.float32)
    held = [k[8:] for k in z.files if k.startswith("refgrad:")]
    assert held and (name not in SMALL or sorted(held) == sorted(g64))
    assert not any(k in held for k in O.GRADLESS)
    gmax = max(float(np.abs(v).max()) for v in g64.values())
    for k in g64:          # the restatement in fp64 is the oracle (a tensor whose gradient is zero in exact arithmetic: against the model's largest)
        assert float(np.abs(t64[k] - g64[k]).max()) < 1e-9 * max(float(np.abs(g64[k]).max()), 1e-6 * gmax), k
    def noise_of(k):
        return max(float(np.abs(t32[k].astype(np.float64) - g64[k]).max()), 2.0 ** -23 * float(np.abs(g64[k]).max()))
    for k in held:
        noise = max(noise_of(k), noise_of(O.noise_partner(k)) if O.noise_partner(k) else 0.0)
        assert float(np.abs(z["refgrad:" + k].astype(np.float64) - g64[k]).max()) <= 16 * noise, k


def test_torch_restatement_with_keep_masks_equals_the_oracle():
    z, cfg, P = load_case(SMALL[1])
    keep = O.keep_masks(z["x"].shape[0], cfg, seed=5, step=3, p=0.5)
    o = O.forward_backward(P, z["x"], z["y"], cfg, keep=keep, dropout_p=0.5)
    pred, mse, recon, g = O.torch_grads(P, z["x"], z["y"], cfg, torch.float64, keep=keep, dropout_p=0.5)
    assert rel(pred, o["pred"]) < 1e-12 and abs(mse - o["mse"]) < 1e-12 and abs(recon - o["recon"]) < 1e-12
    gmax = max(float(np.abs(v).max()) for v in g.values())
    for k in g:
        assert float(np.abs(g[k] - o["grads"][k]).max()) < 1e-9 * max(float(np.abs(g[k]).max()), 1e-6 * gmax), k
    assert rel(o["pred"], oracle_run(SMALL[1])["pred"]) > 1e-3          # the masks do change the function


def test_shards_sum_to_the_batch_in_the_oracle():
    z, cfg, P = load_case(SMALL[0])
    full = oracle_run(SMALL[0])
    a = O.forward_backward(P, z["x"][:1], z["y"][:1], cfg, global_batch=4)
    b = O.forward_backward(P, z["x"][1:], z["y"][1:], cfg, global_batch=4)
    assert abs(a["loss"] + b["loss"] - full["loss"]) < 1e-12
    gmax = max(float(np.abs(v).max()) for v in full["grads"].values())
    for k in full["grads"]:
        assert float(np.abs(a["grads"][k] + b["grads"][k] - full["grads"][k]).max()) < 1e-10 * gmax, k


def test_keep_masks_share_offsets_and_steps():
    cfg = load_case(FULL[2])[1]
    for p in (0.5,):
        masks = O.keep_masks(3, cfg, seed=11, step=1, p=p)
        assert len(masks) == len(cfg["gat_layer_dim"])
        for mk in masks:
            assert mk.size >= 1000 and 0.45 <= mk.mean() <= 0.55
        assert not np.array_equal(masks[0], masks[1])
        assert not np.array_equal(masks[0], O.keep_masks(3, cfg, seed=11, step=2, p=p)[0])
        tail = O.keep_masks(2, cfg, seed=11, step=1, p=p, sample_offset=1)
        assert np.array_equal(tail[0], masks[0][cfg["num_patch"]:])          # masks follow the global sample index
    small = load_case(SMALL[0])[1]
    big = O.keep_masks(40, small, seed=2, step=9, p=0.5)
    assert all(mk.size >= 1000 and 0.45 <= mk.mean() <= 0.55 for mk in big)


def test_names_shapes_and_counts():
    for name, count in zip(FULL, (230347, 280386, 595654)):
        cfg = load_case(name)[1]
        names = O.param_names(cfg)
        assert len(names) == 36 and names.index("node_importance_linear.weight") == 12 and names[14] == "encoder.0.weight"
        assert O.flat_names(cfg)[:2] == list(O.GRADLESS) and sorted(O.flat_names(cfg)) == sorted(names)
        assert O.param_count(cfg) == count
