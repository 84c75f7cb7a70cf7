"""GDAGDL HIP path vs the reference's golden outputs and vs the fp64 oracle (GPU).

Gates.  Predictions, taps and both loss terms: TOL = 1e-4 relative to the tensor's largest value, the bar of the other families; the mask
must be equal element for element and ni NaN exactly where the fixture's is.  Gradients: element by element through tests/grad_gate.py
at RTOL and margin 16.  The floor's noise term is the REFERENCE's fp32 gradient against the fp64 oracle (the fixture's ``refgrad:``
entry where it holds one, else an fp32 run of the torch restatement on the CPU), never the kernels' output.  RTOL starts at 5e-4 and
is halved while the worst ratio of every case stays below 0.5 on an MI355X (the rule LOGO and DVGTformer were given); every case
prints its worst ratio along that ladder ("GDAGDL-GATE ...").
Measured over every case of this file on an MI355X, worst ratio per RTOL: 0.249 from 5e-4 down to 5e-4 / 2^4, then 0.260, 0.299, 0.323,
0.364, 0.410 at the next five halvings, 0.490 at 5e-4 / 2^10 = 4.8828125e-7 (edge-N17-f33, gat_layers.1.linear.bias), 0.543 at
5e-4 / 2^11: RTOL is 5e-4 / 2^10 = 4.8828125e-7, four fp32 ulps -- below that the floor carries every element and the ratio saturates
at 0.60.
Tensors whose gradient is zero in exact arithmetic are detected (grad_gate.zero_in_exact_arithmetic), not listed: an attention bias
whose scores all lie on one side of the leaky ReLU's kink (the softmax ignores a per-row constant), and every GAT tensor of a batch
whose graphs are all masked out.  Inputs of the seeded cases are drawn like the fixtures' (gdagdl_oracle.draw_inputs): every mask
decision stands three orders above fp32 rounding, so the fp32 kernels and the fp64 oracle decide alike."""
import functools
import os

import numpy as np
import pytest
import torch

import family_kit as K
import gdagdl_oracle as O
from family_kit import DEV, GOLD, dev, grads_of, rel
from test_gdagdl_oracle_golden import CURVE, FULL, SMALL, load_case, oracle_run, seeded_weights

pytestmark = pytest.mark.gpu
TOL, RTOL = 1e-4, 5e-4 / 2 ** 10
LADDER = [5e-4 / 2 ** k for k in range(13)]


def make_cfg(nperseg, frames, T, widths, E=3, A=8, Oo=4):
    return dict(num_patch=T, patch_size=(frames - 1) * nperseg, num_nodes=nperseg // 2 + 1, nperseg=nperseg, input_dim=frames,
                gat_layer_dim=list(widths), lstm_hidden_dim=E, autoencoder_hidden_dim=A, autoencoder_out_dim=Oo)


TINY = make_cfg(4, 3, 3, [5, 4, 3])


def build_model(cfg, sd, dropout=0.0):
    from gnn_rul_benchmarking_amd.gdagdl import GDAGDL_model
    return K.build_model(GDAGDL_model, cfg, sd, dropout)


def check_grads(what, got, g64, ref32, cfg):
    """Every live tensor through the element-wise gate; the two gradless tensors' entries must be exact zeros.  Returns the names
    detected as zero in exact arithmetic (held to family_kit.residue_bound)."""
    return K.check_grads(what, "GDAGDL", got, g64, ref32, RTOL, K.RESIDUE, exact_zero=O.GRADLESS, noise_partner=O.noise_partner, ladder=LADDER)


def check_forward(what, m, bs, pred, loss, want, want_loss, want_recon=None):
    errs = {**K.pred_err(pred, want), **K.tap_errs(m, bs, want, [k for k in ("mag", "yo", "H") if k in want], same_shape=False)}
    ni, wni = m.tap(bs, "ni").cpu().numpy(), np.asarray(want["ni"])
    assert np.array_equal(np.isnan(ni), np.isnan(wni)), what                       # NaN exactly where the reference's is
    assert np.array_equal(m.tap(bs, "mask").cpu().numpy(), np.asarray(want["mask"], np.float32)), what      # element for element
    if not np.isnan(ni).all():
        errs["ni"] = rel(ni[~np.isnan(ni)], wni[~np.isnan(wni)])
    errs.update(K.loss_err(loss, want_loss))
    if want_recon is not None:
        errs["recon"] = abs(float(m._grad_flat[m.num_live + 1]) - want_recon) / abs(want_recon)
    K.check_forward(what, "GDAGDL", errs, TOL)


@functools.lru_cache(maxsize=None)
def ref32_of(name):
    """The reference's fp32 gradient: the fixture's where it holds the tensor, else the torch restatement's on the CPU."""
    z, cfg, sd = load_case(name)
    g = O.torch_grads(sd, z["x"], z["y"], cfg, torch.float32)[3] if name in FULL else {}
    g.update({k[8:]: z[k] for k in z.files if k.startswith("refgrad:")})
    return g


# ---- 1. the reference's fixtures ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL + FULL)
def test_fixture_forward_taps_losses_and_gradients(name):
    z, cfg, sd = load_case(name)
    o = oracle_run(name)
    m = build_model(cfg, sd).train()
    x, y = dev(z["x"]), dev(z["y"])
    bs = x.size(0)
    pred, loss = m.fused_mse_step(x, y)
    ref = {k[4:]: z[k] for k in z.files if k.startswith("tap:")}
    ref["pred"] = z["pred"]
    check_forward(name, m, bs, pred, loss, ref, float(z["loss"]), float(z["recon"]))      # against the reference itself ...
    check_forward(name + "-oracle", m, bs, pred, loss, o, o["loss"], o["recon"])          # ... and the fp64 oracle
    assert abs(float(loss) - float(m._grad_flat[m.num_live + 1]) - float(z["mse"])) < TOL * max(float(z["mse"]), float(z["loss"]))
    check_grads(name, grads_of(m), o["grads"], ref32_of(name), cfg)
    fused = m.bucket[:m.num_live + 1].clone()
    m.eval()
    with torch.no_grad():
        ev = m(x)
    assert ev.shape == (bs, 1) and rel(ev.cpu().numpy(), z["pred_eval"]) < TOL
    assert np.isfinite(ev.cpu().numpy()).all()                                        # the zero patch's NaN stays inside the mask
    if name in SMALL:
        m2 = build_model(cfg, sd).train()                                             # forward, then backward through autograd: the same bits
        out, recon = m2(x, train=True)
        assert out.requires_grad and out.shape == (bs, 1)
        (torch.nn.functional.mse_loss(out, y) + recon).backward()
        assert m2.node_importance_linear.weight.grad is None and m2.node_importance_linear.bias.grad is None
        auto = torch.cat([t.grad.reshape(-1) for t in m2._named()[2:]])
        want = fused[cfg["input_dim"] + 1:-1]                                          # (d pred comes from torch's MSE here: not the same bits)
        assert float((auto - want).abs().max()) < 1e-5 * float(want.abs().max())


# ---- 2. seeded cases against the fp64 oracle ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def seeded_case(cfg_items, bs, seed, planted):
    cfg = {k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg_items}
    sd = seeded_weights(cfg, seed)
    x = O.draw_inputs(cfg, bs, seed, sd["node_importance_linear.weight"].astype(np.float64), sd["node_importance_linear.bias"].astype(np.float64),
                      planted=planted)
    y = np.random.default_rng(seed).uniform(0, 1, bs).astype(np.float32)
    return cfg, sd, x, y


def items(cfg):
    return tuple((k, tuple(v) if isinstance(v, list) else v) for k, v in cfg.items())


def oracle_step_check(what, cfg, sd, x, y, torch_noise=True):
    o = O.forward_backward(sd, x, y, cfg)
    g32 = O.torch_grads(sd, x, y, cfg, torch.float32)[3]
    m = build_model(cfg, sd).train()
    pred, loss = m.fused_mse_step(dev(x), dev(y))
    check_forward(what, m, x.shape[0], pred, loss, o, o["loss"], o["recon"])
    return check_grads(what, grads_of(m), o["grads"], g32, cfg), m, o


EDGES = {
    "N17-f33": (make_cfg(32, 33, 2, [9, 5, 3]), 2, True),          # crosses 16 nodes and 32 frames
    "N33-f3-one-layer": (make_cfg(64, 3, 1, [6]), 2, False),       # the node limit: more nodes than half a wavefront
    "one-layer": (make_cfg(8, 5, 2, [7]), 2, True),
    "four-layers": (make_cfg(8, 5, 2, [7, 6, 5, 4]), 2, True),
    "bs1": (make_cfg(4, 3, 5, [5, 4, 3]), 1, True),
    "width-65-and-128": (make_cfg(8, 5, 2, [65, 128, 3]), 2, True),   # a second and a partial channel chunk per lane
}


@pytest.mark.parametrize("key", list(EDGES))
def test_edge_shapes_match_oracle(key):
    cfg, bs, planted = EDGES[key]
    cfg, sd, x, y = seeded_case(items(cfg), bs, 7, planted)
    oracle_step_check("edge-" + key, cfg, sd, x, y)


def test_more_graphs_than_the_attention_grid_has_wavefronts():
    """1 400 samples x 3 patches = 4 200 graphs: the attention grid is capped at 1 024 workgroups of 4 wavefronts, so some wavefronts
    take a second graph and the partial rows hold sums."""
    cfg, sd, x, y = seeded_case(items(TINY), 1400, 9, True)
    oracle_step_check("tiny-bs1400", cfg, sd, x, y)


def test_a_batch_whose_graphs_are_all_masked_out():
    """Zero patches (NaN graphs) and nothing else: h is 0 behind every layer, the prediction is the oracle's, and every GAT gradient is an
    exact zero (Q = 0 => dZ = 0)."""
    cfg, sd, _, y = seeded_case(items(TINY), 4, 9, True)
    x = np.zeros((4, cfg["num_patch"] * cfg["patch_size"]), np.float32)
    zero, m, o = oracle_step_check("all-masked", cfg, sd, x, y)
    assert not o["mask"].any() and np.isnan(o["ni"]).all() and not m.tap(4, "yo").any()
    gat = [k for k in O.param_names(cfg) if k.startswith("gat_layers.")]
    assert set(gat) <= set(zero)
    got = grads_of(m)
    for k in gat:
        assert not got[k].any(), k
    assert got["encoder.0.bias"].any() and got["linear.weight"].any()


# ---- 3. dropout ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [SMALL[1], FULL[1]])
def test_training_with_dropout_matches_oracle(name):
    z, cfg, sd = load_case(name)
    bs, p = z["x"].shape[0], 0.5
    m = build_model(cfg, sd, dropout=p).train()
    keep = O.keep_masks(bs, cfg, m._seed, m._step + 1, p)
    o = O.forward_backward(sd, z["x"], z["y"], cfg, keep=keep, dropout_p=p)
    g32 = O.torch_grads(sd, z["x"], z["y"], cfg, torch.float32, keep, p)[3]
    x, y = dev(z["x"]), dev(z["y"])
    pred, loss = m.fused_mse_step(x, y)
    assert rel(o["pred"], z["pred"]) > 10 * TOL                              # the masks matter
    check_forward(name + "-dropout", m, bs, pred, loss, o, o["loss"], o["recon"])
    check_grads(name + "-dropout", grads_of(m), o["grads"], g32, cfg)
    first = m.bucket[:m.num_live + 1].clone()
    m._step = 0
    m.fused_mse_step(x, y)
    assert torch.equal(m.bucket[:m.num_live + 1], first)                     # the same seed and step: the same bits
    m.fused_mse_step(x, y)
    assert not torch.equal(m.bucket[:m.num_live + 1], first)                 # another step: another mask
    m.eval()                                                                  # eval draws none
    with torch.no_grad():
        assert rel(m(x).cpu().numpy(), z["pred_eval"]) < TOL


# ---- 4. shards -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_two_shards_sum_to_the_full_batch(p):
    z, cfg, sd = load_case(SMALL[0])
    bs = z["x"].shape[0]
    x, y = dev(z["x"]), dev(z["y"])
    full = build_model(cfg, sd, dropout=p).train()
    keep = O.keep_masks(bs, cfg, full._seed, 1, p) if p else None
    o = O.forward_backward(sd, z["x"], z["y"], cfg, keep=keep, dropout_p=p)
    g32 = O.torch_grads(sd, z["x"], z["y"], cfg, torch.float32, keep, p)[3]
    full.fused_mse_step(x, y)
    total = torch.zeros_like(full.bucket)
    preds = []
    for lo, hi in ((0, 1), (1, bs)):
        m = build_model(cfg, sd, dropout=p).train()
        m._seed = full._seed
        pred, _ = m.fused_mse_step(x[lo:hi], y[lo:hi], global_batch=bs, sample_offset=lo)
        preds.append(pred.clone())
        total += m.bucket
    assert rel(torch.cat(preds).cpu().numpy(), o["pred"].reshape(-1)) < TOL       # under dropout: the full batch's masks
    assert abs(float(total[full.num_live]) - o["loss"]) < TOL * o["loss"]
    assert abs(float(total[full.num_live]) - float(full.bucket[full.num_live])) < 1e-6 * o["loss"]
    check_grads(f"shards-p{p}", grads_of(full, total), o["grads"], g32, cfg)
    a, b = total[:full.num_live].cpu().numpy(), full.bucket[:full.num_live].cpu().numpy()
    assert np.abs(a - b).max() < 1e-5 * np.abs(b).max()


# ---- 5. fixed-order reductions ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["xjtu-bs2", "tiny-bs1400"])
def test_two_runs_give_the_same_bits(case):
    if case == "xjtu-bs2":
        z, cfg, sd = load_case(FULL[2])
        x, y = z["x"], z["y"]
    else:
        cfg, sd, x, y = seeded_case(items(TINY), 1400, 9, True)
    outs = []
    for _ in range(2):
        m = build_model(cfg, sd, dropout=0.5).train()
        m._seed = 99
        m.fused_mse_step(dev(x), dev(y))
        outs.append(m._grad_flat.clone())
    assert torch.isfinite(outs[0]).all() and outs[0].abs().max() > 0 and torch.equal(outs[0], outs[1])
    print("GDAGDL-GATE run-to-run: identical bits")


# ---- 6. the optimizer, the curve ---------------------------------------------------------------------------------------------------------
def test_fused_step_applies_adam_to_every_live_element_once_and_never_to_the_gradless():
    """The twin-model procedure (family_kit.adam_twin_check), dropout and weight decay on: the optimized range [f + 1, count) within the
    bounds, the two gradless tensors' parameters and moments bit-identical and their bucket entries exact zeros."""
    from test_fused_adam_families_gpu import _bits, _np
    z, cfg, sd = load_case(SMALL[1])
    f1 = cfg["input_dim"] + 1
    b = K.adam_twin_check(lambda: build_model(cfg, sd, dropout=0.5).train(), dev(z["x"]), dev(z["y"]), "GDAGDL", first=f1)
    assert b.optimized_range == (f1, b.num_live)
    assert np.array_equal(_bits(_np(b.node_importance_linear.weight)), _bits(sd["node_importance_linear.weight"]))
    assert np.array_equal(_bits(_np(b.node_importance_linear.bias)), _bits(sd["node_importance_linear.bias"]))


def test_training_curve_matches_reference_algorithm():
    """Twenty update() steps against the reference's own.  Tolerances: GRU_CM's curve tolerances (tests/test_grucm_gpu.py: the first
    three losses 1e-4, every loss 2e-3, the eval prediction at the end 5e-3)."""
    z = np.load(os.path.join(GOLD, CURVE + ".npz"))
    cfg = load_case(SMALL[1])[1]
    assert cfg == __import__("json").loads(str(z["cfg_json"]))
    sd0 = {k[4:]: z[k] for k in z.files if k.startswith("sd0:")}
    _, sd = K.curve_check("GDAGDL", "GDAGDL", cfg, z, sd0, dict(steps=20, first3=1e-4, every=2e-3, eval=5e-3), dropout_off=True)
    for k in O.GRADLESS:
        assert torch.equal(sd[k].cpu(), torch.from_numpy(z["sd0:" + k])), k           # untouched by Adam and its weight decay


def test_trainer_matches_reference_harness_run_on_phm2012(tmp_path, monkeypatch):
    """--GNN_method GDAGDL on PHM2012 Condition_1 as the reference wires it: the reference's own harness, run on the CPU by
    tests/golden/make_golden_gdagdl.py::case_trainer_phm2012 with the attention dropout switched off on the constructed model, vs this
    package's harness on the GPU with the same switch.  Bars: those of tests/test_trainer_gpu.py's harness tests."""
    z = np.load(os.path.join(GOLD, "gdagdl_trainer_phm2012_c1_reference_run.npz"))

    def row(tr):
        assert tr.train_configs["batch_size"] == int(z["batch_size"]) and tr.train_configs["learning_rate"] == float(z["lr"])
        assert tr.model_configs == load_case(FULL[0])[1]
    tr, per_epoch = K.harness_run(tmp_path, monkeypatch, "GDAGDL", "PHM2012", "Condition_1", z, no_dropout=K.model_dropout_off, configure=row)
    K.assert_harness("GDAGDL", per_epoch, K.state_of(tr), z,      # RMSE, absolute (north star); MAE, RMSE relative
                     dict(rmse_abs=1e-3, rmse_scale=1.0, rel=1e-3, rel_from=2, final=2e-3, final_prefix="model."))


# ---- 7. coverage -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [make_cfg(66, 3, 1, [2]), make_cfg(4, 65, 1, [2]), make_cfg(4, 3, 1, [2] * 5), make_cfg(4, 3, 1, [513]),
                                 make_cfg(4, 3, 1, [2], E=129), make_cfg(4, 3, 1, [2], A=1025), make_cfg(4, 3, 1, [2], Oo=1025)],
                         ids=["nperseg66", "f65", "five-layers", "width513", "lstm129", "A1025", "O1025"])
def test_just_outside_each_limit_is_not_covered_and_launches_nothing(cfg):
    from gnn_rul_benchmarking_amd.gdagdl import GDAGDL_model
    K.refused_outside_limits(GDAGDL_model(**cfg), torch.rand(2, cfg["num_patch"] * cfg["patch_size"], device=DEV))
