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

import adam_reference as R
import grad_gate as GG
import gdagdl_oracle as O
from test_gdagdl_oracle_golden import CURVE, FULL, SMALL, load_case, oracle_run, rel, seeded_weights

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"
TOL, RTOL = 1e-4, 5e-4 / 2 ** 10
LADDER = [5e-4 / 2 ** k for k in range(13)]


def make_cfg(nperseg, frames, T, widths, E=3, A=8, Oo=4):
    return dict(num_patch=T, patch_size=(frames - 1) * nperseg, num_nodes=nperseg // 2 + 1, nperseg=nperseg, input_dim=frames,
                gat_layer_dim=list(widths), lstm_hidden_dim=E, autoencoder_hidden_dim=A, autoencoder_out_dim=Oo)


TINY = make_cfg(4, 3, 3, [5, 4, 3])


def build_model(cfg, sd, dropout=0.0):
    from gnn_rul_benchmarking_amd.gdagdl import GDAGDL_model
    m = GDAGDL_model(**cfg)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in sd.items()}, strict=True)
    m.dropout_p = dropout
    return m.to(DEV)


def grads_of(m, bucket=None):
    flat = (m._grad_flat if bucket is None else bucket)[:m.num_live].detach().cpu().numpy().astype(np.float64)
    return {name: flat[off:off + int(np.prod(shape))].reshape(shape) for name, (off, shape) in m._layout.items()}


def dev(a):
    return torch.from_numpy(np.asarray(a, np.float32)).to(DEV)


def check_grads(what, got, g64, ref32, cfg):
    """Every live tensor through the element-wise gate; the two gradless tensors' entries must be exact zeros.  Returns the names
    detected as zero in exact arithmetic."""
    for k in O.GRADLESS:
        assert not got[k].any(), k
    zero = GG.zero_in_exact_arithmetic(g64, ref32)
    gmax = max(float(np.abs(v).max()) for v in g64.values())
    ladder = np.zeros(len(LADDER))
    worst = (0.0, None)
    for k in g64:
        assert got[k].shape == g64[k].shape, k
        if k in zero:               # rounding residue of a sum that cancels: at most the reference's own, or fp32 ulps of the model's largest gradient
            bound = 16 * max(float(np.abs(ref32[k]).max()), 2.0 ** -23 * gmax)
            assert np.abs(got[k]).max() <= bound, (k, np.abs(got[k]).max(), bound)
            continue
        floor = GG.floor_for(ref32[k], g64[k])
        if O.noise_partner(k):          # a one-element tensor shares its layer's attention.weight noise (gdagdl_oracle.noise_partner)
            floor = max(floor, GG.floor_for(ref32[O.noise_partner(k)], g64[O.noise_partner(k)]))
        ladder = np.maximum(ladder, [GG.gate(got[k], g64[k], r, floor)[0] for r in LADDER])
        ratio, where = GG.gate(got[k], g64[k], RTOL, floor)
        if ratio > 0.25:
            print(f"  grad {k}: gate {ratio:.3f} at {where}  rel {rel(got[k], g64[k]):.2e}  max|g| {np.abs(g64[k]).max():.2e}")
        worst = max(worst, (ratio, k))
    print(f"GDAGDL-GATE {what}: worst gradient gate ratio {worst[0]:.3f} ({worst[1]}); zero in exact arithmetic: {zero}")
    print(f"GDAGDL-LADDER {what}: " + " ".join(f"{v:.3f}" for v in ladder))
    assert worst[0] <= 1.0, worst
    return zero


def check_forward(what, m, bs, pred, loss, want, want_loss, want_recon=None):
    errs = {"pred": rel(pred.detach().cpu().numpy().reshape(-1), np.asarray(want["pred"]).reshape(-1))}
    for k in ("mag", "yo", "H"):
        if k in want:
            errs[k] = rel(m.tap(bs, k).cpu().numpy(), np.asarray(want[k]).reshape(m.tap(bs, k).shape))
    ni, wni = m.tap(bs, "ni").cpu().numpy(), np.asarray(want["ni"])
    assert np.array_equal(np.isnan(ni), np.isnan(wni)), what                       # NaN exactly where the reference's is
    assert np.array_equal(m.tap(bs, "mask").cpu().numpy(), np.asarray(want["mask"], np.float32)), what      # element for element
    if not np.isnan(ni).all():
        errs["ni"] = rel(ni[~np.isnan(ni)], wni[~np.isnan(wni)])
    if loss is not None:
        errs["loss"] = abs(float(loss) - want_loss) / abs(want_loss)
    if want_recon is not None:
        errs["recon"] = abs(float(m._grad_flat[m.num_live + 1]) - want_recon) / abs(want_recon)
    print(f"GDAGDL-GATE {what}: forward " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < TOL, (k, v)


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
    """The twin-model procedure of tests/test_fused_adam_families_gpu.py (bounds from tests/adam_reference.py), dropout and weight decay
    on: the optimized range [f + 1, count) within the bounds, the two gradless tensors' parameters and moments bit-identical and their
    bucket entries exact zeros."""
    from gnn_rul_benchmarking_amd.optim import FusedAdam
    from test_fused_adam_families_gpu import LR, SEED, STEP0, WD, _bits, _np
    z, cfg, sd = load_case(SMALL[1])
    x, y = dev(z["x"]), dev(z["y"])
    f1 = cfg["input_dim"] + 1
    assert WD > 0

    def ready():
        m = build_model(cfg, sd, dropout=0.5).train()
        m._seed = SEED
        return m
    a = ready()
    p0 = _np(a.flat_params)
    _, loss_a = a.fused_mse_step(x, y)
    g_a, loss_a = _np(a.bucket[:a.num_live]), float(loss_a)
    assert np.isfinite(g_a).all() and np.array_equal(_bits(_np(a.flat_params)), _bits(p0)) and not g_a[:f1].any()
    b = ready()
    assert b.optimized_range == (f1, b.num_live)
    opt = FusedAdam(b, lr=LR, weight_decay=WD)
    m0, v0 = R.moments_like(g_a, np.random.default_rng(12))
    s = opt.state_dict()
    s.update(step=STEP0, exp_avg=torch.from_numpy(m0).to(DEV), exp_avg_sq=torch.from_numpy(v0).to(DEV))
    opt.load_state_dict(s)
    worst = dict(p=0.0, m=0.0, v=0.0)
    for k in (STEP0 + 1, STEP0 + 2, STEP0 + 3):
        before = tuple(_np(t) for t in (b.flat_params, opt._exp_avg, opt._exp_avg_sq))
        _, loss_b = b.fused_mse_step(x, y, opt)
        g = _np(b.bucket[:b.num_live])
        after = tuple(_np(t) for t in (b.flat_params, opt._exp_avg, opt._exp_avg_sq))
        if k == STEP0 + 1:
            assert np.array_equal(_bits(g), _bits(g_a)) and float(loss_b) == loss_a
        assert not g[:f1].any()
        for got, was in zip(after, before):
            assert np.array_equal(_bits(got[:f1]), _bits(was[:f1]))               # no update, no weight decay, no moment
        r = R.check(tuple(t[f1:] for t in after), before[0][f1:], g[f1:], before[1][f1:], before[2][f1:], k, WD, 1.0, what=f"GDAGDL, step {k}")
        worst = {q: max(worst[q], r[q]) for q in worst}
    assert opt._steps == STEP0 + 3
    assert np.array_equal(_bits(_np(b.node_importance_linear.weight)), _bits(sd["node_importance_linear.weight"]))
    assert np.array_equal(_bits(_np(b.node_importance_linear.bias)), _bits(sd["node_importance_linear.bias"]))
    print("ADAM-RATIO family GDAGDL: " + " ".join(f"{q}={worst[q]:.3f}" for q in "pmv"))


def test_training_curve_matches_reference_algorithm():
    """Twenty update() steps against the reference's own.  Tolerances: GRU_CM's curve tolerances (tests/test_grucm_gpu.py: the first
    three losses 1e-4, every loss 2e-3, the eval prediction at the end 5e-3)."""
    from gnn_rul_benchmarking_amd.algorithms import get_algorithm_class
    z = np.load(os.path.join(GOLD, CURVE + ".npz"))
    cfg = load_case(SMALL[1])[1]
    assert cfg == __import__("json").loads(str(z["cfg_json"]))
    algo = get_algorithm_class("GDAGDL")(cfg, {"learning_rate": float(z["lr"]), "weight_decay": float(z["wd"])}, DEV)
    algo.model.load_state_dict({k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd0:")}, strict=True)
    algo.model.dropout_p = 0.0
    algo.to(DEV).train()
    xs, ys = torch.from_numpy(z["xs"]).to(DEV), torch.from_numpy(z["ys"]).to(DEV)
    losses = np.asarray([algo.update(xs[s], ys[s], 1)["loss"] for s in range(xs.size(0))])
    ref = z["losses"]
    print("GDAGDL-GATE curve: worst loss ratio", np.abs(losses / ref - 1).max())
    assert len(ref) == 20 and np.max(np.abs(losses[:3] - ref[:3]) / ref[:3]) < 1e-4
    assert np.max(np.abs(losses - ref) / ref) < 2e-3
    algo.eval()
    with torch.no_grad():
        assert rel(algo.model(xs[0]).cpu().numpy(), z["eval_pred_end"]) < 5e-3
    sd = algo.model.state_dict()
    for k in O.GRADLESS:
        assert torch.equal(sd[k].cpu(), torch.from_numpy(z["sd0:" + k])), k           # untouched by Adam and its weight decay


def test_trainer_matches_reference_harness_run_on_phm2012(tmp_path, monkeypatch):
    """--GNN_method GDAGDL on PHM2012 Condition_1 as the reference wires it: the reference's own harness, run on the CPU by
    tests/golden/make_golden_gdagdl.py::case_trainer_phm2012 with the attention dropout switched off on the constructed model, vs this
    package's harness on the GPU with the same switch.  Bars: those of tests/test_trainer_gpu.py's harness tests."""
    import argparse
    import sys
    sys.path.insert(0, GOLD)
    from synth import synthetic_phm2012
    from gnn_rul_benchmarking_amd import trainer as T
    z = np.load(os.path.join(GOLD, "gdagdl_trainer_phm2012_c1_reference_run.npz"))
    (xtr, ytr), (xte, yte) = synthetic_phm2012(int(z["seed"]), int(z["n_train"]), int(z["n_test"]))
    assert abs(xtr.astype(np.float64).sum() - float(z["x_train_checksum"])) < 1e-6
    d = tmp_path / "data" / "PHM2012" / "Condition_1"
    os.makedirs(d)
    torch.save({"samples": xtr, "labels": ytr, "max_ruls": 1.0}, d / "train.pt")
    torch.save({"samples": xte, "labels": yte, "max_ruls": 1.0}, d / "test.pt")
    monkeypatch.chdir(tmp_path)
    base = T.get_algorithm_class("GDAGDL")

    class NoDropout(base):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.model.dropout_p = 0.0
    monkeypatch.setattr(T, "get_algorithm_class", lambda n: NoDropout)
    args = argparse.Namespace(save_dir=str(tmp_path / "logs"), experiment_description="exp", run_description="r",
                              GNN_method="GDAGDL", data_path=str(tmp_path / "data"), dataset="PHM2012",
                              dataset_id="Condition_1", bearing_id="Testing_bearing_1", num_runs=1, device=DEV)
    tr = T.GNN_RUL_trainer(args)
    tr.train_configs["num_epochs"] = int(z["epochs"])
    assert tr.train_configs["batch_size"] == int(z["batch_size"]) and tr.train_configs["learning_rate"] == float(z["lr"])
    assert tr.model_configs == load_case(FULL[0])[1]
    per_epoch = []
    orig = tr.calc_results_per_run

    def spy(run_id):
        per_epoch.append(T._calc_metrics(tr.pred_labels, tr.true_labels, tr.max_ruls))
        return orig(run_id)
    tr.calc_results_per_run = spy
    tr.train()
    got, ref = np.asarray(per_epoch, np.float64), z["per_epoch"]
    print("GDAGDL harness per-epoch got/ref:\n", got, "\n", ref)
    assert got.shape == ref.shape == (int(z["epochs"]), 4)
    assert np.max(np.abs(got[:, 3] - ref[:, 3])) < 1e-3                              # RMSE, absolute (north star)
    assert np.max(np.abs(got[:, 2:] - ref[:, 2:]) / np.abs(ref[:, 2:])) < 1e-3      # MAE, RMSE relative
    sd = tr.algorithm.state_dict()
    for k in z.files:
        if k.startswith("final:"):
            a, b = sd["model." + k[6:]].cpu().numpy().astype(np.float64), z[k].astype(np.float64)
            assert np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30) < 2e-3, k


# ---- 7. coverage -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [make_cfg(66, 3, 1, [2]), make_cfg(4, 65, 1, [2]), make_cfg(4, 3, 1, [2] * 5), make_cfg(4, 3, 1, [513]),
                                 make_cfg(4, 3, 1, [2], E=129), make_cfg(4, 3, 1, [2], A=1025), make_cfg(4, 3, 1, [2], Oo=1025)],
                         ids=["nperseg66", "f65", "five-layers", "width513", "lstm129", "A1025", "O1025"])
def test_just_outside_each_limit_is_not_covered_and_launches_nothing(cfg):
    from gnn_rul_benchmarking_amd.gdagdl import GDAGDL_model
    m = GDAGDL_model(**cfg).to(DEV)
    x = torch.rand(2, cfg["num_patch"] * cfg["patch_size"], device=DEV)
    with pytest.raises(RuntimeError, match="do not cover this configuration"):
        m(x)
    with pytest.raises(RuntimeError, match="do not cover this configuration"):
        m.fused_mse_step(x, torch.zeros(2, device=DEV))
    assert not m._bufs and not m._grad_flat.any()                  # no workspace was made, nothing was written
