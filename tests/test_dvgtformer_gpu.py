"""DVGTformer HIP path vs the reference's golden outputs and vs the fp64 oracle (GPU).

Gates.  Predictions, taps and the loss: TOL = 1e-4 relative to the tensor's largest value, the bar of the other families.  Gradients:
element by element through tests/grad_gate.py at RTOL and margin 16, starting from AGCN_TF's 5e-4 (tests/test_agcntf_gpu.py:23), the
nearest family; RTOL is halved while the worst ratio of every case stays below 0.5 on an MI355X (the rule LOGO was given).  Measured
over every case of this file: 0.370 at 5e-4, 0.376 at 3.1e-5, 0.458 at 7.8e-6 (the floor carries most elements, so the ratio moves
slowly), 0.748 at 5e-4 / 2^7 = 3.90625e-6 (edge-N24, tvgtformer_blocks.0.linears_Q_temp.1.bias): that is RTOL.  The floor's
noise term is the REFERENCE's fp32 gradient against the fp64 oracle (the fixture's ``refgrad:`` entries; without a fixture an fp32 run
of the torch restatement on the CPU), never the kernels' output.  The tensors whose gradient is zero in exact arithmetic are detected
(grad_gate.zero_in_exact_arithmetic), not listed: at lambda = 0.5 they must be exactly the linears_K biases, which the kernels write as
exact zeros.  Every test prints its worst gate ratio ("DVGT-GATE ...")."""
import argparse
import functools
import os

import numpy as np
import pytest
import torch

import adam_reference as R
import grad_gate as GG
import dvgtformer_oracle as O
from test_dvgtformer_oracle_golden import CURVE, FULL, SMALL, load_case, oracle_of, rel, seeded_state

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"
TOL, RTOL = 1e-4, 5e-4 / 2 ** 7
FD = dict(num_nodes=14, time_length=50, d_model=[144, 248], num_heads=4, lambda_param=0.5, d_ff=[72, 124], dropout=0.1, num_blocks=3)


def make_cfg(N, L, H=2, nb=1, lam=0.5, d=(6, 10), ff=(4, 6)):
    return dict(num_nodes=N, time_length=L, d_model=list(d), num_heads=H, lambda_param=lam, d_ff=list(ff), dropout=0.1, num_blocks=nb)


def build_model(cfg, sd, dropout=0.0):
    from gnn_rul_benchmarking_amd.dvgtformer import DVGTformer_model
    m = DVGTformer_model(**cfg)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in sd.items()}, strict=True)
    m.dropout_p = dropout
    return m.to(DEV)


def grads_of(m, bucket=None):
    flat = (m._grad_flat if bucket is None else bucket)[:m.num_live].detach().cpu().numpy().astype(np.float64)
    return {name: flat[off:off + int(np.prod(shape))].reshape(shape) for name, (off, shape) in m._layout.items()}


def k_weight_of(name):
    """The K weight of the head a Q / K tensor belongs to (the scale of the rounding residue a zero-in-exact-arithmetic tensor may hold)."""
    return name.replace("linears_Q_", "linears_K_").rsplit(".", 1)[0] + ".weight" if "linears_" in name else None


def check_grads(what, got, g64, ref32, cfg):
    """Every tensor through the element-wise gate; returns the names detected as zero in exact arithmetic."""
    zero = GG.zero_in_exact_arithmetic(g64, ref32)
    worst = (0.0, None)
    for k in O.param_names(cfg):
        assert got[k].shape == g64[k].shape, k
        if k in zero:
            if got[k].any():                        # not exact zeros: at most the reference's own residue
                kw = k_weight_of(k)
                bound = 16 * max(np.abs(ref32[k]).max(), 2.0 ** -23 * (np.abs(g64[kw]).max() if kw else 0.0))
                assert np.abs(got[k]).max() <= bound, (k, np.abs(got[k]).max(), bound)
            continue
        ratio, where = GG.gate(got[k], g64[k], RTOL, GG.floor_for(ref32[k], g64[k]))
        if ratio > 0.25:
            print(f"  grad {k}: gate {ratio:.3f} at {where}  rel {rel(got[k], g64[k]):.2e}  max|g| {np.abs(g64[k]).max():.2e}")
        worst = max(worst, (ratio, k))
    print(f"DVGT-GATE {what}: worst gradient gate ratio {worst[0]:.3f} ({worst[1]}); zero in exact arithmetic: {len(zero)} tensors")
    assert worst[0] <= 1.0, worst
    return zero


def k_biases(cfg):
    return sorted(k for k in O.param_names(cfg) if "linears_K_" in k and k.endswith(".bias"))


def check_forward(what, m, bs, pred, loss, want, want_loss):
    errs = {"x0": rel(m.tap(bs, "x0").cpu().numpy(), want["x0"]), "enc": rel(m.tap(bs, "enc").cpu().numpy(), want["enc"]),
            "pred": rel(pred.detach().cpu().numpy().reshape(-1), np.asarray(want["pred"]).reshape(-1))}
    if loss is not None:
        errs["loss"] = abs(float(loss) - want_loss) / abs(want_loss)
    print(f"DVGT-GATE {what}: forward " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < TOL, (k, v)


def dev(a):
    return torch.from_numpy(np.asarray(a, np.float32)).to(DEV)


@functools.lru_cache(maxsize=None)
def ref32_of(name):
    """The reference's fp32 gradient: the fixture's, or (full geometry: too large to store) the torch restatement's on the CPU."""
    z, cfg, sd = load_case(name)
    if "refgrad:t_v" in z.files:
        return {k: z["refgrad:" + k] for k in O.param_names(cfg)}
    return O.torch_grads(sd, z["x"], z["y"], cfg, torch.float32)[2]


# ---- 1. the reference's fixtures ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL + FULL)
def test_fixture_forward_taps_loss_and_gradients(name):
    z, cfg, sd = load_case(name)
    o = oracle_of(name)
    m = build_model(cfg, sd).train()
    x, y = dev(z["x"]), dev(z["y"])
    bs = x.size(0)
    pred, loss = m.fused_mse_step(x, y)
    ref = {"x0": z["tap:x0"], "enc": z["tap:enc"], "pred": z["pred"]}
    check_forward(name, m, bs, pred, loss, ref, float(z["loss"]))                  # against the reference itself ...
    check_forward(name + "-oracle", m, bs, pred, loss, o, o["loss"])               # ... and the fp64 oracle
    zero = check_grads(name, grads_of(m), o["grads"], ref32_of(name), cfg)
    assert zero == k_biases(cfg) and len(zero) == 2 * cfg["num_blocks"] * cfg["num_heads"]
    for k in zero:
        assert not grads_of(m)[k].any(), k                                         # written as exact zeros
    fused = m.bucket[:m.num_live + 1].clone()
    m.eval()
    with torch.no_grad():
        ev = m(x)
    assert ev.shape == (bs, 1) and rel(ev.cpu().numpy(), z["pred_eval"]) < TOL
    m2 = build_model(cfg, sd).train()                                               # forward, then backward through autograd: the same bits
    out = m2(x)
    assert out.requires_grad and out.shape == (bs, 1)
    torch.nn.functional.mse_loss(out, y).backward()
    auto = torch.cat([t.grad.reshape(-1) for t in m2._named()])
    assert torch.equal(auto, fused[:-1])
    m3 = build_model(cfg, sd).train()                                               # the forward and backward entries with the targets
    x3, yv = m3._step_inputs(x, y)
    shp = m3._shape(bs)
    a = m3._args(shp, x3, True, 1, y=yv)
    m3._call("forward", shp, a)
    m3._call("backward", shp, a)
    assert torch.equal(m3.bucket[:m3.num_live + 1], fused)


# ---- 2. / 3. seeded cases against the fp64 oracle ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def seeded_case(cfg_items, bs, seed):
    cfg = {k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg_items}
    sd = seeded_state(cfg, seed)
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, (bs, cfg["num_nodes"], cfg["time_length"])).astype(np.float32)
    y = rng.uniform(0, 1, bs).astype(np.float32)
    return cfg, sd, x, y


def items(cfg):
    return tuple((k, tuple(v) if isinstance(v, list) else v) for k, v in cfg.items())


def oracle_step_check(what, cfg, sd, x, y):
    o = O.forward_backward(sd, x, y, cfg)
    g32 = O.torch_grads(sd, x, y, cfg, torch.float32)[2]
    m = build_model(cfg, sd).train()
    pred, loss = m.fused_mse_step(dev(x), dev(y))
    check_forward(what, m, x.shape[0], pred, loss, o, o["loss"])
    return check_grads(what, grads_of(m), o["grads"], g32, cfg), m


@pytest.mark.parametrize("N", [14, 20])
@pytest.mark.parametrize("bs", [3, 1])
def test_full_width_step_matches_oracle(N, bs):
    cfg, sd, x, y = seeded_case(items(dict(FD, num_nodes=N)), bs, 100 + N + bs)
    zero, _ = oracle_step_check(f"full-N{N}-bs{bs}", cfg, sd, x, y)
    assert zero == k_biases(cfg) and len(zero) == 24


EDGES = {
    "N2-L1": make_cfg(2, 1, H=1, d=(3, 2), ff=(2, 3)),                     # the smallest shape
    "L55": make_cfg(3, 55), "L56": make_cfg(3, 56),                        # time_length at its cap - 1 and at its cap
    "N23": make_cfg(23, 4), "N24": make_cfg(24, 4),                        # num_nodes at its cap - 1 and at its cap
    "N24-L56-ff128": make_cfg(24, 56, H=1, ff=(128, 128)),                 # the largest LDS layout (146 KB)
    "H1": make_cfg(5, 7, H=1), "H8": make_cfg(5, 7, H=8),                  # num_heads 1 and its maximum
    "nb1": make_cfg(5, 7, nb=1), "nb8": make_cfg(5, 7, nb=8),              # num_blocks 1 and its maximum
}


@pytest.mark.parametrize("key", list(EDGES))
def test_edge_shapes_match_oracle(key):
    cfg, sd, x, y = seeded_case(items(EDGES[key]), 2, 7)
    zero, _ = oracle_step_check("edge-" + key, cfg, sd, x, y)
    assert zero == k_biases(cfg)


@pytest.mark.parametrize("lam", [0.0, 1.0])
def test_lambda_extremes_drop_one_softmax_out_of_the_gradient(lam):
    """lambda = 1: the score softmax has weight 0, every Q and K tensor's gradient is an exact zero; lambda = 0: the graph softmax has
    weight 0 (no tensor loses its gradient: the input stage still feeds X)."""
    cfg, sd, x, y = seeded_case(items(make_cfg(5, 7, nb=2, lam=lam)), 3, 11)
    zero, m = oracle_step_check(f"lambda-{lam}", cfg, sd, x, y)
    qk = sorted(k for k in O.param_names(cfg) if "linears_Q_" in k or "linears_K_" in k)
    assert zero == (qk if lam == 1.0 else k_biases(cfg))
    got = grads_of(m)
    for k in zero:
        assert not got[k].any(), k


def test_more_samples_than_backward_workgroups():
    """bs = 260 > 256 partial rows: some workgroups of the backward accumulate two samples."""
    cfg, sd, x, y = seeded_case(items(make_cfg(3, 4, H=1, d=(3, 5), ff=(2, 3))), 260, 9)
    oracle_step_check("small-bs260", cfg, sd, x, y)


# ---- 4. dropout ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [SMALL[1], FULL[0]])
def test_training_with_dropout_matches_oracle(name):
    z, cfg, sd = load_case(name)
    bs, p = z["x"].shape[0], 0.1
    m = build_model(cfg, sd, dropout=p).train()
    keep = O.keep_masks(bs, cfg, m._seed, m._step + 1, p)
    assert all(0.8 < k.mean() < 0.97 for k in keep)
    o = O.forward_backward(sd, z["x"], z["y"], cfg, keep=keep, dropout_p=p)
    g32 = O.torch_grads(sd, z["x"], z["y"], cfg, torch.float32, keep, p)[2]
    x, y = dev(z["x"]), dev(z["y"])
    pred, loss = m.fused_mse_step(x, y)
    assert rel(o["pred"], z["pred"].reshape(-1)) > 10 * TOL                # the masks matter
    check_forward(name + "-dropout", m, bs, pred, loss, o, o["loss"])
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


# ---- 5. shards -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_two_shards_sum_to_the_full_batch(p):
    z, cfg, sd = load_case(SMALL[1])
    bs = z["x"].shape[0]
    x, y = dev(z["x"]), dev(z["y"])
    full = build_model(cfg, sd, dropout=p).train()
    keep = O.keep_masks(bs, cfg, full._seed, 1, p) if p else None
    o = O.forward_backward(sd, z["x"], z["y"], cfg, keep=keep, dropout_p=p)
    g32 = O.torch_grads(sd, z["x"], z["y"], cfg, torch.float32, keep, p)[2]
    full.fused_mse_step(x, y)
    total = torch.zeros_like(full.bucket)
    preds = []
    for lo, hi in ((0, bs // 2), (bs // 2, bs)):
        m = build_model(cfg, sd, dropout=p).train()
        m._seed = full._seed
        pred, _ = m.fused_mse_step(x[lo:hi], y[lo:hi], global_batch=bs, sample_offset=lo)
        preds.append(pred.clone())
        total += m.bucket
    assert rel(torch.cat(preds).cpu().numpy(), o["pred"]) < TOL                   # under dropout: the full batch's masks
    assert abs(float(total[full.num_live]) - o["loss"]) < TOL * o["loss"]
    assert abs(float(total[full.num_live]) - float(full.bucket[full.num_live])) < 1e-6 * o["loss"]
    check_grads(f"shards-p{p}", grads_of(full, total), o["grads"], g32, cfg)
    a, b = total[:full.num_live].cpu().numpy(), full.bucket[:full.num_live].cpu().numpy()
    assert np.abs(a - b).max() < 1e-5 * np.abs(b).max()


# ---- 6. fixed-order reductions ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_bs", [(FD, 5), (make_cfg(3, 4, H=1, d=(3, 5), ff=(2, 3)), 300)], ids=["fd-bs5", "small-bs300"])
def test_two_runs_give_the_same_bits(cfg_bs):
    cfg, sd, x, y = seeded_case(items(cfg_bs[0]), cfg_bs[1], 21)
    outs = []
    for _ in range(2):
        m = build_model(cfg, sd, dropout=0.1).train()
        m._seed = 99
        m.fused_mse_step(dev(x), dev(y))
        outs.append(m.bucket[:m.num_live + 1].clone())
    assert torch.isfinite(outs[0]).all() and outs[0].abs().max() > 0 and torch.equal(outs[0], outs[1])
    print("DVGT-GATE run-to-run: identical bits")


# ---- 7. the optimizer, the curve, the trainer ------------------------------------------------------------------------------------------
def test_fused_step_applies_adam_to_every_element_exactly_once():
    """The twin-model procedure of tests/test_fused_adam_families_gpu.py (bounds from tests/adam_reference.py), dropout on."""
    from gnn_rul_benchmarking_amd.optim import FusedAdam
    from test_fused_adam_families_gpu import LR, SEED, STEP0, WD, _bits, _np
    z, cfg, sd = load_case(SMALL[1])
    x, y = dev(z["x"]), dev(z["y"])

    def ready():
        m = build_model(cfg, sd, dropout=0.1).train()
        m._seed = SEED
        return m
    a = ready()
    p0 = _np(a.flat_params)
    _, loss_a = a.fused_mse_step(x, y)
    g_a, loss_a = _np(a.bucket[:a.num_live]), float(loss_a)
    assert np.isfinite(g_a).all() and np.array_equal(_bits(_np(a.flat_params)), _bits(p0))
    b = ready()
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
        r = R.check(after, before[0], g, before[1], before[2], k, WD, 1.0, what=f"DVGTformer, step {k}")
        worst = {q: max(worst[q], r[q]) for q in worst}
    assert opt._steps == STEP0 + 3
    print("ADAM-RATIO family DVGTformer: " + " ".join(f"{q}={worst[q]:.3f}" for q in "pmv"))


def test_training_curve_matches_reference_algorithm():
    """Twenty update() steps against the reference's own.  Tolerances: the project's curve tolerances for a BatchNorm-free family
    (GRU_CM, tests/test_grucm_gpu.py: the first three losses 1e-4, every loss 2e-3, the eval prediction at the end 5e-3)."""
    from gnn_rul_benchmarking_amd.algorithms import get_algorithm_class
    z, cfg, sd0 = load_case(CURVE, "sd0:")
    algo = get_algorithm_class("DVGTformer")(cfg, {"learning_rate": float(z["lr"]), "weight_decay": float(z["wd"])}, DEV)
    algo.model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd0.items()})
    algo.model.dropout_p = 0.0
    algo.to(DEV).train()
    xs, ys = torch.from_numpy(z["xs"]).to(DEV), torch.from_numpy(z["ys"]).to(DEV)
    losses = np.asarray([algo.update(xs[s], ys[s], 1)["loss"] for s in range(xs.size(0))])
    ref = z["losses"]
    print("DVGT-GATE curve: worst loss ratio", np.abs(losses / ref - 1).max())
    assert len(ref) == 20 and np.max(np.abs(losses[:3] - ref[:3]) / ref[:3]) < 1e-4
    assert np.max(np.abs(losses - ref) / ref) < 2e-3
    algo.eval()
    with torch.no_grad():
        assert rel(algo.model(xs[0]).cpu().numpy(), z["eval_pred_end"]) < 5e-3


def test_trainer_matches_reference_harness_run_on_cmapss(tmp_path, monkeypatch):
    """--GNN_method DVGTformer on C-MAPSS FD001 as the reference wires it: the reference's own harness, run on the CPU by
    tests/golden/make_golden_dvgtformer.py::case_trainer_cmapss with dropout switched off on the constructed model, vs this package's
    harness on the GPU with the same switch.  Bars: those of the other families' harness tests (tests/test_trainer_gpu.py)."""
    import sys
    sys.path.insert(0, GOLD)
    from synth import synthetic_cmapss
    from gnn_rul_benchmarking_amd import trainer as T
    z = np.load(os.path.join(GOLD, "dvgtformer_trainer_fd001_reference_run.npz"))
    (xtr, ytr), (xte, yte) = synthetic_cmapss(int(z["seed"]), int(z["n_train"]), int(z["n_test"]))
    assert abs(xtr.astype(np.float64).sum() - float(z["x_train_checksum"])) < 1e-6
    d = tmp_path / "data" / "CMAPSS" / "FD001"
    os.makedirs(d)
    torch.save({"samples": xtr, "labels": ytr, "max_ruls": 125}, d / "train.pt")
    torch.save({"samples": xte, "labels": yte, "max_ruls": 125}, d / "test.pt")
    monkeypatch.chdir(tmp_path)
    base = T.get_algorithm_class("DVGTformer")

    class NoDropout(base):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.model.dropout_p = 0.0
    monkeypatch.setattr(T, "get_algorithm_class", lambda n: NoDropout)
    args = argparse.Namespace(save_dir=str(tmp_path / "logs"), experiment_description="exp", run_description="r",
                              GNN_method="DVGTformer", data_path=str(tmp_path / "data"), dataset="CMAPSS",
                              dataset_id="FD001", bearing_id=None, num_runs=1, device=DEV)
    tr = T.GNN_RUL_trainer(args)
    tr.train_configs["num_epochs"] = int(z["epochs"])
    assert tr.train_configs["batch_size"] == int(z["batch_size"]) and tr.train_configs["learning_rate"] == float(z["lr"])
    assert tr.model_configs == FD
    per_epoch = []
    orig = tr.calc_results_per_run

    def spy(run_id):
        per_epoch.append(T._calc_metrics(tr.pred_labels, tr.true_labels, tr.max_ruls))
        return orig(run_id)
    tr.calc_results_per_run = spy
    tr.train()
    got, ref = np.asarray(per_epoch, np.float64), z["per_epoch"]
    print("DVGT harness per-epoch got/ref:\n", got, "\n", ref)
    assert got.shape == ref.shape == (int(z["epochs"]), 4)
    assert np.max(np.abs(got[:, 2:] - ref[:, 2:]) / np.abs(ref[:, 2:])) < 1e-3      # MAE, RMSE (in RUL cycles), relative
    assert np.max(np.abs(got[:, 3] - ref[:, 3]) / 125.0) < 1e-3                      # RMSE on the normalised scale, absolute
    sd = tr.algorithm.state_dict()
    for k in z.files:
        if k.startswith("final:"):
            a, b = sd["model." + k[6:]].cpu().numpy().astype(np.float64), z[k].astype(np.float64)
            assert np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30) < 3e-3, k


# ---- 8. coverage -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [make_cfg(25, 1), make_cfg(2, 57), make_cfg(2, 1, H=9), make_cfg(2, 1, nb=9), make_cfg(2, 1, ff=(129, 1)),
                                 make_cfg(2, 1, d=(1, 1025))], ids=["N25", "L57", "H9", "nb9", "ff129", "d1025"])
def test_just_outside_each_limit_is_not_covered_and_launches_nothing(cfg):
    from gnn_rul_benchmarking_amd.dvgtformer import DVGTformer_model
    m = DVGTformer_model(**cfg).to(DEV)
    x = torch.rand(2, cfg["num_nodes"], cfg["time_length"], device=DEV)
    with pytest.raises(RuntimeError, match="do not cover this configuration"):
        m(x)
    with pytest.raises(RuntimeError, match="do not cover this configuration"):
        m.fused_mse_step(x, torch.zeros(2, device=DEV))
    assert not m._bufs and not m.bucket.any()                  # no workspace was made, nothing was written
