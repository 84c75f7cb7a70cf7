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
import functools
import os

import numpy as np
import pytest
import torch

import family_kit as K
import grad_gate as GG
import dvgtformer_oracle as O
from family_kit import DEV, GOLD, dev, grads_of, rel_same_shape as rel
from test_dvgtformer_oracle_golden import CURVE, FULL, SMALL, load_case, oracle_of, seeded_state

pytestmark = pytest.mark.gpu
TOL, RTOL = 1e-4, 5e-4 / 2 ** 7
FD = dict(num_nodes=14, time_length=50, d_model=[144, 248], num_heads=4, lambda_param=0.5, d_ff=[72, 124], dropout=0.1, num_blocks=3)


def make_cfg(N, L, H=2, nb=1, lam=0.5, d=(6, 10), ff=(4, 6)):
    return dict(num_nodes=N, time_length=L, d_model=list(d), num_heads=H, lambda_param=lam, d_ff=list(ff), dropout=0.1, num_blocks=nb)


def build_model(cfg, sd, dropout=0.0):
    from gnn_rul_benchmarking_amd.dvgtformer import DVGTformer_model
    return K.build_model(DVGTformer_model, cfg, sd, dropout)


def k_weight_of(name):
    """The K weight of the head a Q / K tensor belongs to (the scale of the rounding residue a zero-in-exact-arithmetic tensor may hold)."""
    return name.replace("linears_Q_", "linears_K_").rsplit(".", 1)[0] + ".weight" if "linears_" in name else None


def k_weight_bound(name, g64, ref32):
    """Not exact zeros: at most the reference's own residue, or fp32 ulps of the head's K-weight gradient."""
    kw = k_weight_of(name)
    return 16 * max(np.abs(ref32[name]).max(), 2.0 ** -23 * (np.abs(g64[kw]).max() if kw else 0.0))


K_WEIGHT_RULE = K.ZeroRule(GG.zero_in_exact_arithmetic, k_weight_bound, lambda zero: f"; zero in exact arithmetic: {len(zero)} tensors")


def check_grads(what, got, g64, ref32, cfg):
    """Every tensor through the element-wise gate; returns the names detected as zero in exact arithmetic."""
    assert list(g64) == O.param_names(cfg)
    return K.check_grads(what, "DVGT", got, g64, ref32, RTOL, K_WEIGHT_RULE)


def k_biases(cfg):
    return sorted(k for k in O.param_names(cfg) if "linears_K_" in k and k.endswith(".bias"))


def check_forward(what, m, bs, pred, loss, want, want_loss):
    errs = {**K.tap_errs(m, bs, want, ("x0", "enc"), rel), **K.pred_err(pred, want, rel), **K.loss_err(loss, want_loss)}
    K.check_forward(what, "DVGT", errs, TOL)


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
    """The twin-model procedure (family_kit.adam_twin_check), dropout on."""
    z, cfg, sd = load_case(SMALL[1])
    K.adam_twin_check(lambda: build_model(cfg, sd, dropout=0.1).train(), dev(z["x"]), dev(z["y"]), "DVGTformer")


def test_training_curve_matches_reference_algorithm():
    """Twenty update() steps against the reference's own.  Tolerances: the project's curve tolerances for a BatchNorm-free family
    (GRU_CM, tests/test_grucm_gpu.py: the first three losses 1e-4, every loss 2e-3, the eval prediction at the end 5e-3)."""
    z, cfg, sd0 = load_case(CURVE, "sd0:")
    K.curve_check("DVGTformer", "DVGT", cfg, z, sd0, dict(steps=20, first3=1e-4, every=2e-3, eval=5e-3), dropout_off=True)


def test_trainer_matches_reference_harness_run_on_cmapss(tmp_path, monkeypatch):
    """--GNN_method DVGTformer on C-MAPSS FD001 as the reference wires it: the reference's own harness, run on the CPU by
    tests/golden/make_golden_dvgtformer.py::case_trainer_cmapss with dropout switched off on the constructed model, vs this package's
    harness on the GPU with the same switch.  Bars: those of the other families' harness tests (tests/test_trainer_gpu.py)."""
    z = np.load(os.path.join(GOLD, "dvgtformer_trainer_fd001_reference_run.npz"))

    def row(tr):
        assert tr.train_configs["batch_size"] == int(z["batch_size"]) and tr.train_configs["learning_rate"] == float(z["lr"])
        assert tr.model_configs == FD
    tr, per_epoch = K.harness_run(tmp_path, monkeypatch, "DVGTformer", "CMAPSS", "FD001", z, no_dropout=K.model_dropout_off, configure=row)
    K.assert_harness("DVGT", per_epoch, K.state_of(tr), z,        # MAE, RMSE (in RUL cycles), relative; RMSE on the normalised scale, absolute
                     dict(rmse_abs=1e-3, rmse_scale=125.0, rel=1e-3, rel_from=2, final=3e-3, final_prefix="model."))


# ---- 8. coverage -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [make_cfg(25, 1), make_cfg(2, 57), make_cfg(2, 1, H=9), make_cfg(2, 1, nb=9), make_cfg(2, 1, ff=(129, 1)),
                                 make_cfg(2, 1, d=(1, 1025))], ids=["N25", "L57", "H9", "nb9", "ff129", "d1025"])
def test_just_outside_each_limit_is_not_covered_and_launches_nothing(cfg):
    from gnn_rul_benchmarking_amd.dvgtformer import DVGTformer_model
    K.refused_outside_limits(DVGTformer_model(**cfg), torch.rand(2, cfg["num_nodes"], cfg["time_length"], device=DEV))
