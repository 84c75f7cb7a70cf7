"""HierCorrPool HIP path vs the reference's golden outputs and vs the fp64 oracle (GPU).

Gates.  Predictions, taps, the loss and the BatchNorm running statistics after a step: TOL = 1e-4 relative to the tensor's largest
value, the bar of the other families.  Gradients: element by element through tests/grad_gate.py at rtol 5e-4 and margin 16; the floor's
noise term is the REFERENCE's fp32 gradient against the fp64 oracle (the fixture's ``refgrad:`` entries; without a fixture an fp32 run
of the torch restatement on the CPU), never the kernels' output.  ``matrix.bias`` (constant along the softmax axis) must be exactly 0.
Every test prints its worst gate ratio ("HCP-GATE ...")."""
import functools
import os

import numpy as np
import pytest
import torch

import adam_reference as R
import family_kit as K
import hiercorrpool_oracle as O
from family_kit import DEV, GOLD, grads_of, rel_same_shape as rel
from oracle import stgcn_oracle as SO
from test_hiercorrpool_oracle_golden import CASES, CURVE, load_case

pytestmark = pytest.mark.gpu
TOL, RTOL = 1e-4, 5e-4
TAPS = ("encoder", "pooled_x", "pooled_adj", "H")
KEYS = "patch_size num_patch input_dim hidden_dim embedding_dim num_nodes encoder_conv_kernel num_nodes_out".split()


def make_cfg(p, P, N, h, e, K, M):
    return dict(patch_size=p, num_patch=P, input_dim=10, hidden_dim=h, embedding_dim=e, num_nodes=N, encoder_conv_kernel=K, num_nodes_out=M)


FD001, FD004, NCMAPSS = make_cfg(25, 2, 14, 10, 10, 8, 6), make_cfg(10, 5, 14, 10, 10, 12, 6), make_cfg(1, 50, 20, 10, 10, 32, 6)


def build_model(cfg, sd, dropout=0.0):
    from gnn_rul_benchmarking_amd.hiercorrpool import HierCorrPool_model
    return K.build_model(HierCorrPool_model, cfg, sd, dropout, KEYS)


def seeded_state(cfg, seed):
    """The state dict the constructor gives under ``seed`` (numpy)."""
    from gnn_rul_benchmarking_amd.hiercorrpool import HierCorrPool_model
    torch.manual_seed(seed)
    return {k: v.numpy().copy() for k, v in HierCorrPool_model(**{k: cfg[k] for k in KEYS}).state_dict().items()}


def check_grads(what, got, g64, ref32):
    """Every tensor's ratio is printed; ``matrix.bias`` (constant along the softmax axis) must be exactly zero."""
    K.check_grads(what, "HCP", got, g64, ref32, RTOL, exact_zero=(O.ZERO_GRAD,), verbose=True)


def check_forward(what, m, bs, pred, loss, want, want_loss, running=None):
    errs = {**K.tap_errs(m, bs, want, TAPS, rel), **K.pred_err(pred, want, rel), **K.loss_err(loss, want_loss)}
    if running is not None:
        sd = m.state_dict()
        for k, v in running.items():
            errs[k.split("conv_")[1]] = rel(sd[k].cpu().numpy(), v)
    K.check_forward(what, "HCP", errs, TOL)


@functools.lru_cache(maxsize=None)
def fixture_oracle(name):
    z, cfg, sd = load_case(name)
    loss, g, fw = O.loss_and_grads(sd, z["x"], z["y"], cfg)
    return z, cfg, sd, loss, g, fw


# ---- 1. the reference's fixtures ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_fixture_forward_taps_statistics_and_gradients(name):
    z, cfg, sd, loss64, g64, fw = fixture_oracle(name)
    m = build_model(cfg, sd).train()
    x, y = torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(z["y"]).to(DEV)
    bs = x.size(0)
    pred, loss = m.fused_mse_step(x, y)
    running = {k[9:]: z[k] for k in z.files if k.startswith("bn_after:") and "running" in k}
    check_forward(name, m, bs, pred, loss, {**{t: z[t] for t in TAPS}, "pred": z["pred"]}, float(z["loss"]), running)
    assert int(m.state_dict()[O.ENC.format(2) + "1.num_batches_tracked"]) == 1
    check_grads(name, grads_of(m), g64, {k: z["refgrad:" + k] for k in O.param_names()})
    m.eval()
    with torch.no_grad():
        ev = m(x)
    want = O.forward({k: v.cpu().numpy() for k, v in m.state_dict().items()}, z["x"], cfg, training=False)["pred"]
    assert ev.shape == (bs, 1) and rel(ev.cpu().numpy(), want) < TOL


# ---- 2. full width against the fp64 oracle ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def seeded_case(tag, bs, seed):
    cfg = {"fd001": FD001, "fd004": FD004, "ncmapss": NCMAPSS}[tag]
    sd = seeded_state(cfg, seed)
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, (bs, cfg["num_nodes"], cfg["num_patch"] * cfg["patch_size"])).astype(np.float32)
    y = rng.uniform(0, 1, bs).astype(np.float32)
    return cfg, sd, x, y


@pytest.mark.parametrize("tag,bs", [("fd001", 8), ("fd004", 5), ("ncmapss", 3), ("fd001", 1)])
def test_full_width_step_matches_oracle(tag, bs):
    cfg, sd, x, y = seeded_case(tag, bs, 100 + bs)
    loss64, g64, fw = O.loss_and_grads(sd, x, y, cfg)
    _, _, g32 = O.torch_grads(sd, x, y, cfg, torch.float32)
    m = build_model(cfg, sd).train()
    pred, loss = m.fused_mse_step(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV))
    what = f"{tag}-full-bs{bs}"
    check_forward(what, m, bs, pred, loss, fw, loss64, O.running_after(sd, fw))
    check_grads(what, grads_of(m), g64, g32)


# ---- 3. dropout ------------------------------------------------------------------------------------------------------------------------
def keep_mask(bs, C1, L1, seed, step, p, offset=0):
    """The kernels' dropout mask behind block 1, restated: element counter ((offset + b) C1 + c) L1 + t over [b][c][t]."""
    ctr = (np.arange(bs * C1 * L1, dtype=np.uint64) + np.uint64(offset * C1 * L1)).astype(np.uint32)
    key = SO.dropout_layer_key(seed, step, 0)
    with np.errstate(over="ignore"):
        keep = SO._lowbias32(ctr ^ np.uint32(key)) >= np.uint32(SO.dropout_threshold(p))
    return keep.reshape(bs, C1, L1).astype(np.float64)


@pytest.mark.parametrize("name", ["hiercorrpool_small_7x3_n5_bs6", "hiercorrpool_fd004geom_bs4"])
def test_training_with_dropout_matches_oracle(name):
    z, cfg, sd = load_case(name)
    bs, C1, L1 = z["x"].shape[0], cfg["hidden_dim"] * cfg["num_nodes"], O.lengths(cfg["num_patch"])[0]
    m = build_model(cfg, sd, dropout=0.35).train()
    keep = keep_mask(bs, C1, L1, m._seed, m._step + 1, 0.35)
    assert 0.4 < keep.mean() < 0.9
    loss64, g64, fw = O.loss_and_grads(sd, z["x"], z["y"], cfg, keep_mask=keep)
    _, _, g32 = O.torch_grads(sd, z["x"], z["y"], cfg, torch.float32, keep_scale=(keep / 0.65).astype(np.float32))
    x, y = torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(z["y"]).to(DEV)
    pred, loss = m.fused_mse_step(x, y)
    check_forward(name + "-dropout", m, bs, pred, loss, fw, loss64)
    check_grads(name + "-dropout", grads_of(m), g64, g32)
    # a shard that starts at global sample 3 draws rows 3... of the unsharded mask
    assert np.array_equal(keep_mask(bs - 3, C1, L1, m._seed, 1, 0.35, offset=3), keep_mask(bs, C1, L1, m._seed, 1, 0.35)[3:])
    m2 = build_model(cfg, sd, dropout=0.35).train()
    m2._seed = m._seed
    m2.fused_mse_step(x[3:], y[3:], sample_offset=3)
    sh = O.forward(sd, z["x"][3:], cfg, True, keep[3:])         # (batch statistics of the shard, the whole batch's mask rows)
    assert rel(m2.tap(bs - 3, "encoder").cpu().numpy(), sh["encoder"]) < TOL


# ---- 4. path equalities ------------------------------------------------------------------------------------------------------------
def _case(name=CASES[0]):
    z, cfg, sd = load_case(name)
    return cfg, sd, torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(z["y"]).to(DEV)


@pytest.mark.parametrize("name", [CASES[0], CASES[3]])
def test_forward_then_backward_equals_fwdbwd_bit_for_bit(name):
    cfg, sd, x, y = _case(name)
    m = build_model(cfg, sd, dropout=0.35).train()
    m.fused_mse_step(x, y)
    fused = m.bucket[:m.num_live + 1].clone()
    assert not fused[m._layout[O.ZERO_GRAD][0]:m._layout[O.ZERO_GRAD][0] + cfg["num_nodes_out"]].any()
    m._step = 0
    m.fused_mse_step(x, y)
    assert torch.equal(m.bucket[:m.num_live + 1], fused)                      # twice the same step: the same bits
    m2 = build_model(cfg, sd, dropout=0.35).train()
    m2._seed = m._seed
    x2, yv = m2._step_inputs(x, y)
    shp = m2._shape(x2.size(0))
    a = m2._args(shp, x2, True, 1, y=yv)
    m2._call("forward", shp, a)
    m2._call("backward", shp, a)
    assert torch.equal(m2.bucket[:m2.num_live + 1], fused)


def test_autograd_path_equals_fused_path_and_update_reference_style_equals_update():
    from gnn_rul_benchmarking_amd.algorithms import get_algorithm_class
    cfg, sd, x, y = _case()
    m = build_model(cfg, sd).train()
    m.fused_mse_step(x, y)
    fused = m._grad_flat[:m.num_live].clone()
    m2 = build_model(cfg, sd).train()
    torch.nn.functional.mse_loss(m2(x), y).backward()
    auto = torch.cat([t.grad.reshape(-1) for t in m2._named()])
    assert torch.equal(auto, fused)
    assert torch.equal(m2._bn, m._bn) and int(m2.state_dict()[O.ENC.format(1) + "1.num_batches_tracked"]) == 1
    algos = []
    for _ in range(2):
        algo = get_algorithm_class("HierCorrPool")({k: cfg[k] for k in KEYS}, {"learning_rate": 1e-3, "weight_decay": 1e-4}, DEV)
        algo.model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
        algo.model.dropout_p = 0.0
        algos.append(algo.to(DEV).train())
    la = algos[0].update(x, y, 1)["loss"]
    lb = algos[1].update_reference_style(x, y, 1)["loss"]
    assert abs(la - lb) <= 1e-6 * abs(la)
    sa, sb = algos[0].state_dict(), algos[1].state_dict()
    for k in sa:
        assert rel(sb[k].cpu().numpy(), sa[k].cpu().numpy()) < 1e-6, k       # one Adam step from the same gradient bits
    assert not torch.equal(sa["model.fc_0.weight"].cpu(), torch.from_numpy(np.asarray(sd["fc_0.weight"])))


# ---- 5. training curve -----------------------------------------------------------------------------------------------------------------
def test_training_curve_matches_reference_algorithm():
    """Twelve update() steps against the reference's own.  Tolerances: the project's curve tolerances for BatchNorm families
    (tests/test_stagnn_gpu.py:144-150: losses rtol 2e-3, end state and eval prediction 5e-3)."""
    z, cfg, sd0 = load_case(CURVE, "sd0:")
    _, sd = K.curve_check("HierCorrPool", "HCP", {k: cfg[k] for k in KEYS}, z, sd0, dict(steps=12, first3=None, every=2e-3, params=5e-3, eval=5e-3),
                          dropout_off=True)
    assert list(sd) == O.state_keys()
    # matrix.bias has no gradient: twelve steps of Adam on wd * p alone, which is what the reference's ~1e-10 of noise amounts to as well
    b0, b1 = np.asarray(sd0[O.ZERO_GRAD], np.float64), sd[O.ZERO_GRAD].cpu().numpy().astype(np.float64)
    p, mm, vv = b0, np.zeros_like(b0), np.zeros_like(b0)
    for k in range(1, 13):
        p, mm, vv = R.reference(p, np.zeros_like(b0), mm, vv, k, float(z["lr"]), 0.9, 0.999, 1e-8, float(z["wd"]), 1.0)
    assert np.abs(b1 - p).max() <= 1e-6 * np.abs(b0).max() + 12 * 2.0 ** -24 * np.abs(b0).max()


# ---- 6. the optimizer inside the fused step -----------------------------------------------------------------------------------------
def test_fused_step_applies_adam_to_every_element_exactly_once():
    """The twin-model procedure (family_kit.adam_twin_check: steps 7-9), dropout on."""
    z, cfg, sd = load_case(CASES[0])
    b = K.adam_twin_check(lambda: build_model(cfg, sd, dropout=0.35).train(), torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(z["y"]).to(DEV),
                          "HierCorrPool")
    assert int(b.state_dict()[O.ENC.format(3) + "1.num_batches_tracked"]) == 3


# ---- 7. coverage ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [make_cfg(1, 2, 33, 1, 1, 8, 1), make_cfg(1, 2, 4, 1, 1, 8, 17), make_cfg(1, 65, 4, 1, 1, 40, 2), make_cfg(65, 2, 4, 1, 1, 8, 2),
                                 make_cfg(1, 2, 2, 65, 65, 8, 2), make_cfg(1, 2, 32, 9, 9, 8, 2)],
                         ids=["N33", "M17", "P65", "p65", "d520", "C3-1152"])
def test_just_outside_each_limit_is_not_covered_and_launches_nothing(cfg):
    from gnn_rul_benchmarking_amd.hiercorrpool import HierCorrPool_model
    K.refused_outside_limits(HierCorrPool_model(**cfg), torch.zeros(2, cfg["num_nodes"], cfg["num_patch"] * cfg["patch_size"], device=DEV))


@pytest.mark.parametrize("cfg", [make_cfg(1, 2, 32, 1, 1, 8, 16), make_cfg(1, 2, 4, 64, 64, 8, 16), make_cfg(1, 64, 32, 8, 8, 40, 16)],
                         ids=["N32-M16", "d512-M16", "N32-M16-d320-P64"])
def test_just_inside_the_limits_matches_oracle(cfg):
    """N = 32 and M = 16 together; d = 512 (C3 <= 1024 leaves N = 4 beside it); and the widest d that N = 32 allows, at P = 64."""
    bs = 2
    sd = seeded_state(cfg, 7)
    rng = np.random.default_rng(7)
    x = rng.uniform(0, 1, (bs, cfg["num_nodes"], cfg["num_patch"] * cfg["patch_size"])).astype(np.float32)
    y = rng.uniform(0, 1, bs).astype(np.float32)
    loss64, g64, fw = O.loss_and_grads(sd, x, y, cfg)
    _, _, g32 = O.torch_grads(sd, x, y, cfg, torch.float32)
    m = build_model(cfg, sd).train()
    pred, loss = m.fused_mse_step(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV))
    what = "limits-" + "-".join(str(cfg[k]) for k in KEYS)
    check_forward(what, m, bs, pred, loss, fw, loss64, O.running_after(sd, fw))
    check_grads(what, grads_of(m), g64, g32)


# ---- 8. trainer ------------------------------------------------------------------------------------------------------------------------
def test_trainer_matches_reference_harness_run_on_cmapss(tmp_path, monkeypatch):
    """--GNN_method HierCorrPool on C-MAPSS FD001 as the reference wires it (configs/hparams.py:17,35; shuffling DataLoader): the
    reference's own harness, run on the CPU by tests/golden/make_golden_hiercorrpool.py::case_trainer_cmapss with the encoder's dropout
    switched off on the constructed model, vs this package's harness on the GPU with the same switch.  Bars: those of the other
    families' harness tests (tests/test_trainer_gpu.py)."""
    z = np.load(os.path.join(GOLD, "hiercorrpool_trainer_fd001_reference_run.npz"))
    assert int(z["epochs"]) == 3

    def row(tr):
        assert tr.train_configs["batch_size"] == int(z["batch_size"]) and tr.train_configs["learning_rate"] == float(z["lr"])
        assert tr.model_configs == FD001
    tr, per_epoch = K.harness_run(tmp_path, monkeypatch, "HierCorrPool", "CMAPSS", "FD001", z, no_dropout=K.model_dropout_off, configure=row)
    K.assert_harness("HierCorrPool", per_epoch, K.state_of(tr), z,   # MAE, RMSE (in RUL cycles), relative; RMSE on the normalised scale, absolute
                     dict(rmse_abs=1e-3, rmse_scale=125.0, rel=1e-3, rel_from=2, final=3e-3, final_prefix=""))
