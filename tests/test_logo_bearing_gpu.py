"""LOGO_bearing HIP path vs the reference's golden outputs and vs the fp64 oracle (GPU).

Gates (LOGO's, tests/test_logo_gpu.py: it is the same stack behind another front end).  Predictions, taps, L_GL and the loss:
TOL = 1e-4 relative to the tensor's largest value.  Gradients: element by element through tests/grad_gate.py at rtol 5e-4 and margin 16;
the floor's noise term is the REFERENCE's fp32 gradient against the fp64 oracle (the fixture's ``refgrad:`` entries; without a fixture an
fp32 run of the torch restatement, ``torch.stft`` included, on the CPU), never the kernels' output.  A tensor whose gradient is zero in
exact arithmetic (the twelve fusion tensors at two nodes) has no magnitude of its own: it is held to the margin times one fp32 ulp of the
model's largest gradient element, or the reference's own residue if that is larger.  Every test prints its worst gate ratio
("LOGOB-GATE ...").

Worst gradient gate ratios on an MI355X (1 passes; profiles/r28_logo_bearing.md): tiny shape 0.037 (bs 3 fixture), 0.014 / 0.139 / 0.006
(bs 1 / 2 / 257); nperseg 2: 0.027; patch_size no multiple of nperseg: 0.123 (0.057 with dropout); T = 1: 0.038; PHM2012 and XJTU_SY at
full width: 0.072 each (fc.fc1.weight).  Forward: 1.14e-6 at worst (PHM2012, lstm) against TOL."""
import functools

import numpy as np
import pytest
import torch

import family_kit as K
import grad_gate as GG
import logo_bearing_oracle as O
from family_kit import DEV, grads_of, rel_same_shape as rel
from test_logo_bearing_oracle_golden import CASES, CURVE, SMALL, fixture_oracle, fusion_is_constant, load_case, seeded_state
from test_logo_gpu import check_forward as logo_check_forward

pytestmark = pytest.mark.gpu
TOL, RTOL = 1e-4, 5e-4
KEYS = O.KEYS
TINY = dict(patch_size=8, num_patch=2, input_dim=3, num_nodes=3, nperseg=4, hidden_dim=1)


def build_model(cfg, sd, dropout=0.0):
    from gnn_rul_benchmarking_amd.logo_bearing import LOGO_bearing_model
    return K.build_model(LOGO_bearing_model, cfg, sd, dropout, KEYS)


def check_grads(what, cfg, got, g64, ref32):
    worst = (0.0, None)
    gmax = max(float(np.abs(v).max()) for v in g64.values())
    zero = fusion_is_constant(cfg)
    for k in O.param_names():
        if not g64[k].any():              # exactly zero in the oracle (bs = 1: a one-step recurrence has h_prev = 0, so g weight_hh = 0)
            assert got[k].shape == g64[k].shape and not got[k].any() and not np.asarray(ref32[k]).any(), f"{k} must be exactly zero"
            continue
        floor = GG.floor_for(ref32[k], g64[k])
        if k in zero:
            floor = max(floor, GG.MARGIN * 2.0 ** -23 * gmax)
        ratio, where = GG.gate(got[k], g64[k], RTOL, floor)
        print(f"  grad {k}: gate {ratio:.3f} at {where}  max|g| {np.abs(g64[k]).max():.2e}")
        worst = max(worst, (ratio, k))
    print(f"LOGOB-GATE {what}: worst gradient gate ratio {worst[0]:.3f} ({worst[1]})")
    assert worst[0] <= 1.0, worst


def check_forward(what, m, bs, pred, loss, want, want_loss):
    logo_check_forward(what, m, bs, pred, loss, want, want_loss, tag="LOGOB")


# ---- 1. the reference's fixtures: the tiny shapes and both reference geometries at full width -----------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_fixture_forward_taps_loss_and_gradients(name):
    z, cfg, sd, loss64, g64, fw = fixture_oracle(name)
    theta = float(z["theta"])
    m = build_model(cfg, sd).train()
    x, y = torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(z["y"]).to(DEV)
    bs = x.size(0)
    pred, loss = m.fused_mse_step(x, y, theta=theta)
    ref = {"mpnn": z["mpnn"], "lstm": z["lstm"], "gl": float(z["loss_gl"]), "pred": z["pred"]}
    check_forward(name, m, bs, pred, loss, ref, float(z["loss"]))                  # against the reference itself ...
    check_forward(name + "-oracle", m, bs, pred, loss, fw, loss64)                 # ... and the fp64 oracle
    check_grads(name, cfg, grads_of(m), g64, {k: z["refgrad:" + k] for k in O.param_names()})
    m.eval()
    with torch.no_grad():
        ev, gl = m(x.reshape(bs, 1, -1), GL=True)                                  # (any shape with numel / bs == num_patch * patch_size)
    assert ev.shape == (bs, 1) and gl.dim() == 0
    assert rel(ev.cpu().numpy(), z["pred_eval"]) < TOL and abs(float(gl) - float(z["loss_gl"])) < TOL * float(z["loss_gl"])


# ---- 2. the tiny shape at other batch sizes, against the fp64 oracle ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def seeded_case(bs, seed):
    """Weights, inputs and targets of the tiny shape under ``seed``, advanced until at least half of the samples reach the prediction
    through an open ReLU of fc1 and of fc2; with the oracle's step and the fp32 restatement's gradients.  Never modified."""
    cfg = dict(TINY)
    while True:
        sd = seeded_state(cfg, seed)
        rng = np.random.default_rng(seed)
        x = rng.standard_normal((bs, cfg["num_patch"] * cfg["patch_size"])).astype(np.float32)
        y = rng.uniform(0, 1, bs).astype(np.float32)
        fw = O.forward(sd, x, cfg)
        if 2 * int(((fw["pre1"] > 0).any(1) & (fw["pre2"] > 0).any(1)).sum()) >= bs:
            break
        seed += 1
    loss64, g64, fw = O.loss_and_grads(sd, x, y, cfg, 0.01)
    _, _, g32 = O.torch_grads(sd, x, y, cfg, 0.01, torch.float32)
    return cfg, sd, x, y, loss64, g64, fw, g32


@pytest.mark.parametrize("bs", [1, 2, 257])
def test_tiny_shape_step_matches_oracle(bs):
    """bs 1 (a one-step recurrence) and 2 beside the fixture's 3; bs 257: the backward's 256 partial rows wrap (workgroup 0 accumulates
    two samples in its registers and its LDS row) and so does every grid stride of the chain that is capped at or below 256."""
    cfg, sd, x, y, loss64, g64, fw, g32 = seeded_case(bs, 300 + bs)
    m = build_model(cfg, sd).train()
    pred, loss = m.fused_mse_step(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV), theta=0.01)
    check_forward(f"tiny-bs{bs}", m, bs, pred, loss, fw, loss64)
    check_grads(f"tiny-bs{bs}", cfg, grads_of(m), g64, g32)


# ---- 3. dropout, determinism ---------------------------------------------------------------------------------------------------------------
def test_train_forward_with_dropout_is_bit_equal_across_two_runs_and_matches_the_oracle():
    z, cfg, sd = load_case(SMALL[2])
    bs, theta = z["x"].shape[0], float(z["theta"])
    x, y = torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(z["y"]).to(DEV)
    outs = []
    for _ in range(2):
        torch.manual_seed(1234)
        m = build_model(cfg, sd, dropout=0.2).train()
        with torch.no_grad():
            pred, gl = m(x, GL=True)
        outs.append((pred.clone(), gl.clone(), m.tap(bs, "lstm")))
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    m._step = 0
    keep = O.keep_masks(bs, cfg, m._seed, 1, 0.2)
    loss64, g64, fw = O.loss_and_grads(sd, z["x"], z["y"], cfg, theta, keep_mask=keep)
    assert rel(fw["pred"], z["pred"]) > 10 * TOL                          # the masks matter
    assert rel(outs[0][0].cpu().numpy(), fw["pred"]) < TOL
    pred, loss = m.fused_mse_step(x, y, theta=theta)
    fused = m.bucket[:m.num_live + 1].clone()
    check_forward("ragged-dropout", m, bs, pred, loss, fw, loss64)
    _, _, g32 = O.torch_grads(sd, z["x"], z["y"], cfg, theta, torch.float32, keep_scale=tuple((k / 0.8).astype(np.float32) for k in keep))
    check_grads("ragged-dropout", cfg, grads_of(m), g64, g32)
    m._step = 0
    m.fused_mse_step(x, y, theta=theta)
    assert torch.equal(m.bucket[:m.num_live + 1], fused)                  # twice the same step: the same bits


# ---- 4. training curve: the scheduler steps once per update --------------------------------------------------------------------------------
def test_training_curve_and_learning_rates_match_reference_algorithm():
    """28 update() steps against the reference's own LOGO_bearing.update, whose MultiStepLR([5, 10, 20, 25], 0.5) steps per update: the
    optimizer's rate behind every step equals the recorded one (a constant rate, or one stepped per epoch, fails at step 5).  Tolerances:
    those of tests/test_logo_gpu.py's curve (the first three losses 1e-4, every loss 2e-3, end state and eval prediction 5e-3)."""
    from gnn_rul_benchmarking_amd.algorithms import LOGO_bearing
    z, cfg, sd0 = load_case(CURVE, "sd0:")
    algo = LOGO_bearing({k: cfg[k] for k in KEYS}, {"learning_rate": float(z["lr"]), "weight_decay": float(z["wd"]),
                                                                              "theta": float(z["theta"])}, DEV)
    algo.model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd0.items()})
    algo.model.dropout_p = 0.0
    algo.to(DEV).train()
    xs, ys = torch.from_numpy(z["xs"]).to(DEV), torch.from_numpy(z["ys"]).to(DEV)
    assert xs.size(0) == 28
    losses, lrs = [], []
    for s in range(28):
        losses.append(algo.update(xs[s], ys[s], 1)["loss"])               # (epoch 1 throughout: the schedule does not look at it)
        lrs.append(algo.optimizer.param_groups[0]["lr"])
    losses, ref = np.asarray(losses), z["losses"]
    print("LOGOB-GATE curve: worst loss ratio", np.abs(losses / ref - 1).max(), "rates", sorted(set(lrs), reverse=True))
    assert np.allclose(lrs, z["lrs"], rtol=1e-12, atol=0), (lrs, z["lrs"])
    assert np.max(np.abs(losses[:3] - ref[:3]) / ref[:3]) < 1e-4
    assert np.max(np.abs(losses - ref) / ref) < 2e-3
    sd = algo.model.state_dict()
    assert list(sd) == O.state_keys()
    for k in sd:
        assert rel(sd[k].cpu().numpy(), z["sd_end:" + k]) < 5e-3, k
    algo.eval()
    with torch.no_grad():
        assert rel(algo.model(xs[0]).cpu().numpy(), z["eval_pred_end"]) < 5e-3


def test_update_reference_style_steps_the_scheduler_too_and_equals_update():
    from gnn_rul_benchmarking_amd.algorithms import LOGO_bearing
    z, cfg, sd0 = load_case(CURVE, "sd0:")
    x, y = torch.from_numpy(z["xs"][0]).to(DEV), torch.from_numpy(z["ys"][0]).to(DEV)
    algos = []
    for _ in range(2):
        algo = LOGO_bearing({k: cfg[k] for k in KEYS}, {"learning_rate": 1e-3, "weight_decay": 1e-4, "theta": 0.01}, DEV)
        algo.model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd0.items()})
        algo.model.dropout_p = 0.0
        algos.append(algo.to(DEV).train())
    for _ in range(5):
        la = algos[0].update(x, y, 1)["loss"]
        lb = algos[1].update_reference_style(x, y, 1)["loss"]
        assert abs(la - lb) <= 1e-5 * abs(la)
    assert algos[0].optimizer.param_groups[0]["lr"] == algos[1].optimizer.param_groups[0]["lr"] == 5e-4
    sa, sb = algos[0].state_dict(), algos[1].state_dict()
    for k in sa:
        assert rel(sb[k].cpu().numpy(), sa[k].cpu().numpy()) < 1e-5, k


# ---- 5. coverage -----------------------------------------------------------------------------------------------------------------------
def _cfg(P, T, ns, h, **over):
    return dict(dict(patch_size=P, num_patch=T, input_dim=1 + P // ns, num_nodes=ns // 2 + 1, nperseg=ns, hidden_dim=h), **over)


@pytest.mark.parametrize("cfg", [_cfg(64, 1, 34, 1), _cfg(68, 1, 2, 1), _cfg(8, 1, 4, 22), _cfg(1024, 46, 32, 1), _cfg(8, 1, 3, 1),
                                 _cfg(2, 1, 4, 1)], ids=["N18", "f35", "6h132", "lds", "odd-nperseg", "short-patch"])
def test_just_outside_each_limit_is_not_covered_and_launches_nothing(cfg):
    from gnn_rul_benchmarking_amd.logo_bearing import LOGO_bearing_model
    K.refused_outside_limits(LOGO_bearing_model(**cfg), torch.randn(2, cfg["num_patch"] * cfg["patch_size"], device=DEV), theta=0.01)


def test_kwargs_that_do_not_describe_the_stft_fail_at_the_first_forward_naming_both():
    from gnn_rul_benchmarking_amd.logo_bearing import LOGO_bearing_model
    m = LOGO_bearing_model(**_cfg(8, 2, 4, 1, num_nodes=4, input_dim=2)).to(DEV)          # constructs, as the reference does
    with pytest.raises(RuntimeError, match="3 frequency bins of 3 frames.*num_nodes 4 and input_dim 2"):
        m(torch.randn(2, 16, device=DEV))
    assert not m._bufs
