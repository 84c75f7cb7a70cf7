"""GAT_LSTM HIP path vs the reference's golden outputs and vs the fp64 oracle (GPU).

Gates.  Predictions, taps and the loss: TOL = 1e-4 relative to the tensor's largest value, the project's forward gate; ``feat`` must be
NaN exactly where the expected one is.  Every fixture holds every tap and all 22 gradients of the reference's fp64 run, and the kernels
are gated against those.  Gradients: element by element through tests/grad_gate.py at RTOL and margin 16.  The floor's noise term is the
REFERENCE's fp32 gradient against the fp64 oracle (the fixture's ``refgrad:`` entry where it holds one, else an fp32 run of the torch
restatement on the CPU), never the kernels' output.  RTOL starts at
5e-4, the starting gate of every family, and is halved while the worst ratio of every case stays below 0.5 on an MI355X (the rule LOGO,
DVGTformer and GDAGDL were given); every case prints its worst ratio along that ladder ("GATLSTM-LADDER ...").
Measured over the 36 gradient checks of this file on an MI355X, worst ratio per RTOL: 0.271 from 5e-4 down to 5e-4 / 2^3 (edge-T2-P4), then
0.282, 0.299, 0.308, 0.330, 0.421 at the next five halvings, 0.488 at 5e-4 / 2^9 = 9.765625e-7 (edge-T3-P2048), 0.530 at 5e-4 / 2^10:
RTOL is 5e-4 / 2^9 = 9.765625e-7, eight fp32 ulps (profiles/r27_gatlstm.md).
Tensors whose gradient is zero in exact arithmetic are detected (grad_gate.zero_in_exact_arithmetic), not listed, and held to the rule
GDAGDL uses: at most 16 times the reference's own residue, or fp32 ulps of the model's largest gradient."""
import functools
import io
import json
import os

import numpy as np
import pytest
import torch

import family_kit as K
import gatlstm_oracle as O
from family_kit import DEV, GOLD, dev, grads_of, rel, rel_finite
from test_gatlstm_oracle_golden import CURVE, FULL, NAN, SMALL, load_case, oracle_run, seeded_weights

pytestmark = pytest.mark.gpu
TOL, RTOL = 1e-4, 5e-4 / 2 ** 9
LADDER = [5e-4 / 2 ** k for k in range(13)]


def make_cfg(T, P, widths, lstm=(3, 2), dropout=0.2):
    return dict(num_patch=T, patch_size=P, hidden_dim=list(widths), lstm_hidden_dim=list(lstm), dropout=dropout)


TINY = make_cfg(3, 4, [5, 4, 3])


def build_model(cfg, sd, dropout=0.0):
    from gnn_rul_benchmarking_amd.gatlstm import GAT_LSTM_model
    return K.build_model(GAT_LSTM_model, cfg, sd, dropout)


def check_grads(what, got, g64, ref32):
    """Every tensor through the element-wise gate.  Returns the names detected as zero in exact arithmetic (family_kit.residue_bound)."""
    return K.check_grads(what, "GATLSTM", got, g64, ref32, RTOL, K.RESIDUE, noise_partner=O.noise_partner, ladder=LADDER)


def check_forward(what, m, bs, pred, loss, want, want_loss):
    taps = [k for k in ["feat", "lstm"] + [f"h{l}" for l in range(len(m.hidden_dim))] if k in want]
    errs = {**K.pred_err(pred, want, rel_finite), **K.tap_errs(m, bs, want, taps, rel_finite, same_shape=False),      # NaN exactly where the expected one is
            **(K.loss_err(loss, want_loss) if np.isfinite(want_loss) else {})}
    K.check_forward(what, "GATLSTM", errs, TOL)


def fixture_grads(name):
    """(the reference's fp64 gradients, its fp32 gradients): all 22 tensors of a fixture."""
    z, cfg, _ = load_case(name)
    names = O.param_names(cfg)
    return {k: z["grad64:" + k] for k in names}, {k: z["refgrad:" + k] for k in names}


# ---- 1. the reference's fixtures ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL + FULL)
def test_fixture_forward_taps_loss_and_gradients(name):
    z, cfg, sd = load_case(name)
    o = oracle_run(name)
    m = build_model(cfg, sd).train()
    x, y = dev(z["x"]), dev(z["y"])
    bs = x.size(0)
    pred, loss = m.fused_mse_step(x, y)
    ref = {k[4:]: z[k] for k in z.files if k.startswith("tap:")}
    ref["pred"] = z["pred"]
    assert sorted(ref) == sorted(["pred", "feat", "lstm"] + [f"h{l}" for l in range(len(cfg["hidden_dim"]))])
    check_forward(name, m, bs, pred, loss, ref, float(z["loss"]))                # against the reference itself, every tap ...
    check_forward(name + "-oracle", m, bs, pred, loss, o, o["loss"])             # ... and the fp64 oracle
    g64, g32 = fixture_grads(name)
    check_grads(name, grads_of(m), g64, g32)                                     # all 22 against the reference's own
    fused = m.bucket[:m.num_live].clone()
    m.eval()
    with torch.no_grad():
        ev = m(x)
    assert ev.shape == (bs, 1) and rel(ev.cpu().numpy(), z["pred_eval"]) < TOL
    if name in SMALL:
        m2 = build_model(cfg, sd).train()                                        # forward, then backward through autograd
        out = m2(x)
        assert out.requires_grad and out.shape == (bs, 1)
        torch.nn.functional.mse_loss(out, y.reshape(-1, 1)).backward()
        auto = torch.cat([t.grad.reshape(-1) for t in m2._named()])
        assert float((auto - fused).abs().max()) < 1e-5 * float(fused.abs().max())     # (d pred comes from torch's MSE here: not the same bits)


# ---- 2. edge shapes against the fp64 oracle ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def seeded_case(cfg_items, bs, seed):
    cfg = {k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg_items}
    sd = seeded_weights(cfg, seed)
    x = O.seeded_input(cfg, bs, seed)
    y = np.random.default_rng(seed).uniform(0, 1, bs).astype(np.float32)
    return cfg, sd, x, y


def items(cfg):
    return tuple((k, tuple(v) if isinstance(v, list) else v) for k, v in cfg.items())


def oracle_step_check(what, cfg, sd, x, y):
    o = O.forward_backward(sd, x, y, cfg)
    g32 = O.torch_grads(sd, x, y, cfg, torch.float32)[2]
    m = build_model(cfg, sd).train()
    pred, loss = m.fused_mse_step(dev(x), dev(y))
    check_forward(what, m, x.shape[0], pred, loss, o, o["loss"])
    return check_grads(what, grads_of(m), o["grads"], g32), m, o


EDGES = {}
for _T in (1, 2, 3, 64, 65, 128):
    EDGES[f"T{_T}-P4"] = (make_cfg(_T, 4, [5, 4, 3]), 2)
for _P in (5, 63, 65, 2048):                                    # (P = 4 at T = 3 is T3-P4)
    EDGES[f"T3-P{_P}"] = (make_cfg(3, _P, [5, 4, 3]), 2)
for _C in (1, 63, 64, 65, 512):
    EDGES[f"width{_C}-one-layer"] = (make_cfg(3, 8, [_C]), 2)
EDGES["four-layers"] = (make_cfg(5, 8, [7, 6, 5, 4]), 2)
EDGES["lstm-hidden-1"] = (make_cfg(5, 8, [6, 4], lstm=[1]), 2)
EDGES["lstm-hidden-128"] = (make_cfg(5, 8, [6, 4], lstm=[128]), 2)
EDGES["three-lstm-layers"] = (make_cfg(5, 8, [6, 4], lstm=[4, 3, 2]), 2)
EDGES["bs1"] = (make_cfg(5, 8, [5, 4, 3]), 1)


@pytest.mark.parametrize("key", list(EDGES))
def test_edge_shapes_match_oracle(key):
    cfg, bs = EDGES[key]
    cfg, sd, x, y = seeded_case(items(cfg), bs, 7)
    oracle_step_check("edge-" + key, cfg, sd, x, y)


def test_more_graphs_than_the_attention_grid_has_workgroups():
    """1 400 samples = 1 400 graphs: the attention grid is capped at 1 024 workgroups, so some take a second graph and the partial rows
    hold sums."""
    cfg, sd, x, y = seeded_case(items(TINY), 1400, 9)
    oracle_step_check("tiny-bs1400", cfg, sd, x, y)


# ---- 3. dropout ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,p", [(SMALL[1], 0.2), (SMALL[1], 0.5), (FULL[1], 0.2), (FULL[1], 0.5)])
def test_training_with_dropout_matches_oracle(name, p):
    z, cfg, sd = load_case(name)
    bs = z["x"].shape[0]
    m = build_model(cfg, sd, dropout=p).train()
    x, y = dev(z["x"]), dev(z["y"])
    firsts = []
    for step in (1, 2):                                        # the step counter changes the mask
        keep = O.keep_masks(bs, cfg, m._seed, step, p)
        o = O.forward_backward(sd, z["x"], z["y"], cfg, keep=keep, dropout_p=p)
        g32 = O.torch_grads(sd, z["x"], z["y"], cfg, torch.float32, keep, p)[2]
        pred, loss = m.fused_mse_step(x, y)
        assert m._step == step
        assert rel(o["h0"], oracle_run(name)["h0"]) > 10 * TOL                   # the masks matter
        check_forward(f"{name}-dropout{p}-step{step}", m, bs, pred, loss, o, o["loss"])
        check_grads(f"{name}-dropout{p}-step{step}", grads_of(m), o["grads"], g32)
        firsts.append(m.bucket[:m.num_live + 1].clone())
    assert not torch.equal(firsts[0], firsts[1])
    m._step = 0
    m.fused_mse_step(x, y)
    assert torch.equal(m.bucket[:m.num_live + 1], firsts[0])                     # the same seed and step: the same bits
    m.eval()                                                                      # eval draws none
    with torch.no_grad():
        assert rel(m(x).cpu().numpy(), z["pred_eval"]) < TOL


# ---- 4. shards -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_two_shards_sum_to_the_full_batch(p):
    z, cfg, sd = load_case(SMALL[0])
    bs = z["x"].shape[0]
    x, y = dev(z["x"]), dev(z["y"])
    full = build_model(cfg, sd, dropout=p).train()
    keep = O.keep_masks(bs, cfg, full._seed, 1, p) if p else None
    o = O.forward_backward(sd, z["x"], z["y"], cfg, keep=keep, dropout_p=p)
    g32 = O.torch_grads(sd, z["x"], z["y"], cfg, torch.float32, keep, p)[2]
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
    check_grads(f"shards-p{p}", grads_of(full, total), o["grads"], g32)
    a, b = total[:full.num_live].cpu().numpy(), full.bucket[:full.num_live].cpu().numpy()
    assert np.abs(a - b).max() < 1e-5 * np.abs(b).max()


# ---- 5. fixed-order reductions ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["32x1024-bs2", "tiny-bs1400"])
def test_two_runs_give_the_same_bits(case):
    if case == "32x1024-bs2":
        z, cfg, sd = load_case(FULL[2])
        x, y = z["x"], z["y"]
    else:
        cfg, sd, x, y = seeded_case(items(TINY), 1400, 9)
    outs = []
    for _ in range(2):
        m = build_model(cfg, sd, dropout=0.2).train()
        m._seed = 99
        m.fused_mse_step(dev(x), dev(y))
        outs.append(m._grad_flat.clone())
    assert torch.isfinite(outs[0]).all() and outs[0].abs().max() > 0 and torch.equal(outs[0], outs[1])
    print("GATLSTM-GATE run-to-run: identical bits")


# ---- 6. the optimizer, the curve, the harness -------------------------------------------------------------------------------------------
def test_fused_step_applies_adam_to_every_element_once():
    """The twin-model procedure (family_kit.adam_twin_check), dropout and weight decay on: every element of the flat buffer within the
    bounds."""
    z, cfg, sd = load_case(SMALL[1])
    K.adam_twin_check(lambda: build_model(cfg, sd, dropout=0.2).train(), dev(z["x"]), dev(z["y"]), "GAT_LSTM")


def test_training_curve_matches_reference_algorithm():
    """Twenty update() steps against the reference's own.  Tolerances: GRU_CM's curve tolerances (tests/test_grucm_gpu.py: the first
    three losses 1e-4, every loss 2e-3, the eval prediction at the end 5e-3)."""
    z = np.load(os.path.join(GOLD, CURVE + ".npz"))
    cfg = json.loads(str(z["cfg_json"]))
    sd0 = {k[4:]: z[k] for k in z.files if k.startswith("sd0:")}
    _, sd = K.curve_check("GAT_LSTM", "GATLSTM", cfg, z, sd0, dict(steps=20, first3=1e-4, every=2e-3, params=2e-3, eval=5e-3), dropout_off=False)
    assert list(sd) == O.param_names(cfg)


def test_trainer_matches_reference_harness_run_on_phm2012(tmp_path, monkeypatch):
    """--GNN_method GAT_LSTM on PHM2012 Condition_1 as the reference wires it: the reference's own harness, run on the CPU by
    tests/golden/make_golden_gatlstm.py::case_trainer_phm2012 with the row's dropout set to 0, vs this package's harness on the GPU with
    the same switch.  Bars: those of tests/test_trainer_gpu.py's harness tests."""
    import pandas as pd
    z = np.load(os.path.join(GOLD, "gatlstm_trainer_phm2012_c1_reference_run.npz"))

    def row(tr):
        assert tr.train_configs["batch_size"] == int(z["batch_size"]) and tr.train_configs["learning_rate"] == float(z["lr"])
        assert tr.model_configs == dict(load_case(FULL[0])[1], dropout=0.2)
        tr.model_configs["dropout"] = 0.0
    tr, per_epoch = K.harness_run(tmp_path, monkeypatch, "GAT_LSTM", "PHM2012", "Condition_1", z, configure=row)
    K.assert_harness("GATLSTM", per_epoch, K.state_of(tr), z,     # RMSE, absolute (north star); MAE, RMSE relative
                     dict(rmse_abs=1e-3, rmse_scale=1.0, rel=1e-3, rel_from=2, final=2e-3, final_prefix="model."))
    csv = pd.read_csv(tmp_path / "logs" / "exp" / "r" / "GAT_LSTM_run_0" / "results.csv")
    ref_csv = pd.read_csv(io.StringIO(str(z["csv_text"])))
    assert list(csv.columns) == list(ref_csv.columns) and len(csv) == len(ref_csv)
    assert np.allclose(csv.iloc[1:].to_numpy()[:, 2:], ref_csv.iloc[1:].to_numpy()[:, 2:], rtol=2e-3)


# ---- 7. NaN ----------------------------------------------------------------------------------------------------------------------------
def test_nan_fixture_poisons_exactly_its_own_samples():
    z, cfg, sd = load_case(NAN)
    m = build_model(cfg, sd).eval()
    x = dev(z["x"])
    with torch.no_grad():
        pred = m(x).cpu().numpy()
    want = z["pred_eval"]
    assert np.isnan(want).reshape(-1).tolist() == [True, False, True]
    assert rel_finite(pred, want) < TOL                                              # NaN in exactly the fixture's samples
    feat = m.tap(3, "feat").cpu().numpy()
    assert np.isnan(feat).sum() == 8 and rel_finite(feat, z["tap:feat"]) < TOL
    for k in ("h0", "h1", "lstm"):
        assert rel_finite(m.tap(3, k).cpu().numpy(), z["tap:" + k]) < TOL, k


# ---- 8. coverage -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [make_cfg(129, 4, [2]), make_cfg(1, 3, [2]), make_cfg(1, 2049, [2]), make_cfg(1, 4, [513]), make_cfg(1, 4, [2] * 5),
                                 make_cfg(1, 4, [2], lstm=[129]), make_cfg(1, 4, [2], lstm=[2] * 4)],
                         ids=["num_patch129", "patch_size3", "patch_size2049", "width513", "five-layers", "lstm129", "four-lstm-layers"])
def test_just_outside_each_limit_is_not_covered_and_launches_nothing(cfg):
    from gnn_rul_benchmarking_amd.gatlstm import GAT_LSTM_model
    K.refused_outside_limits(GAT_LSTM_model(**cfg), torch.rand(2, cfg["num_patch"] * cfg["patch_size"], device=DEV))
