"""AGCN_TF HIP path vs the reference's golden outputs and vs the fp64 oracle (GPU).

Gates, relative to each tensor's largest entry: 1e-4 on features, taps, predictions and loss, 5e-4 on gradients -- against the fp32
reference fixtures and the fp64 oracle alike (the fp32 reference against its own fp64 run stays within 3.3e-6 / 4.7e-5 over shapes from
5 x 7 to 256 x 128, so the reference alone passes them with 10x room).  Each head's W_k.bias gradient is analytically zero (the rows of a
softmax gradient sum to zero): it is compared as max|g| <= 5e-4 max|grad W_q.bias| of the same head."""
import os

import numpy as np
import pytest
import torch

import agcntf_oracle as O
import family_kit as K
from family_kit import grads_of
from test_agcntf_oracle_golden import CASES, load_case
from test_sagcn_gpu import rank_margin, signal
from test_sagcn_oracle_golden import rel

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"
TOL, GTOL = 1e-4, 5e-4


def build_model(cfg, p):
    from gnn_rul_benchmarking_amd.agcntf import AGCN_TF_model
    m = AGCN_TF_model(**cfg)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in p.items()})
    return m.to(DEV)


def check_grads(got, want, heads):
    for k in O.param_names(heads):
        print(f"  grad {k}: rel {rel(got[k], want[k]):.3e}  max|want| {np.abs(want[k]).max():.3e}")
    for k in O.param_names(heads):
        if k.endswith("W_k.bias"):
            assert np.abs(got[k]).max() <= GTOL * np.abs(want[k.replace("W_k", "W_q")]).max(), k
            continue
        assert got[k].shape == want[k].shape and rel(got[k], want[k]) < GTOL, k


def draw_input(bs, P, n, seed):
    for attempt in range(50):
        x = signal(bs, P * n, seed + 1000 * attempt)
        if rank_margin(x, n) > 1e-5:
            return x
    pytest.fail("no input away from the rank edges")


# ---- 1. the reference's fixtures ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_forward_taps_and_fused_step_match_reference_golden(name):
    z, cfg, p = load_case(name)
    heads = cfg.get("num_heads", 1)
    m = build_model(cfg, p)
    x, y = torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(z["y"]).to(DEV)
    bs = x.size(0)
    m.eval()
    with torch.no_grad():
        pred = m(x)
    print(name, "pred", rel(pred.cpu().numpy(), z["pred"]), "feat", rel(m.tap(bs, "features").cpu().numpy(), z["feat"]),
          "H", rel(m.tap(bs, "H").cpu().numpy(), z["H"]), "O", rel(m.tap(bs, "attention_out").cpu().numpy(), z["attn_out"]))
    assert pred.shape == (bs, 1) and rel(pred.cpu().numpy(), z["pred"]) < TOL
    assert rel(m.tap(bs, "features").cpu().numpy(), z["feat"]) < TOL
    assert rel(m.tap(bs, "H").cpu().numpy(), z["H"]) < TOL
    assert rel(m.tap(bs, "attention_out").cpu().numpy(), z["attn_out"]) < TOL
    m.train()
    pred2, loss = m.fused_mse_step(x, y)
    assert rel(pred2.cpu().numpy().reshape(-1, 1), z["pred"]) < TOL
    assert abs(float(loss) - float(z["loss"])) < TOL * abs(float(z["loss"]))
    check_grads(grads_of(m), {k: z["grad:" + k] for k in O.param_names(heads)}, heads)


# ---- 2. the oracle ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,n,Ha,Hg,heads,bs", [(40, 64, 100, 100, 1, 12), (128, 256, 100, 100, 1, 3), (256, 128, 100, 100, 1, 2), (1, 16, 8, 8, 1, 4),
                                                (5, 7, 6, 7, 2, 9), (70, 20, 33, 50, 3, 3), (24, 16, 128, 128, 4, 2), (17, 3, 1, 1, 1, 5)])
def test_training_step_matches_oracle(P, n, Ha, Hg, heads, bs):
    cfg = dict(num_patch=P, patch_size=n, hidden_adj_dim=Ha, hidden_gnn_dim=Hg, num_heads=heads)
    p = O.random_params(P, Ha, Hg, heads, seed=bs)
    y = np.random.default_rng(bs).uniform(0, 1, bs)
    x = draw_input(bs, P, n, P * 10 + bs)
    loss, grads, fw = O.loss_and_grads(p, x, y, P, n)
    m = build_model(cfg, p).train()
    xt, yt = torch.from_numpy(x.astype(np.float32)).to(DEV), torch.from_numpy(y.astype(np.float32)).to(DEV)
    pred, l = m.fused_mse_step(xt, yt)
    print((P, n, Ha, Hg, heads, bs), "feat", rel(m.tap(bs, "features").cpu().numpy(), fw.feat), "H", rel(m.tap(bs, "H").cpu().numpy(), fw.H),
          "O", rel(m.tap(bs, "attention_out").cpu().numpy(), fw.O), "pred", rel(pred.cpu().numpy().reshape(-1, 1), fw.pred),
          "loss", abs(float(l) - loss) / abs(loss))
    assert rel(m.tap(bs, "features").cpu().numpy(), fw.feat) < TOL
    assert rel(m.tap(bs, "H").cpu().numpy(), fw.H) < TOL
    assert rel(m.tap(bs, "attention_out").cpu().numpy(), fw.O) < TOL
    assert rel(pred.cpu().numpy().reshape(-1, 1), fw.pred) < TOL
    assert abs(float(l) - loss) < TOL * abs(loss)
    check_grads(grads_of(m), grads, heads)


# ---- 3. ragged batches -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ragged_reference():
    P, n, Ha, Hg = 40, 64, 100, 100
    p = O.random_params(P, Ha, Hg, 1, seed=77)
    x = draw_input(257, P, n, 4242)
    return p, x, O.forward(p, x, P, n).pred


@pytest.mark.parametrize("bs", [1, 3, 100, 257])
def test_eval_forward_at_ragged_batches(ragged_reference, bs):
    p, x, want = ragged_reference
    m = build_model(dict(num_patch=40, patch_size=64, hidden_adj_dim=100, hidden_gnn_dim=100), p).eval()
    with torch.no_grad():
        pred = m(torch.from_numpy(x[:bs].astype(np.float32)).to(DEV))
    assert pred.shape == (bs, 1) and rel(pred.cpu().numpy(), want[:bs]) < TOL


# ---- 4. split equals fused -------------------------------------------------------------------------------------------------------------
def _case(name="agcntf_small_5x7_bs6"):
    z, cfg, p = load_case(name)
    return cfg, p, torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(z["y"]).to(DEV)


@pytest.mark.parametrize("name", ["agcntf_small_5x7_bs6", "agcntf_phm_40x64_bs4"])
def test_forward_then_backward_equals_fwdbwd_bit_for_bit(name):
    cfg, p, x, y = _case(name)
    m = build_model(cfg, p).train()
    m.fused_mse_step(x, y)
    fused = m.bucket[:m.num_live + 1].clone()
    m.fused_mse_step(x, y)
    assert torch.equal(m.bucket[:m.num_live + 1], fused)                      # twice the same step: the same bits
    m2 = build_model(cfg, p).train()
    x2, yv = m2._step_inputs(x, y)
    shp = m2._shape(x2.size(0))
    a = m2._args(shp, x2, y=yv)
    m2._call("forward", shp, a)
    m2._call("backward", shp, a)
    assert torch.equal(m2.bucket[:m2.num_live + 1], fused)


def test_autograd_path_equals_fused_path_and_both_updates_move_the_weights():
    from gnn_rul_benchmarking_amd.algorithms import get_algorithm_class
    cfg, p, x, y = _case()
    m = build_model(cfg, p).train()
    m.fused_mse_step(x, y)
    fused = m._grad_flat[:m.num_live].clone()
    m2 = build_model(cfg, p).train()
    torch.nn.functional.mse_loss(m2(x), y).backward()
    auto = torch.cat([t.grad.reshape(-1) for t in m2._named()])
    assert torch.equal(auto, fused)
    algo = get_algorithm_class("AGCN_TF")(cfg, {"learning_rate": 1e-3, "weight_decay": 1e-4}, DEV)
    algo.to(DEV).train()
    before = algo.model.fc.weight.clone()
    a = algo.update(x, y, 1)["loss"]
    mid = algo.model.fc.weight.clone()
    b = algo.update_reference_style(x, y, 1)["loss"]
    assert np.isfinite(a) and np.isfinite(b) and not torch.equal(mid, before) and not torch.equal(algo.model.fc.weight, mid)


# ---- 5. shards -------------------------------------------------------------------------------------------------------------------------
def test_two_shards_sum_to_the_one_piece_step():
    cfg, p, x, y = _case()
    B = x.size(0)
    m = build_model(cfg, p).train()
    m.fused_mse_step(x, y)
    whole = m.bucket[:m.num_live + 1].cpu().numpy().astype(np.float64)
    acc = np.zeros_like(whole)
    for sl in (slice(0, B // 2), slice(B // 2, B)):
        m.fused_mse_step(x[sl], y[sl], global_batch=B)
        acc += m.bucket[:m.num_live + 1].cpu().numpy().astype(np.float64)
    n = m.num_live
    assert abs(acc[n] - whole[n]) < GTOL * abs(whole[n])
    for name, (off, shape) in m._layout.items():
        k = int(np.prod(shape))
        if name.endswith("W_k.bias"):                 # analytically zero: measured against the same head's W_q.bias gradient
            qoff = m._layout[name.replace("W_k", "W_q")][0]
            assert np.abs(acc[off:off + k] - whole[off:off + k]).max() <= GTOL * np.abs(whole[qoff:qoff + k]).max(), name
            continue
        assert rel(acc[off:off + k], whole[off:off + k]) < GTOL, name


# ---- 6. training curve -----------------------------------------------------------------------------------------------------------------
def test_training_curve_matches_reference_algorithm():
    from gnn_rul_benchmarking_amd.algorithms import get_algorithm_class
    z = np.load(os.path.join(GOLD, "agcntf_train_curve_12x16_bs8.npz"))
    cfg = {k[4:]: int(z[k]) for k in z.files if k.startswith("cfg:")}
    algo = get_algorithm_class("AGCN_TF")(cfg, {"learning_rate": float(z["lr"]), "weight_decay": float(z["wd"])}, DEV)
    algo.load_state_dict({k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd0:")})
    algo.to(DEV).train()
    xs, ys = torch.from_numpy(z["xs"]).to(DEV), torch.from_numpy(z["ys"]).to(DEV)
    assert xs.size(0) == 12
    losses = [algo.update(xs[s], ys[s], 1)["loss"] for s in range(xs.size(0))]
    assert np.allclose(losses, z["losses"], rtol=1e-3), (losses, z["losses"].tolist())
    algo.eval()
    with torch.no_grad():
        assert rel(algo.model(xs[0]).cpu().numpy(), z["eval_pred_end"]) < 1e-3
    sd = algo.state_dict()
    for k in sd:
        assert rel(sd[k].cpu().numpy(), z["sd_end:" + k]) < 1e-3, k


# ---- 7. module round trip and guards ---------------------------------------------------------------------------------------------------
def test_state_dict_round_trip():
    from gnn_rul_benchmarking_amd.agcntf import AGCN_TF_model
    cfg, p, x, y = _case()
    m = build_model(cfg, p).eval()
    m2 = AGCN_TF_model(**cfg).to(DEV).eval()
    m2.load_state_dict(m.state_dict())
    assert list(m2.state_dict()) == O.param_names(cfg["num_heads"])
    with torch.no_grad():
        assert torch.equal(m(x), m2(x))
    assert torch.equal(m.flat_params, m2.flat_params)


def test_unsupported_configuration_raises_at_the_first_call():
    from gnn_rul_benchmarking_amd.agcntf import AGCN_TF_model
    m = AGCN_TF_model(5, 7, 6, 129).to(DEV)
    with pytest.raises(RuntimeError, match="do not cover this configuration"):
        m(torch.zeros(2, 35, device=DEV))
    with pytest.raises(RuntimeError, match="do not cover this configuration"):
        m.fused_mse_step(torch.zeros(2, 35, device=DEV), torch.zeros(2, device=DEV))


def test_autograd_backward_after_a_second_forward_raises():
    cfg, p, x, y = _case()
    m = build_model(cfg, p).train()
    p1 = m(x)
    with torch.no_grad():
        m(x * 0.5)
    with pytest.raises(RuntimeError, match="overwritten"):
        p1.sum().backward()
    p2 = m(x)
    torch.nn.functional.mse_loss(p2, y).backward()
    m2 = build_model(cfg, p).train()
    m2.fused_mse_step(x, y)
    assert torch.equal(torch.cat([t.grad.reshape(-1) for t in m._named()]), m2._grad_flat[:m2.num_live])


# ---- 8. trainer ------------------------------------------------------------------------------------------------------------------------
def test_trainer_matches_reference_harness_run_on_phm2012(tmp_path, monkeypatch):
    """--GNN_method AGCN_TF on PHM2012 Condition_1 as the reference wires it (configs/hparams.py:227,243: 40 patches of 64 points, hidden
    100 / 100, batch 100, lr 1e-4, wd 1e-4): the reference's own harness, run on the CPU with the argsort pinned to the stable order by
    tests/golden/make_golden_agcntf.py::case_trainer_phm2012, vs this package's harness on the GPU."""
    import io
    import pandas as pd
    z = np.load(os.path.join(GOLD, "agcntf_trainer_phm2012_c1_reference_run.npz"))
    assert bool(z["argsort_pinned_stable"])

    def row(tr):
        assert tr.model_configs == dict(num_patch=40, patch_size=64, hidden_adj_dim=100, hidden_gnn_dim=100)
        assert tr.train_configs == {'num_epochs': 3, 'batch_size': 100, 'weight_decay': 1e-4, 'learning_rate': 1e-4}
    _, per_epoch = K.harness_run(tmp_path, monkeypatch, "AGCN_TF", "PHM2012", "Condition_1", z, configure=row)
    K.assert_harness("AGCN_TF", per_epoch, None, z, dict(rmse_abs=1e-4, rmse_scale=1.0, rel=1e-4, rel_from=2))
    csv = pd.read_csv(tmp_path / "logs" / "exp" / "r" / "AGCN_TF_run_0" / "results.csv")
    ref_csv = pd.read_csv(io.StringIO(str(z["csv_text"])))
    assert list(csv.columns) == list(ref_csv.columns) and len(csv) == len(ref_csv)
