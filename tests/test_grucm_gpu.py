"""GRU_CM on the GPU (csrc/grucm.hip, csrc/gru_seq.hip): the C entries against the reference's fixtures (tests/golden/make_golden_grucm.py)
and against the fp64 oracle (tests/grucm_oracle.py), the persistent GRU against the oracle's GRU and the step-loop entries, shard
semantics, and the module / algorithm / trainer surface.

Tolerances (each relative to the largest entry of the tensor, gpu_util.rel_err): 1e-4 on predictions and loss, 5e-4 on gradients against
the fp32 reference, 2e-4 against the fp64 oracle."""
import ctypes as C
import glob
import os

import numpy as np
import pytest
import torch

from gnn_rul_benchmarking_amd import _lib

import family_kit
import gpu_util as G
import grucm_oracle as O
from conftest import GOLDEN
from golden_io import load_npz

pytestmark = pytest.mark.gpu

TOL, GTOL_REF, GTOL_ORACLE = 1e-4, 5e-4, 2e-4
CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "grucm_*x*_bs*.npz")) if "curve" not in p)


def load(name):
    z = load_npz(os.path.join(GOLDEN, name + ".npz"))
    cfg = {k[4:]: int(z[k]) for k in z.files if k.startswith("cfg:")}
    p = {k[3:]: z[k] for k in z.files if k.startswith("sd:")}
    return z, cfg, p


def abi(x_np, p, cfg, mode="forward", y_np=None, training=False, dropout=(0.0, 0.0, 0.0), seed=0, step=1, global_batch=None,
        sample_offset=0, gru_path=_lib.GRUCM_GRU_AUTO, dpred_np=None):
    """The rulgnn_grucm_* entries on cuda:0.  mode: forward | split (forward then backward) | fwdbwd.  Returns dict(pred, loss, grads)."""
    lib = _lib.load()
    dev = torch.device("cuda:0")
    B = x_np.shape[0]
    x = torch.from_numpy(np.ascontiguousarray(x_np, np.float32)).to(dev)
    y = torch.from_numpy(np.ascontiguousarray(y_np, np.float32).reshape(B)).to(dev) if y_np is not None else None
    dp = torch.from_numpy(np.ascontiguousarray(dpred_np, np.float32).reshape(B)).to(dev) if dpred_np is not None else None
    prm = torch.from_numpy(O.flatten(p)).to(dev)
    grads = torch.full_like(prm, float("nan"))
    pred = torch.full((B,), float("nan"), device=dev)
    loss = torch.full((1,), float("nan"), device=dev)
    shp = _lib.GrucmShape(B, cfg["num_nodes"], cfg["time_length"], cfg["gru_hidden_dim"])
    nbytes = lib.rulgnn_grucm_workspace_bytes(C.byref(shp))
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    a = _lib.GrucmArgs()
    a.x = x.data_ptr(); a.y = y.data_ptr() if y is not None else None
    a.dpred = dp.data_ptr() if dp is not None else None
    a.params = prm.data_ptr(); a.grads = grads.data_ptr(); a.pred = pred.data_ptr(); a.loss = loss.data_ptr()
    a.workspace = ws.data_ptr(); a.workspace_bytes = nbytes
    a.global_batch = B if global_batch is None else global_batch
    a.sample_offset = sample_offset
    for i in range(3):
        a.dropout_p[i] = dropout[i]
    a.seed, a.step, a.training, a.gru_path = seed, step, 1 if training else 0, gru_path
    st = G.stream_ptr()
    if mode in ("forward", "split"):
        _lib.check(lib.rulgnn_grucm_forward_f32(C.byref(shp), C.byref(a), st), "grucm_forward")
    if mode == "split":
        _lib.check(lib.rulgnn_grucm_backward_f32(C.byref(shp), C.byref(a), st), "grucm_backward")
    if mode == "fwdbwd":
        _lib.check(lib.rulgnn_grucm_fwdbwd_f32(C.byref(shp), C.byref(a), None, st), "grucm_fwdbwd")
    torch.cuda.synchronize()
    return {"pred": pred.cpu().numpy(), "loss": float(loss.item()), "grads": grads.cpu().numpy()}


def check_grads(flat, ref, p, tol, what=""):
    got = O.unflatten(flat, p)
    for k in O.param_names():
        e = G.rel_err(got[k], np.asarray(ref[k]).reshape(got[k].shape))
        print(f"  {what} grad {k}: rel err {e:.3e}")
        assert e < tol, (what, k, e)


# ---- 1. eval forward ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_eval_forward_matches_reference_and_oracle(name):
    z, cfg, p = load(name)
    r = abi(z["x"], p, cfg)
    e_ref, e_or = G.rel_err(r["pred"], z["eval_pred"][:, 0]), G.rel_err(r["pred"], O.forward(z["x"], p)[:, 0])
    print(name, "eval pred rel err vs reference", e_ref, "vs oracle", e_or)
    assert e_ref < TOL and e_or < TOL


@pytest.mark.parametrize("B", [1, 3, 100, 257, 4100])
def test_eval_forward_ragged_batches(B):
    """Batches that do not fill the last wavefront / workgroup / sequence tile, against the oracle."""
    z, cfg, p = load("grucm_cmapss_14x50_bs8")
    rng = np.random.default_rng(100 + B)
    x = rng.uniform(0.0, 1.0, size=(B, 14, 50)).astype(np.float32)
    r = abi(x, p, cfg)
    ref = np.concatenate([O.forward(x[i:i + 256], p)[:, 0] for i in range(0, B, 256)])
    e = G.rel_err(r["pred"], ref)
    print("ragged batch", B, "rel err", e)
    assert e < TOL


# ---- 2. training, p = 0, against the reference's autograd -------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["split", "fwdbwd"])
@pytest.mark.parametrize("name", CASES)
def test_training_step_matches_reference_gradients(name, mode):
    z, cfg, p = load(name)
    r = abi(z["x"], p, cfg, mode=mode, y_np=z["y"], training=True)
    print(name, mode, "pred", G.rel_err(r["pred"], z["pred"][:, 0]), "loss", abs(r["loss"] - float(z["loss"])) / float(z["loss"]))
    assert G.rel_err(r["pred"], z["pred"][:, 0]) < TOL
    assert abs(r["loss"] - float(z["loss"])) < TOL * float(z["loss"])
    check_grads(r["grads"], {k: z["grad:" + k] for k in O.param_names()}, p, GTOL_REF, name)


# ---- 3. dropout on, against the oracle with the hash masks ---------------------------------------------------------------------------
# (not on the wrap fixture: four fp64 oracle steps over thousands of samples; tests/test_grad_elementwise_gpu.py holds that batch element-wise)
@pytest.mark.parametrize("rates", [(0.2, 0.2, 0.2), (0.1, 0.3, 0.5)])
@pytest.mark.parametrize("name", [n for n in CASES if "_wrap_" not in n])
def test_dropout_step_matches_oracle(name, rates):
    z, cfg, p = load(name)
    x, y = z["x"], z["y"]
    B, N, L, H = x.shape[0], cfg["num_nodes"], cfg["time_length"], cfg["gru_hidden_dim"]
    preds = []
    for step in (3, 4):
        r = abi(x, p, cfg, mode="fwdbwd", y_np=y, training=True, dropout=rates, seed=77, step=step)
        loss, g, pred, _ = O.forward_backward(x, y, p, O.masks(B, N, L, H, 77, step, rates))
        print(name, rates, "step", step, "pred", G.rel_err(r["pred"], pred[:, 0]), "loss", abs(r["loss"] - loss) / loss)
        assert G.rel_err(r["pred"], pred[:, 0]) < TOL
        assert abs(r["loss"] - loss) < TOL * loss
        check_grads(r["grads"], g, p, GTOL_ORACLE, f"{name} step {step}")
        preds.append(r["pred"])
    assert G.rel_err(preds[0], preds[1]) > 1e-3          # the next step draws other masks


# ---- 4. the persistent GRU alone ------------------------------------------------------------------------------------------------------
def gru_abi(persistent, x, w, dout):
    lib = _lib.load()
    dev = torch.device("cuda:0")
    S, L, I = x.shape
    H = w["w_hh"].shape[1]
    t = {k: torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(dev) for k, v in dict(w, x=x, dout=dout).items()}
    out = torch.full((S, L, H), float("nan"), device=dev)
    dx = torch.full((S, L, I), float("nan"), device=dev)
    g = {k: torch.full_like(t[k], float("nan")) for k in ("w_ih", "w_hh", "b_ih", "b_hh")}
    shp = _lib.GruShape(S, L, I, H)
    pre = "rulgnn_gru_persistent_" if persistent else "rulgnn_gru_"
    nbytes = getattr(lib, pre + "workspace_bytes")(C.byref(shp))
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    a = _lib.GruArgs(t["x"].data_ptr(), t["w_ih"].data_ptr(), t["w_hh"].data_ptr(), t["b_ih"].data_ptr(), t["b_hh"].data_ptr(), out.data_ptr(),
                     t["dout"].data_ptr(), dx.data_ptr(), g["w_ih"].data_ptr(), g["w_hh"].data_ptr(), g["b_ih"].data_ptr(), g["b_hh"].data_ptr(),
                     ws.data_ptr(), nbytes)
    _lib.check(getattr(lib, pre + "forward_f32")(C.byref(shp), C.byref(a), G.stream_ptr()), pre + "forward_f32")
    _lib.check(getattr(lib, pre + "backward_f32")(C.byref(shp), C.byref(a), G.stream_ptr()), pre + "backward_f32")
    torch.cuda.synchronize()
    res = {"out": out.cpu().numpy(), "dx": dx.cpu().numpy()}
    res.update({"d" + k: v.cpu().numpy() for k, v in g.items()})
    return res


def gru_inputs(S, L, I, H, seed):
    rng = np.random.default_rng(seed)
    k = 1.0 / np.sqrt(H)
    w = {"w_ih": rng.uniform(-k, k, (3 * H, I)), "w_hh": rng.uniform(-k, k, (3 * H, H)), "b_ih": rng.uniform(-k, k, 3 * H),
         "b_hh": rng.uniform(-k, k, 3 * H)}
    return rng.uniform(-1.0, 1.0, (S, L, I)), w, rng.uniform(-1.0, 1.0, (S, L, H))


@pytest.mark.parametrize("S,L,I,H", [(100, 50, 7, 64), (256, 50, 10, 64), (37, 21, 5, 64), (1, 1, 7, 64)])
def test_persistent_gru_matches_oracle_and_step_loop(S, L, I, H):
    x, w, dout = gru_inputs(S, L, I, H, 1000 + S)
    w32 = {k: v.astype(np.float32).astype(np.float64) for k, v in w.items()}
    x32, d32 = x.astype(np.float32).astype(np.float64), dout.astype(np.float32).astype(np.float64)
    out, tape = O.gru_forward(x32, w32["w_ih"], w32["w_hh"], w32["b_ih"], w32["b_hh"])
    dx, dw_ih, dw_hh, db_ih, db_hh = O.gru_backward(x32, w32["w_ih"], w32["w_hh"], tape, d32)
    ref = {"out": out, "dx": dx, "dw_ih": dw_ih, "dw_hh": dw_hh, "db_ih": db_ih, "db_hh": db_hh}
    pers, loop = gru_abi(True, x, w, dout), gru_abi(False, x, w, dout)
    for k in ref:
        tol = TOL if k == "out" else GTOL_ORACLE
        e_or, e_loop = G.rel_err(pers[k], ref[k]), G.rel_err(pers[k], loop[k])
        print(f"  persistent GRU {(S, L, I, H)} {k}: vs oracle {e_or:.3e}, vs step loop {e_loop:.3e}")
        assert e_or < tol and e_loop < tol, (k, e_or, e_loop)


def test_step_loop_gru_is_untouched_by_the_persistent_path():
    """rulgnn_gru_* on STGNN's shapes (C-MAPSS: 100 x 14 sequences of one step; N-CMAPSS: 100 x 20 sequences of five steps, width 64):
    bit-identical results before and after the persistent kernels ran on the device."""
    for S, L, I, H in [(1400, 1, 64, 64), (2000, 5, 64, 64)]:
        x, w, dout = gru_inputs(S, L, I, H, 5)
        first = gru_abi(False, x, w, dout)
        xp, wp, dp = gru_inputs(64, 50, 7, 64, 6)
        gru_abi(True, xp, wp, dp)
        again = gru_abi(False, x, w, dout)
        for k in first:
            assert np.array_equal(first[k], again[k]), k


# ---- 5. the two recurrences inside GRU_CM ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_step_loop_switch_gives_the_same_step(name):
    z, cfg, p = load(name)
    kw = dict(mode="fwdbwd", y_np=z["y"], training=True, dropout=(0.2, 0.2, 0.2), seed=5, step=2)
    a = abi(z["x"], p, cfg, gru_path=_lib.GRUCM_GRU_PERSISTENT, **kw)
    b = abi(z["x"], p, cfg, gru_path=_lib.GRUCM_GRU_STEP_LOOP, **kw)
    d = abi(z["x"], p, cfg, gru_path=_lib.GRUCM_GRU_AUTO, **kw)
    assert np.array_equal(a["pred"], d["pred"]) and np.array_equal(a["grads"], d["grads"])      # the default IS the persistent path here
    assert G.rel_err(a["pred"], b["pred"]) < TOL and abs(a["loss"] - b["loss"]) < TOL * b["loss"]
    check_grads(a["grads"], O.unflatten(b["grads"], p), p, GTOL_REF, name + " persistent vs step loop")


# ---- 6. shard semantics -----------------------------------------------------------------------------------------------------------------
def test_shards_sum_to_the_one_piece_step():
    z, cfg, p = load("grucm_cmapss_14x50_bs8")
    rng = np.random.default_rng(42)
    B = 96
    x = rng.uniform(0.0, 1.0, (B, 14, 50)).astype(np.float32)
    y = rng.uniform(0.0, 1.0, (B, 1)).astype(np.float32)
    kw = dict(mode="fwdbwd", training=True, dropout=(0.2, 0.2, 0.2), seed=11, step=7)
    whole = abi(x, p, cfg, y_np=y, **kw)
    parts = [abi(x[lo:hi], p, cfg, y_np=y[lo:hi], global_batch=B, sample_offset=lo, **kw) for lo, hi in ((0, 40), (40, 96))]
    assert G.rel_err(np.concatenate([q["pred"] for q in parts]), whole["pred"]) < TOL
    assert abs(sum(q["loss"] for q in parts) - whole["loss"]) < TOL * whole["loss"]
    check_grads(parts[0]["grads"] + parts[1]["grads"], O.unflatten(whole["grads"], p), p, GTOL_REF, "shards")


# ---- 7. module surface ------------------------------------------------------------------------------------------------------------------
def _algo(cfg, lr, wd, dev):
    from gnn_rul_benchmarking_amd.algorithms import GRU_CM
    algo = GRU_CM(cfg, {"learning_rate": lr, "weight_decay": wd}, dev)
    algo.to(dev)
    for d in (algo.model.dropout1, algo.model.dropout2, algo.model.dropout3):
        d.p = 0.0
    return algo


def _curve():
    z = np.load(os.path.join(GOLDEN, "grucm_train_curve_14x50_bs16.npz"))
    cfg = {k[4:]: int(z[k]) for k in z.files if k.startswith("cfg:")}
    sd0 = {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd0:")}
    return z, cfg, sd0


def test_update_follows_the_reference_update_curve():
    z, cfg, sd0 = _curve()
    dev = torch.device("cuda:0")
    algo = _algo(cfg, float(z["lr"]), float(z["wd"]), dev)
    missing = algo.load_state_dict(sd0, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    algo.train()
    losses = [algo.update(torch.from_numpy(z["xs"][s]).to(dev), torch.from_numpy(z["ys"][s]).to(dev), 1)["loss"] for s in range(z["xs"].shape[0])]
    ref = z["losses"]
    print("curve losses got/ref", losses, ref)
    assert np.max(np.abs(np.array(losses[:3]) - ref[:3]) / ref[:3]) < 1e-4
    assert np.max(np.abs(np.array(losses) - ref) / ref) < 2e-3
    sd = algo.state_dict()
    for name in O.param_names():
        assert G.rel_err(sd["model." + name].cpu().numpy(), z["sd_end:model." + name]) < 5e-3, name
    algo.eval()
    with torch.no_grad():
        pred = algo.model(torch.from_numpy(z["xs"][0]).to(dev)).cpu().numpy()
    assert G.rel_err(pred, z["eval_pred_end"]) < 5e-3


def test_update_reference_style_and_autograd_equal_the_fused_step():
    z, cfg, sd0 = _curve()
    dev = torch.device("cuda:0")
    x, y = torch.from_numpy(z["xs"][0]).to(dev), torch.from_numpy(z["ys"][0]).to(dev)
    a, b = _algo(cfg, 1e-3, 1e-4, dev), _algo(cfg, 1e-3, 1e-4, dev)
    a.load_state_dict(sd0); b.load_state_dict(sd0)
    a.train(); b.train()
    # model(x) under autograd gives the fused step's gradients
    loss = torch.nn.functional.mse_loss(a.model(x), y)
    loss.backward()
    _, floss = b.model.fused_mse_step(x, y)
    assert abs(loss.item() - floss.item()) < TOL * floss.item()
    fg = b.model.bucket[:b.model.num_live].cpu().numpy()
    ag = np.concatenate([dict(a.model.named_parameters())[k].grad.reshape(-1).cpu().numpy() for k in O.param_names()])
    assert G.rel_err(ag, fg) < GTOL_REF
    a.optimizer.zero_grad()
    la = [a.update_reference_style(x, y, 1)["loss"] for _ in range(3)]
    lb = [b.update(x, y, 1)["loss"] for _ in range(3)]
    assert np.max(np.abs(np.array(la) - np.array(lb)) / np.array(lb)) < TOL
    assert G.rel_err(a.model.flat_params.cpu().numpy(), b.model.flat_params.cpu().numpy()) < GTOL_REF
    b.eval()
    with pytest.raises(RuntimeError, match="needs algorithm.train"):
        b.update(x, y, 1)


def test_state_dict_round_trip_and_guards():
    from gnn_rul_benchmarking_amd.algorithms import GRU_CM
    z, cfg, sd0 = _curve()
    dev = torch.device("cuda:0")
    x = torch.from_numpy(z["xs"][0]).to(dev)
    a = _algo(cfg, 1e-3, 1e-4, dev)
    a.train()
    a.update(x, torch.from_numpy(z["ys"][0]).to(dev), 1)
    a.eval()
    with torch.no_grad():
        pa = a.model(x)
    b = GRU_CM(cfg, {"learning_rate": 1e-3, "weight_decay": 1e-4}, dev)
    b.to(dev)
    b.load_state_dict(a.state_dict())
    b.eval()
    with torch.no_grad():
        pb = b.model(x)
    assert pa.shape == (x.size(0), 1) and torch.equal(pa, pb)
    with pytest.raises(RuntimeError, match="HIP path only"):
        a.model(x.cpu())
    with pytest.raises(RuntimeError, match="cannot reshape tensor of 0 elements"):
        a.model(x[:0])


# ---- 8. the trainer ---------------------------------------------------------------------------------------------------------------------
def test_trainer_drives_grucm_on_cmapss(tmp_path, monkeypatch):
    """--GNN_method GRU_CM on a synthetic C-MAPSS-format file for one epoch (batch 100, ragged last batch), dropout on: finite metrics."""
    import sys
    sys.path.insert(0, GOLDEN)
    from synth import synthetic_cmapss
    (xtr, ytr), (xte, yte) = synthetic_cmapss(4, 250, 80)
    data = ({"samples": xtr, "labels": ytr, "max_ruls": 125}, {"samples": xte, "labels": yte, "max_ruls": 125})

    def row(tr):
        assert tr.model_configs == dict(num_nodes=14, time_length=50, gru_hidden_dim=64)
    _, per_epoch = family_kit.harness_run(tmp_path, monkeypatch, "GRU_CM", "CMAPSS", "FD004", {"epochs": 1}, data=data, configure=row)
    got = np.asarray(per_epoch, np.float64)
    print("GRU_CM harness metrics:", got)
    assert got.shape == (1, 4) and np.isfinite(got).all()
