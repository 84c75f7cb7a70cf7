"""-m gpu: the grouped fused steps of DVGTformer and LOGO (rulgnn_<family>_fwdbwd_group_f32: the dominant kernels launched once for all
runs, grid y = the run) against each run's single call, bit for bit; run 0 against the fp64 oracles at the families' own bars;
``runs.DVGTformer_runs`` / ``runs.LOGO_runs`` against plain algorithms stepped alone; ``--concurrent_runs`` against the sequential loop.

Equality is the bar of the first group of tests because it is derivable: a run's per-sample arithmetic, its partial-row count and every
reduction order are the single call's (tests/test_dvgtformer_gpu.py::test_two_runs_give_the_same_bits and
tests/test_logo_gpu.py::test_same_step_twice_... hold the single call to determinism)."""
import argparse
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch

import dvgtformer_oracle as DO
import logo_oracle as LO
import test_dvgtformer_gpu as DV
import test_logo_gpu as LG
from family_kit import DEV, dev, grads_of

pytestmark = pytest.mark.gpu
STEPS = 3
SMALL_DV = DV.make_cfg(3, 4, H=1, d=(3, 5), ff=(2, 3))


def _optimizer(m):
    from gnn_rul_benchmarking_amd.optim import FusedAdam
    return FusedAdam(m, lr=1e-3, weight_decay=1e-4)


def _snapshot(m, opt, pred):
    mom = opt._state_buffers()
    return dict(pred=pred.clone(), bucket=m.bucket[:m.num_live + 1].clone(), params=m.flat_params.clone(), exp_avg=mom[0].clone(),
                exp_avg_sq=mom[1].clone())


def _same_bits(a, b):
    """torch.equal on the bit patterns: what torch.equal asks of finite values, and a NaN has to be the same NaN."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _stepped_together_equal_stepped_alone(build, cases, fields, finite=True):
    """``cases[r]`` = (state dict, x, y) of run r.  Twin models per run, dropout on, their own dropout seeds: three fused steps with Adam
    alone, three as one grouped call each; the prediction, the loss, the whole [gradient | loss] bucket, the parameters and both moments
    are compared bit for bit after every step (and with torch.equal where the values are finite)."""
    from gnn_rul_benchmarking_amd.runs import fused_group_step
    R = len(cases)
    xs, ys = [dev(c[1]) for c in cases], [dev(c[2]) for c in cases]

    def twins():
        models = [build(c[0]).train() for c in cases]
        for r, m in enumerate(models):
            m._seed = 1000 + 37 * r                                     # a run's own dropout stream
        return models, [_optimizer(m) for m in models]

    alone, alone_opt = twins()
    want = [[] for _ in range(R)]
    for r in range(R):
        for _ in range(STEPS):
            pred, _ = alone[r].fused_mse_step(xs[r], ys[r], alone_opt[r], **fields[r])
            want[r].append(_snapshot(alone[r], alone_opt[r], pred))
    together, together_opt = twins()
    for s in range(STEPS):
        outs = fused_group_step(together, together_opt, xs, ys, fields)
        for r in range(R):
            got = _snapshot(together[r], together_opt[r], outs[r][0])
            assert _same_bits(outs[r][1], got["bucket"][-1])
            for k, v in want[r][s].items():
                assert _same_bits(got[k], v), f"run {r} step {s}: {k}"
                if finite:
                    assert torch.isfinite(v).all() and torch.equal(got[k], v), f"run {r} step {s}: {k}"
    if finite:
        first = [float(want[r][0]["bucket"][-1]) for r in range(R)]
        assert len(set(first)) == R                                     # other weights, other batches: a crossed pointer shows
        assert all(w[0]["exp_avg"].abs().max() > 0 and not torch.equal(w[0]["params"], w[-1]["params"]) for w in want)
    return together


# ---- 1. the grouped step against the run alone ------------------------------------------------------------------------------------------
DV_CASES = [(1, DV.FD, 3), (2, DV.FD, 5), (3, SMALL_DV, 300), (8, SMALL_DV, 2), (5, dict(DV.FD, num_nodes=20), 4)]


@pytest.mark.parametrize("R,cfg,bs", DV_CASES, ids=["R1-fd-bs3", "R2-fd-bs5", "R3-small-bs300", "R8-small-bs2", "R5-ncmapss-bs4"])
def test_dvgtformer_runs_stepped_together_equal_the_runs_alone_bit_for_bit(R, cfg, bs):
    """bs 300 is above the 256 partial rows: the backward's grid-stride wraps, the forward's grid is sized for the whole group."""
    cases = [DV.seeded_case(DV.items(cfg), bs, 300 + 11 * r)[1:] for r in range(R)]
    _stepped_together_equal_stepped_alone(lambda sd: DV.build_model(cfg, sd, dropout=0.1), cases, [{}] * R)


# (R, p, T, N, h, bs); 6h = 120 is the 128-wide LSTM form.  (8, 1, 1, 2, 1, 2) has windows of ONE point per sensor (T p = 1): the Pearson
# graph is 0 / 0 and, as in the reference, every value behind it is NaN -- the case holds the grouped call to the single call's bits
# all the same (the same NaNs), and the case behind it (two points per sensor) is the same group count on finite values.
LG_CASES = [(2, 10, 5, 14, 8, 6), (3, 2, 3, 2, 1, 300), (2, 3, 2, 3, 20, 4), (8, 1, 1, 2, 1, 2), (8, 2, 1, 2, 1, 2)]
LG_IDS = ["R2-fd001-bs6", "R3-small-bs300", "R2-h20-bs4", "R8-one-point-bs2", "R8-tiny-bs2"]


def _logo_case(cfg, bs, seed):
    """(state dict, x, y): test_logo_gpu.seeded_case's -- advanced until half of the samples pass open ReLUs -- where the window has more
    than one point; its recipe without that search where every value is NaN and the search would never end."""
    if cfg["num_patch"] * cfg["patch_size"] > 1:
        return LG.seeded_case(tuple(cfg.items()), bs, seed)[1:]
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, (bs, cfg["num_nodes"], 1)).astype(np.float32)
    return LG.seeded_state(cfg, seed), x, rng.uniform(0, 1, bs).astype(np.float32)


@pytest.mark.parametrize("R,p,T,N,h,bs", LG_CASES, ids=LG_IDS)
def test_logo_runs_stepped_together_equal_the_runs_alone_bit_for_bit(R, p, T, N, h, bs):
    """Every run has its own theta as well: the graph backward takes it from the run's table entry."""
    cfg = LG.make_cfg(p, T, N, h)
    cases = [_logo_case(cfg, bs, 500 + 11 * r) for r in range(R)]
    finite = T * p > 1
    together = _stepped_together_equal_stepped_alone(lambda sd: LG.build_model(cfg, sd, dropout=0.2), cases,
                                                     [{"theta": 0.01 * (r + 1)} for r in range(R)], finite=finite)
    assert finite or all(torch.isnan(m.bucket[:m.num_live + 1]).any() for m in together)


# ---- 2. run 0 of the R = 2 cases against the fp64 oracles, at the families' own bars and gates ----------------------------------------------
def test_dvgtformer_run_0_of_a_grouped_step_matches_the_oracle():
    from gnn_rul_benchmarking_amd.runs import fused_group_step
    _, cfg, bs = DV_CASES[1]
    cases = [DV.seeded_case(DV.items(cfg), bs, 300 + 11 * r) for r in range(2)]
    models = [DV.build_model(cfg, c[1]).train() for c in cases]
    outs = fused_group_step(models, [None, None], [dev(c[2]) for c in cases], [dev(c[3]) for c in cases])
    _, sd, x, y = cases[0]
    o = DO.forward_backward(sd, x, y, cfg)
    g32 = DO.torch_grads(sd, x, y, cfg, torch.float32)[2]
    DV.check_forward("group-run0", models[0], bs, outs[0][0], outs[0][1], o, o["loss"])
    DV.check_grads("group-run0", grads_of(models[0]), o["grads"], g32, cfg)


@pytest.mark.parametrize("case", [LG_CASES[0], LG_CASES[2]], ids=["fd001", "h20"])
def test_logo_run_0_of_a_grouped_step_matches_the_oracle(case):
    from gnn_rul_benchmarking_amd.runs import fused_group_step
    _, p, T, N, h, bs = case
    cfg = LG.make_cfg(p, T, N, h)
    cases = [LG.seeded_case(tuple(cfg.items()), bs, 500 + 11 * r) for r in range(2)]
    models = [LG.build_model(cfg, c[1]).train() for c in cases]
    thetas = [0.01, 0.02]
    outs = fused_group_step(models, [None, None], [dev(c[2]) for c in cases], [dev(c[3]) for c in cases], [{"theta": t} for t in thetas])
    _, sd, x, y = cases[0]
    loss64, g64, fw = LO.loss_and_grads(sd, x, y, cfg, thetas[0])
    _, _, g32 = LO.torch_grads(sd, x, y, cfg, thetas[0], torch.float32)
    LG.check_forward("group-run0", models[0], bs, outs[0][0], outs[0][1], fw, loss64)
    LG.check_grads("group-run0", grads_of(models[0]), g64, g32)


# ---- 3. the runs classes against plain algorithms, on the recipe of tests/test_bilstm_group_gpu.py ------------------------------------------
RUN_IDS = (0, 1, 2)


def _tables(method, subset="FD001"):
    from gnn_rul_benchmarking_amd import hparams as HP
    hp = HP.get_hparams_class("CMAPSS")(subset)
    return dict(hp.alg_hparams[method]), dict(hp.train_params[method])


def _batches(bs=6):
    g = torch.Generator(device="cpu").manual_seed(3)
    return [(torch.rand(bs, 14, 50, generator=g).to(DEV), torch.rand(bs, 1, generator=g).to(DEV)) for _ in RUN_IDS]


def _state(algo):
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in algo.state_dict().items()}


@pytest.mark.parametrize("method", ["DVGTformer", "LOGO"])
def test_runs_class_takes_the_steps_the_plain_algorithms_take_alone(method):
    """FD001 hparams, batch 6, three updates, dropout on: the runs class over run ids (0, 1, 2), each on its own batch, against the three
    plain algorithms built and stepped alone under ``RunGenerators``: the losses and every state_dict entry with torch.equal."""
    from gnn_rul_benchmarking_amd import runs as R
    from gnn_rul_benchmarking_amd.algorithms import get_algorithm_class
    cfg, tc = _tables(method)
    plain = get_algorithm_class(method)
    batches = _batches()
    alone = []
    for run_id, (X, y) in zip(RUN_IDS, batches):
        with R.RunGenerators(run_id, DEV).active():
            algo = plain(cfg, tc, torch.device(DEV))
            algo.to(DEV)
            algo.train()
            losses = [algo.update(X, y, 1)["loss"] for _ in range(STEPS)]
        alone.append((losses, _state(algo), algo.model._step, algo.optimizer._steps))
    group = R.get_runs_class(method)(cfg, tc, torch.device(DEV), RUN_IDS)
    group.train()
    assert all(type(a) is plain for a in group.runs)
    steps = [group.update([b[0] for b in batches], [b[1] for b in batches], 1) for _ in range(STEPS)]
    for r, (losses, sd, model_step, adam_steps) in enumerate(alone):
        got = [s[r]["loss"] for s in steps]
        print(f"{method} run {RUN_IDS[r]}: losses together {got} alone {losses}")
        assert all(isinstance(v, float) and np.isfinite(v) for v in got) and got == losses
        mine = _state(group.runs[r])
        assert list(mine) == list(sd)
        for k in sd:
            assert torch.equal(mine[k], sd[k]), (r, k)
        assert (group.runs[r].model._step, group.runs[r].optimizer._steps) == (model_step, adam_steps) == (STEPS, STEPS)
    first = [s["loss"] for s in steps[0]]
    assert len(set(first)) == len(first)                                # other seeds, other batches
    group.eval()
    with torch.no_grad():
        assert group.runs[1].model(batches[1][0]).shape == (6, 1)
    group.train()
    with pytest.raises(ValueError, match="one batch size"):
        group.update([batches[0][0], batches[1][0][:4], batches[2][0]], [batches[0][1], batches[1][1][:4], batches[2][1]], 1)


# ---- 4. --concurrent_runs against the sequential loop, on the recipe of test_concurrent_runs_write_what_the_sequential_loop_writes ---------
def _write_dataset(root, n_train=64, n_test=40, window=50):
    rng = np.random.default_rng(0)
    d = os.path.join(root, "CMAPSS", "FD001")
    os.makedirs(d)
    for name, n in (("train.pt", n_train), ("test.pt", n_test)):
        x = rng.uniform(0, 1, (n, window, 14)).astype(np.float32)
        y = np.clip(x.mean(axis=(1, 2)) * 1.5 - 0.25, 0, 1).astype(np.float32)
        torch.save({"samples": x, "labels": y, "max_ruls": 125}, os.path.join(d, name))


def _train(tmp_path, method, tag, **extra):
    from gnn_rul_benchmarking_amd.trainer import GNN_RUL_trainer
    args = argparse.Namespace(save_dir=str(tmp_path / tag), experiment_description="exp", run_description="r", GNN_method=method,
                              data_path=str(tmp_path / "data"), dataset="CMAPSS", dataset_id="FD001", bearing_id="Testing_bearing_1",
                              num_runs=2, device=DEV, window=None, num_epochs=2, **extra)
    tr = GNN_RUL_trainer(args)
    tr.train_configs["batch_size"] = 16
    assert tr.train_configs["num_epochs"] == 2
    tr.train()
    root = tmp_path / tag / "exp" / "r"
    files = sorted(re.sub(r"logs_[0-9_]+\.log$", "logs_<time>.log", os.path.relpath(os.path.join(d, f), root))
                   for d, _, fs in os.walk(root) for f in fs)
    return root, files


@pytest.mark.parametrize("method", ["DVGTformer", "LOGO"])
def test_concurrent_runs_write_what_the_sequential_loop_writes(method, tmp_path, monkeypatch):
    """64 training windows of 14 x 50, batch 16, 2 epochs, ``--num_runs 2``: once through the unchanged sequential loop (the reference
    here), once with ``--concurrent_runs 2``.  Same files (a log's name carries its time stamp), as many rows per results.csv, every
    entry equal: the grouped step is bit-equal to the single one and nothing else differs between the loops."""
    _write_dataset(str(tmp_path / "data"))
    monkeypatch.chdir(tmp_path)
    seq_root, seq_files = _train(tmp_path, method, "seq")
    con_root, con_files = _train(tmp_path, method, "con", concurrent_runs=2)
    run_dirs = [f"{method}_run_0", f"{method}_run_1"]
    assert seq_files == con_files
    assert {os.path.basename(f) for f in seq_files} == {"results.csv", "results.pt", "checkpoint.pt", "logs_<time>.log"}
    assert {os.path.dirname(f) for f in seq_files} == set(run_dirs)
    worst, tables = 0.0, []
    for run in run_dirs:
        a, b = pd.read_csv(seq_root / run / "results.csv"), pd.read_csv(con_root / run / "results.csv")
        assert list(a.columns) == list(b.columns) == ["Score_v1", "Score_v2", "MAE", "RMSE"]
        assert len(a) == len(b) >= 2 and np.isinf(b.iloc[0]).all()
        va, vb = a.iloc[1:].to_numpy(np.float64), b.iloc[1:].to_numpy(np.float64)
        assert np.isfinite(va).all() and np.isfinite(vb).all()
        worst = max(worst, float(np.max(np.abs(vb - va) / np.abs(va))))
        tables.append(vb)
        ca = torch.load(seq_root / run / "checkpoint.pt", weights_only=False)
        cb = torch.load(con_root / run / "checkpoint.pt", weights_only=False)
        assert set(ca) == set(cb) and list(ca["model_dict"]) == list(cb["model_dict"])
        for k, v in ca["model_dict"].items():
            assert torch.equal(v, cb["model_dict"][k]), (run, k)
    print(f"{method}: largest relative difference of a results.csv entry, sequential vs --concurrent_runs 2: {worst:.3e}")
    assert worst == 0.0
    assert tables[0].shape != tables[1].shape or not np.array_equal(tables[0], tables[1])            # two seeds, two runs


# ---- 5. a configuration the kernels do not cover ---------------------------------------------------------------------------------------
def test_fd003_through_logo_runs_is_refused_and_launches_nothing():
    from gnn_rul_benchmarking_amd.runs import LOGO_runs
    cfg, tc = _tables("LOGO", "FD003")
    assert cfg["hidden_dim"] == 32
    group = LOGO_runs(cfg, tc, torch.device(DEV), (0, 1))
    group.train()
    batches = _batches()[:2]
    with pytest.raises(RuntimeError, match="do not cover this configuration"):
        group.update([b[0] for b in batches], [b[1] for b in batches], 1)
    torch.cuda.synchronize()
    assert all(not a.model.bucket.any() for a in group.runs)
