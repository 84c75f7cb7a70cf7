"""-m gpu: the grouped Bi-LSTM kernels (csrc/bilstm.hip, workgroup = (group, direction, sequence)) against the single-layer entry and the
numpy oracle; ``runs.HAGCN_runs`` against plain ``HAGCN`` objects stepped alone; ``--concurrent_runs`` against the sequential loop."""
import argparse
import contextlib
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch

from oracle import hagcn_oracle as O
from test_hagcn_oracle_golden import rel
from test_hagcn_gpu import TOL, GTOL            # that file's bars for the same quantities: layer output 1e-4, gradients 1e-3

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (G, Bq, T, I, H)
GROUP_CASES = [
    (1, 2, 9, 3, 16),         # degenerate group count
    (2, 1, 1, 4, 64),         # one step
    (3, 3, 8, 6, 5),          # T = LSTM_AHEAD, lanes beyond H
    (2, 2, 9, 7, 60),         # ring wrap, the KLIVE form
    (3, 1, 33, 9, 64),
    (2, 2, 17, 10, 120),
    (2, 1, 12, 8, 128),
    (8, 1, 10, 5, 8),         # maximum group count
    (5, 2, 140, 25, 60),      # the protocol's five seeds on a short FD004-like sequence
]


@pytest.mark.parametrize("G,Bq,T,I,H", GROUP_CASES)
def test_grouped_layers_equal_the_single_entry_bit_for_bit_and_match_the_oracle(G, Bq, T, I, H):
    """Independently drawn weights, inputs and output weights per group (a crossed pointer shows): group g's out, dx and eight parameter
    gradients are bit-equal to ``bilstm_sum`` on group g's tensors alone -- the same step body per workgroup, the same GEMM calls and
    the same split-K batch per group -- and groups 0 and G - 1 agree with the fp64 oracle at tests/test_hagcn_gpu.py's bars."""
    from gnn_rul_benchmarking_amd.hagcn import bilstm_sum, bilstm_sum_group
    rng = np.random.default_rng(1000 * G + 10 * T + H)
    torch.manual_seed(G * 131 + T)
    lstms = [torch.nn.LSTM(I, H, 1, batch_first=True, bidirectional=True).to(DEV) for _ in range(G)]
    xs = [rng.normal(size=(Bq, T, I)) for _ in range(G)]
    ws = [rng.normal(size=(Bq, T, H)) for _ in range(G)]
    wt = [torch.from_numpy(w.astype(np.float32)).to(DEV) for w in ws]

    def inputs():
        return [torch.from_numpy(x.astype(np.float32)).to(DEV).requires_grad_(True) for x in xs]

    def grads_of(lstm):
        got = {k: v.grad.clone() for k, v in lstm.named_parameters()}
        for v in lstm.parameters():
            v.grad = None
        return got

    xg = inputs()
    outs = bilstm_sum_group(lstms, xg)
    assert isinstance(outs, tuple) and len(outs) == G
    sum((o * w).sum() for o, w in zip(outs, wt)).backward()
    torch.cuda.synchronize()
    grouped = [(outs[g].detach().clone(), xg[g].grad.clone(), grads_of(lstms[g])) for g in range(G)]

    xa = inputs()
    for g in range(G):
        out = bilstm_sum(lstms[g], xa[g])
        (out * wt[g]).sum().backward()
        single = grads_of(lstms[g])
        assert torch.equal(grouped[g][0], out.detach()), f"out of group {g}"
        assert torch.equal(grouped[g][1], xa[g].grad), f"dx of group {g}"
        assert set(single) == set(grouped[g][2]) and len(single) == 8
        for k in single:
            assert torch.equal(grouped[g][2][k], single[k]), f"{k} of group {g}"

    for g in sorted({0, G - 1}):
        p = {"L." + k: v.detach().cpu().numpy().astype(np.float64) for k, v in lstms[g].state_dict().items()}
        assert rel(grouped[g][0].cpu().numpy(), O.bilstm_sum(xs[g], p, "L")) < TOL
        dx, ref = O.bilstm_sum_backward(xs[g], p, "L", ws[g])
        assert rel(grouped[g][1].cpu().numpy(), dx) < GTOL
        for k, v in grouped[g][2].items():
            assert rel(v.cpu().numpy(), ref["L." + k]) < GTOL, (g, k)


def test_more_groups_than_the_kernels_take_is_an_error_not_a_fallback():
    from gnn_rul_benchmarking_amd.hagcn import bilstm_sum_group
    lstms = [torch.nn.LSTM(3, 4, 1, batch_first=True, bidirectional=True).to(DEV) for _ in range(9)]
    with pytest.raises(RuntimeError, match="rulgnn_bilstm_forward_group_f32"):
        bilstm_sum_group(lstms, [torch.rand(1, 5, 3, device=DEV) for _ in range(9)])


# ---- HAGCN_runs against plain HAGCN objects, on the recipe of test_deferred_lstm_weight_gradients_give_the_same_step --------------------
RUN_IDS = (0, 1, 2)
STEPS = 3


def _tables():
    from gnn_rul_benchmarking_amd import hparams as HP
    hp = HP.get_hparams_class("CMAPSS")("FD004")
    return dict(hp.alg_hparams["HAGCN"]), dict(hp.train_params["HAGCN"])


def _batches():
    g = torch.Generator(device="cpu").manual_seed(3)
    return [(torch.rand(24, 14, 50, generator=g).to(DEV), torch.rand(24, 1, generator=g).to(DEV)) for _ in RUN_IDS]


def _state(algo):
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in algo.model.state_dict().items()}, algo.model.last_topk.clone()


@pytest.fixture(scope="module")
def runs_alone():
    """Per run id: (losses, state dict, last_topk) of a plain HAGCN built and stepped alone under that run's generator states."""
    from gnn_rul_benchmarking_amd.algorithms import HAGCN
    from gnn_rul_benchmarking_amd.runs import RunGenerators
    cfg, tc = _tables()
    out = []
    for run_id, (X, y) in zip(RUN_IDS, _batches()):
        with RunGenerators(run_id, DEV).active():
            algo = HAGCN(cfg, tc, torch.device(DEV))
            algo.to(DEV)
            algo.train()
            losses = [algo.update(X, y, 1)["loss"] for _ in range(STEPS)]
        out.append((losses, *_state(algo)))
    return out


@pytest.mark.parametrize("deferred", [True, False])
def test_runs_stepped_together_take_the_steps_they_take_alone(runs_alone, deferred, monkeypatch):
    """FD004 hparams, batch 24, three updates, dropout on: ``HAGCN_runs`` over run ids (0, 1, 2), each on its own batch, against the three
    plain runs -- at the bars of "same step, other schedule" (tests/test_hagcn_gpu.py): losses rtol 1e-6, every state_dict entry atol
    2e-6, and the node selection of the last step exactly.  ``deferred=False``: the same with everything on one stream."""
    from gnn_rul_benchmarking_amd import runs as R
    from gnn_rul_benchmarking_amd.algorithms import HAGCN
    cfg, tc = _tables()
    if not deferred:
        monkeypatch.setattr(R, "deferred_weight_gradients", lambda device: contextlib.nullcontext())
    batches = _batches()
    group = R.HAGCN_runs(cfg, tc, torch.device(DEV), RUN_IDS)
    group.train()
    assert all(type(a) is HAGCN for a in group.runs)
    steps = [group.update([b[0] for b in batches], [b[1] for b in batches], 1) for _ in range(STEPS)]
    for r, (losses, sd, topk) in enumerate(runs_alone):
        got = [s[r]["loss"] for s in steps]
        print(f"run {RUN_IDS[r]}: losses together {got} alone {losses}")
        assert all(np.isfinite(got)) and np.allclose(got, losses, rtol=1e-6, atol=0)
        mine, my_topk = _state(group.runs[r])
        assert set(mine) == set(sd) and len(sd) == 67
        for k in sd:
            assert torch.allclose(mine[k].float(), sd[k].float(), rtol=0, atol=2e-6), (r, k)
        assert torch.equal(my_topk, topk)
    group.eval()
    with torch.no_grad():
        assert group.runs[1].model(batches[1][0]).shape == (24, 1)
    assert losses_differ_between_runs(steps)


def losses_differ_between_runs(steps):
    first = [s["loss"] for s in steps[0]]
    return len(set(first)) == len(first)          # other seeds, other batches: a run that got another run's tensors would show here too


# ---- --concurrent_runs against the sequential loop -----------------------------------------------------------------------------------
# Largest relative difference of any results.csv entry between the two loops, measured on an MI355X before the bar was set: 0 -- the
# grouped kernels are bit-equal to the single ones and nothing else differs between the loops (profiles/r35_hagcn_runs.md).  The bar is
# ten times the measurement and never looser than 1e-4 relative (the LSTM output bar of tests/test_hagcn_gpu.py): here, equality.
TRAINER_MEASURED = 0.0
TRAINER_RTOL = min(10 * TRAINER_MEASURED, 1e-4)


def _write_dataset(root, n_train=64, n_test=40, window=50):
    rng = np.random.default_rng(0)
    d = os.path.join(root, "CMAPSS", "FD004")
    os.makedirs(d)
    for name, n in (("train.pt", n_train), ("test.pt", n_test)):
        x = rng.uniform(0, 1, (n, window, 14)).astype(np.float32)
        y = np.clip(x.mean(axis=(1, 2)) * 1.5 - 0.25, 0, 1).astype(np.float32)
        torch.save({"samples": x, "labels": y, "max_ruls": 125}, os.path.join(d, name))


def _train(tmp_path, tag, **extra):
    from gnn_rul_benchmarking_amd.trainer import GNN_RUL_trainer
    args = argparse.Namespace(save_dir=str(tmp_path / tag), experiment_description="exp", run_description="r", GNN_method="HAGCN",
                              data_path=str(tmp_path / "data"), dataset="CMAPSS", dataset_id="FD004", bearing_id="Testing_bearing_1",
                              num_runs=2, device=DEV, window=None, num_epochs=2, **extra)
    tr = GNN_RUL_trainer(args)
    tr.train_configs["batch_size"] = 16
    assert tr.model_configs["patch_size"] == 50 and tr.train_configs["num_epochs"] == 2
    tr.train()
    root = tmp_path / tag / "exp" / "r"
    files = sorted(re.sub(r"logs_[0-9_]+\.log$", "logs_<time>.log", os.path.relpath(os.path.join(d, f), root))
                   for d, _, fs in os.walk(root) for f in fs)
    return root, files


def test_concurrent_runs_write_what_the_sequential_loop_writes(tmp_path, monkeypatch):
    """64 training windows of 14 x 50, batch 16, 2 epochs, ``--num_runs 2``: once through the unchanged sequential loop (the reference
    here), once with ``--concurrent_runs 2``.  Same files (a log's name carries its time stamp), as many rows per results.csv, every
    metric within TRAINER_RTOL."""
    _write_dataset(str(tmp_path / "data"))
    monkeypatch.chdir(tmp_path)
    seq_root, seq_files = _train(tmp_path, "seq")
    con_root, con_files = _train(tmp_path, "con", concurrent_runs=2)
    assert seq_files == con_files
    assert {os.path.basename(f) for f in seq_files} == {"results.csv", "results.pt", "checkpoint.pt", "logs_<time>.log"}
    assert {os.path.dirname(f) for f in seq_files} == {"HAGCN_run_0", "HAGCN_run_1"}
    worst = 0.0
    for run in ("HAGCN_run_0", "HAGCN_run_1"):
        a, b = pd.read_csv(seq_root / run / "results.csv"), pd.read_csv(con_root / run / "results.csv")
        assert list(a.columns) == list(b.columns) == ["Score_v1", "Score_v2", "MAE", "RMSE"]
        assert len(a) == len(b) >= 2 and np.isinf(b.iloc[0]).all()
        va, vb = a.iloc[1:].to_numpy(np.float64), b.iloc[1:].to_numpy(np.float64)
        assert np.isfinite(va).all() and np.isfinite(vb).all()
        worst = max(worst, float(np.max(np.abs(vb - va) / np.abs(va))))
        ca = torch.load(seq_root / run / "checkpoint.pt", weights_only=False)
        cb = torch.load(con_root / run / "checkpoint.pt", weights_only=False)
        assert set(ca) == set(cb) and list(ca["model_dict"]) == list(cb["model_dict"])
    print(f"largest relative difference of a results.csv entry, sequential vs --concurrent_runs 2: {worst:.3e}")
    assert worst <= TRAINER_RTOL
    a0 = pd.read_csv(con_root / "HAGCN_run_0" / "results.csv").iloc[1:].to_numpy()
    a1 = pd.read_csv(con_root / "HAGCN_run_1" / "results.csv").iloc[1:].to_numpy()
    assert a0.shape != a1.shape or not np.array_equal(a0, a1)            # two seeds, two runs
