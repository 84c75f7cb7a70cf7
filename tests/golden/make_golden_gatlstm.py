"""Golden fixtures for the GAT_LSTM path, produced by RUNNING THE REFERENCE on the CPU.

    python tests/golden/make_golden_gatlstm.py     # needs the reference checkout (make_golden.py: RUL_REFERENCE; read-only import)

Only data is written (inputs, weights, the outputs / gradients the reference produced, its hparams rows); see make_golden.py for the
shims.  Weights are the constructor's under torch.manual_seed(seed), moved away from init by uniform(-0.1, 0.1) from
torch.Generator().manual_seed(seed + 1000) in state_dict order: at fresh initialisation the output is almost independent of the input.
The reference's F.dropout draws from torch's Bernoulli stream, which no other implementation reproduces: the train-mode cases set the
layers' ``dropout`` attribute to 0 on the constructed instance.

Every case stores the reference's fp64 run (the model in double) as the expected values and its fp32 gradients under ``refgrad:`` keys
(tests/grad_cases.py globs for ``grad:``); the maker asserts that the reference's own fp32 forward stays within 1e-5 of its fp64 one,
relative to the largest prediction.  Every case holds every tap (the features, each GAT layer's output, the LSTM output) and all 22
gradients in both precisions.  The small cases hold their weights; the full-width geometry cases hold the seed and a checksum of the
weights instead -- the tests rebuild the weights from the seed and assert the checksum -- and are written as four files, each below
1 MiB: ``<name>.npz`` (input, predictions, loss, the features and the LSTM output), ``<name>_taps.npz`` (the GAT layers' outputs),
``<name>_grad64.npz`` and ``<name>_refgrad.npz``.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as mg                                   # noqa: E402  (installs the shims, sets sys.path)
from models.GAT_LSTM import Model as ref_model             # noqa: E402
from algorithms.algorithms import get_algorithm_class      # noqa: E402
from configs.hparams import get_hparams_class              # noqa: E402
import gatlstm_oracle as GO                                # noqa: E402


def seeded_model(cfg, seed):
    torch.manual_seed(seed)
    m = ref_model.GAT_LSTM_model(**cfg)
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        m.load_state_dict({k: v + torch.empty_like(v).uniform_(-0.1, 0.1, generator=g) for k, v in m.state_dict().items()})
    return m


def dropout_off(m):
    for layer in m.gat_layers:
        layer.dropout = 0.0


def run_with_taps(m, x):
    taps = {}
    hs = [m.gat_layers[0].register_forward_pre_hook(lambda mod, a: taps.update(feat=a[0].detach().numpy().copy()))]
    for l, layer in enumerate(m.gat_layers):
        hs.append(layer.register_forward_hook(lambda mod, a, out, l=l: taps.update({f"h{l}": out.detach().numpy().copy()})))
    hs.append(m.lstm_layers[-1].register_forward_hook(lambda mod, a, out: taps.update(lstm=out[0].detach().numpy().copy())))
    pred = m(x)
    for h in hs:
        h.remove()
    return pred, taps


def cfg_entries(cfg):
    return {"cfg_json": np.array(json.dumps(cfg, sort_keys=True))}


def case_forward_backward(name, cfg, bs, seed, full, x_np=None):
    m = seeded_model(cfg, seed)
    sd = {k: v.detach().numpy() for k, v in m.state_dict().items()}
    if x_np is None:
        x_np = GO.seeded_input(cfg, bs, seed)
    y = torch.rand(bs, 1, generator=torch.Generator().manual_seed(seed + 8))
    out = {"x": x_np, "y": y.numpy().copy(), "seed": np.int64(seed), **cfg_entries(cfg)}
    flat = np.concatenate([v.astype(np.float64).ravel() for v in sd.values()])
    out["checksum"] = np.array([flat.sum(), (flat * flat).sum()], np.float64)
    m.train()
    dropout_off(m)
    # the reference in fp32: its prediction and gradients as it computes them
    pred32, taps32 = run_with_taps(m, torch.tensor(x_np))
    loss32 = torch.nn.functional.mse_loss(pred32, y)
    m.zero_grad()
    loss32.backward()
    for n_, p in m.named_parameters():
        out["refgrad:" + n_] = p.grad.numpy().copy()
    out["pred32"] = pred32.detach().numpy().copy()
    # ... and in fp64: the expected values
    m.double()
    m.eval()
    with torch.no_grad():
        out["pred_eval"] = m(torch.tensor(x_np).double()).numpy().copy()
    m.train()
    pred, taps = run_with_taps(m, torch.tensor(x_np).double())
    loss = torch.nn.functional.mse_loss(pred, y.double())
    m.zero_grad()
    loss.backward()
    out["pred"], out["loss"] = pred.detach().numpy().copy(), np.float64(loss.item())
    for k in ("feat", "lstm") + tuple(f"h{l}" for l in range(len(cfg["hidden_dim"]))):
        out["tap:" + k] = taps[k]
    for n_, p in m.named_parameters():
        out["grad64:" + n_] = p.grad.numpy().copy()
    if full:
        for k, v in sd.items():
            out["sd:" + k] = v
    fin = np.isfinite(out["pred"])
    scale = max(float(np.abs(out["pred"][fin]).max()), 1e-30) if fin.any() else 1.0
    assert np.array_equal(np.isfinite(out["pred32"]), fin), "fp32 and fp64 NaN in different samples"
    err = float(np.abs(out["pred32"][fin] - out["pred"][fin]).max()) / scale if fin.any() else 0.0
    assert err < 1e-5, err
    parts = {"": out}
    if not full:                                            # four files, each within the size limit of a committed file
        pick = lambda pre: {k: out.pop(k) for k in [k for k in out if k.startswith(pre)]}      # noqa: E731
        parts = {"_taps": pick("tap:h"), "_grad64": pick("grad64:"), "_refgrad": pick("refgrad:"), "": out}
    for suffix, content in parts.items():
        path = os.path.join(HERE, name + suffix + ".npz")
        np.savez_compressed(path, **content)
        assert os.path.getsize(path) < 1 << 20, (path, os.path.getsize(path))
        print("wrote", name + suffix, os.path.getsize(path), "bytes")
    print("     ", name, out["pred"].ravel()[:4], "loss", out["loss"], "fp32-fp64", err)


def case_nan(name, cfg, seed):
    """A batch of 3: sample 0 holds one patch constant at 0.5 (std = 0: NaN skewness and kurtosis), sample 1 is clean, sample 2 holds one
    all-zero patch (NaN also in the four factors).  Sums of those values are exact in any order, so the NaNs do not depend on the
    summation order; the maker asserts fp32 and fp64 give NaN in the same samples."""
    x = GO.seeded_input(cfg, 3, seed).reshape(3, cfg["num_patch"], cfg["patch_size"])
    x[0, 1] = 0.5
    x[2, cfg["num_patch"] - 1] = 0.0
    case_forward_backward(name, cfg, 3, seed, True, x.reshape(3, -1))
    z = np.load(os.path.join(HERE, name + ".npz"))
    assert np.isnan(z["pred_eval"]).reshape(-1).tolist() == [True, False, True] and np.isnan(z["pred32"]).reshape(-1).tolist() == [True, False, True]
    f = z["tap:feat"]
    assert np.isnan(f[0, 1, [5, 6]]).all() and not np.isnan(f[0, 1, [0, 1, 2, 3, 4, 7, 8, 9, 10]]).any()
    assert np.isnan(f[2, -1, [5, 6, 7, 8, 9, 10]]).all() and np.isnan(f).sum() == 8


def case_training_curve(name, cfg, bs, steps, seed, lr, wd):
    """The reference's own GAT_LSTM.update (algorithms.py:508-517) on fixed batches, dropout 0, from perturbed weights."""
    torch.manual_seed(seed)
    algo = get_algorithm_class("GAT_LSTM")(cfg, {"learning_rate": lr, "weight_decay": wd}, "cpu")
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        algo.model.load_state_dict({k: v + torch.empty_like(v).uniform_(-0.1, 0.1, generator=g) for k, v in algo.model.state_dict().items()})
    sd0 = {k: v.detach().numpy().copy() for k, v in algo.model.state_dict().items()}
    xs = np.stack([GO.seeded_input(cfg, bs, seed + 31 * s) for s in range(steps)])
    ys = torch.rand(steps, bs, 1, generator=torch.Generator().manual_seed(seed + 8))
    out = {"xs": xs, "ys": ys.numpy().copy(), "lr": np.float64(lr), "wd": np.float64(wd), "seed": np.int64(seed), **cfg_entries(cfg)}
    for k, v in sd0.items():
        out["sd0:" + k] = v
    algo.train()
    losses = []
    for s in range(steps):
        losses.append(algo.update(torch.tensor(xs[s]), ys[s], 1)["loss"])
        if s + 1 in (1, 10, 20):
            for k, v in algo.model.state_dict().items():
                out[f"sd{s + 1}:" + k] = v.detach().numpy().copy()
    out["losses"] = np.asarray(losses, dtype=np.float64)
    algo.eval()
    with torch.no_grad():
        out["eval_pred_end"] = algo.model(torch.tensor(xs[0])).numpy().copy()
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print("wrote", name, losses[:3], "...", losses[-1])


def case_trainer_phm2012(name, seed, n_train=40, n_test=20, epochs=3):
    """The reference's OWN harness with --GNN_method GAT_LSTM on the synthetic PHM2012 Condition_1 dataset of synth.py with its own hparams
    (40 patches of 64 points, batch 100, lr 1e-4, wd 1e-4; no shuffling); num_epochs patched, the row's dropout set to 0."""
    import argparse
    import tempfile
    import trainer as ref_trainer
    from synth import synthetic_phm2012
    _orig_load = torch.load
    torch.load = lambda *a, **k: _orig_load(*a, **{**k, "weights_only": False})
    (xtr, ytr), (xte, yte) = synthetic_phm2012(seed, n_train, n_test)
    with tempfile.TemporaryDirectory() as tmp:
        d = os.path.join(tmp, "data", "PHM2012", "Condition_1")
        os.makedirs(d)
        torch.save({"samples": xtr, "labels": ytr, "max_ruls": 1.0}, os.path.join(d, "train.pt"))
        torch.save({"samples": xte, "labels": yte, "max_ruls": 1.0}, os.path.join(d, "test.pt"))
        cwd = os.getcwd()
        os.chdir(tmp)
        try:
            args = argparse.Namespace(save_dir=os.path.join(tmp, "logs"), experiment_description="exp", run_description="r",
                                      GNN_method="GAT_LSTM", data_path=os.path.join(tmp, "data"), dataset="PHM2012",
                                      dataset_id="Condition_1", bearing_id="Testing_bearing_1", num_runs=1, device="cpu")
            tr = ref_trainer.GNN_RUL_trainer(args)
            tr.train_configs["num_epochs"] = epochs
            tr.model_configs["dropout"] = 0.0
            per_epoch = []
            orig = tr.calc_results_per_run

            def spy(run_id):
                per_epoch.append(mg.ref_utils._calc_metrics(tr.pred_labels, tr.true_labels, tr.max_ruls))
                return orig(run_id)
            tr.calc_results_per_run = spy
            tr.train()
            final = {k: v.detach().numpy().copy() for k, v in tr.algorithm.model.state_dict().items()}
            csv_text = open(os.path.join(tmp, "logs", "exp", "r", "GAT_LSTM_run_0", "results.csv")).read()
        finally:
            os.chdir(cwd)
            torch.load = _orig_load
    out = {"seed": np.int64(seed), "n_train": np.int64(n_train), "n_test": np.int64(n_test), "epochs": np.int64(epochs),
           "per_epoch": np.asarray(per_epoch, np.float64), "csv_text": np.array(csv_text),
           "x_train_checksum": np.float64(xtr.astype(np.float64).sum()),
           "batch_size": np.int64(tr.train_configs["batch_size"]), "lr": np.float64(tr.train_configs["learning_rate"])}
    for k in ("gat_layers.0.linear.bias", "gat_layers.2.attention.weight", "lstm_layers.1.bias_hh_l0", "fc.weight"):
        out["final:" + k] = final[k]
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print("wrote", name, np.asarray(per_epoch))


def case_hparams(name):
    rows = {}
    for ds in ("PHM2012", "XJTU_SY"):
        for did in ("Condition_1", "Condition_2", "Condition_3"):
            hp = get_hparams_class(ds)(did)
            rows[f"{ds}/{did}"] = {"train_params": hp.train_params["GAT_LSTM"], "alg_hparams": hp.alg_hparams["GAT_LSTM"]}
    absent = []
    for ds, ids in (("CMAPSS", ["FD001", "FD002", "FD003", "FD004"]), ("NCMAPSS", [None])):
        for did in ids:
            hp = get_hparams_class(ds)(did) if did is not None else get_hparams_class(ds)()
            assert "GAT_LSTM" not in hp.alg_hparams
            absent.append(f"{ds}/{did}")
    np.savez_compressed(os.path.join(HERE, name + ".npz"), rows_json=np.array(json.dumps(rows, sort_keys=True)),
                        absent_json=np.array(json.dumps(absent)))
    print("wrote", name, rows)


if __name__ == "__main__":
    base = dict(hidden_dim=[300, 200, 100], lstm_hidden_dim=[30, 20], dropout=0.2)
    small = dict(num_patch=3, patch_size=4, hidden_dim=[5, 4, 3], lstm_hidden_dim=[3, 2], dropout=0.2)
    odd = dict(num_patch=5, patch_size=8, hidden_dim=[7, 3], lstm_hidden_dim=[4], dropout=0.2)
    case_hparams("gatlstm_hparams_rows")
    case_forward_backward("gatlstm_small_t3_p4_bs4", small, 4, 51, True)
    case_forward_backward("gatlstm_small_t5_p8_bs3", odd, 3, 52, True)
    case_nan("gatlstm_nan_t5_p8_bs3", odd, 56)
    case_forward_backward("gatlstm_geom_40x64_bs2", dict(base, num_patch=40, patch_size=64), 2, 53, False)
    case_forward_backward("gatlstm_geom_80x32_bs2", dict(base, num_patch=80, patch_size=32), 2, 54, False)
    case_forward_backward("gatlstm_geom_32x1024_bs2", dict(base, num_patch=32, patch_size=1024), 2, 55, False)
    hp = get_hparams_class("PHM2012")("Condition_1").train_params["GAT_LSTM"]
    case_training_curve("gatlstm_train_curve_t5_p8_bs8", dict(odd, dropout=0.0), 8, 20, 57, hp["learning_rate"], hp["weight_decay"])
    if "--no-trainer" not in sys.argv:
        case_trainer_phm2012("gatlstm_trainer_phm2012_c1_reference_run", 58)
