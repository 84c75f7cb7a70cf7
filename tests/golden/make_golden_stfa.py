"""Golden fixtures for the STFA path, produced by RUNNING THE REFERENCE on the CPU.

    python tests/golden/make_golden_stfa.py     # needs the reference checkout (make_golden.py: RUL_REFERENCE; read-only import)

Only data is written (inputs, weights, the outputs / gradients the reference produced, its hparams rows); see make_golden.py for the
shims.  One more shim is this file's own: the reference's STFA algorithm hard-codes ``configs['device'] = 'cuda:0'`` and
``prior_knowledge_graph(device)`` moves the adjacency there, so ``models.STFA.Model.prior_knowledge_graph`` is wrapped to build on the CPU.
Weights are the constructor's under torch.manual_seed(seed), moved away from init by uniform(-0.1, 0.1) from
torch.Generator().manual_seed(seed + 1000) in state_dict order.  The reference's F.dropout draws from torch's Bernoulli stream, which no
other implementation reproduces: the train-mode cases set the layers' ``dropout`` attribute to 0 on the constructed instance (the
curve and the harness run put ``dropout = 0`` into the config).

Every case stores the reference's fp64 run (the model in double) as the expected values and its fp32 gradients under ``refgrad:`` keys
(tests/grad_cases.py globs for ``grad:``), every tap (``gat``: the stage output [bs, T, 14 C]; ``rows``: the LSTM's input; ``lstm``) and
all 48 gradients in both precisions.  The small cases hold their weights; the full-width case holds the seed and a checksum of the
weights instead.  Asserted on every case:

  * the reference's own fp32 forward stays within 1e-5 of its fp64 one, relative to the largest prediction;
  * the KINK MARGIN: every leakyrelu argument and every ReLU argument of the fp64 run is farther from zero than 16 fp32 ulps (16 * 2^-23)
    of its tensor's largest magnitude -- a condition, not a measurement: a flipped kink is a discrete gradient difference that no
    tolerance covers.  ``pick_seed`` walks the seeds upwards from the requested one until it holds and prints what it skipped;
    The training curve asserts it at every state it stores together with the batch that meets it (steps 0, 1 and 10).  The harness run
    cannot hold it and does not pretend to: its 250 training windows put 12 million leakyrelu arguments in front of the constructed
    model, against 14 thousand in the curve; the margin at the start is stored as a measurement (``kink_margin_start``, 0.07) -- one
    flipped kink there moves one of those 12 million terms of a summed gradient by a tenth, seven orders below the harness test's bars;
  * zeroing the ``gat`` tap changes the prediction by more than 100 x the forward tolerance (1e-4): the stage matters in the fixture.
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
from models.STFA import Model as ref_model                 # noqa: E402
from algorithms.algorithms import get_algorithm_class      # noqa: E402
from configs.hparams import get_hparams_class              # noqa: E402
import stfa_oracle as SO                                   # noqa: E402

_orig_graph = ref_model.prior_knowledge_graph
ref_model.prior_knowledge_graph = lambda device: _orig_graph("cpu")      # the project's own shim: the reference asks for 'cuda:0'

TOL = 1e-4


def seeded_model(cfg, seed):
    torch.manual_seed(seed)
    m = ref_model.STFA_model(device="cpu", **cfg)
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        m.load_state_dict({k: v + torch.empty_like(v).uniform_(-0.1, 0.1, generator=g) for k, v in m.state_dict().items()})
    return m


def dropout_off(m):
    for layer in m.gat.attentions:
        layer.dropout = 0.0


def run_with_taps(m, x, zero_gat=False):
    taps = {}
    bs = x.shape[0]
    T = m.num_patch

    def gat_hook(mod, a, out):
        taps["gat"] = out.detach().numpy().reshape(bs, T, -1).copy()
        return torch.zeros_like(out) if zero_gat else None
    hs = [m.gat.register_forward_hook(gat_hook),
          m.lstm.register_forward_pre_hook(lambda mod, a: taps.update(rows=a[0].detach().numpy().copy())),
          m.lstm.register_forward_hook(lambda mod, a, out: taps.update(lstm=out[0].detach().numpy().copy()))]
    pred = m(x)
    for h in hs:
        h.remove()
    return pred, taps


def cfg_entries(cfg):
    return {"cfg_json": np.array(json.dumps(cfg, sort_keys=True))}


def margin_of(cfg, bs, seed, x_np=None):
    m = seeded_model(cfg, seed)
    sd = {k: v.detach().numpy() for k, v in m.state_dict().items()}
    x = SO.seeded_input(cfg, bs, seed) if x_np is None else x_np
    return SO.kink_margin(SO.forward_backward(sd, x, None, cfg))


def pick_seed(cfg, bs, start):
    for seed in range(start, start + 32):
        k = margin_of(cfg, bs, seed)
        if k > 1.0:
            return seed
        print(f"      seed {seed}: kink margin {k:.3f} <= 1, skipped")
    raise AssertionError("no seed holds the kink margin")


def case_forward_backward(name, cfg, bs, seed, full, x_np=None):
    m = seeded_model(cfg, seed)
    sd = {k: v.detach().numpy() for k, v in m.state_dict().items()}
    if x_np is None:
        x_np = SO.seeded_input(cfg, bs, seed)
    y = torch.rand(bs, 1, generator=torch.Generator().manual_seed(seed + 8))
    out = {"x": x_np, "y": y.numpy().copy(), "seed": np.int64(seed), **cfg_entries(cfg)}
    flat = np.concatenate([v.astype(np.float64).ravel() for v in sd.values()])
    out["checksum"] = np.array([flat.sum(), (flat * flat).sum()], np.float64)
    m.train()
    dropout_off(m)
    # the reference in fp32: its prediction and gradients as it computes them
    pred32, _ = run_with_taps(m, torch.tensor(x_np))
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
        pred_zero = run_with_taps(m, torch.tensor(x_np).double(), zero_gat=True)[0].numpy().copy()
    m.train()
    pred, taps = run_with_taps(m, torch.tensor(x_np).double())
    loss = torch.nn.functional.mse_loss(pred, y.double())
    m.zero_grad()
    loss.backward()
    out["pred"], out["loss"] = pred.detach().numpy().copy(), np.float64(loss.item())
    for k in ("gat", "rows", "lstm"):
        out["tap:" + k] = taps[k]
    for n_, p in m.named_parameters():
        assert p.grad is not None, n_                       # v's gradients are zeros, not None
        out["grad64:" + n_] = p.grad.numpy().copy()
    if np.isfinite(out["pred"]).all():                      # exactly zero, in both precisions
        assert not out["grad64:v.weight"].any() and not out["grad64:v.bias"].any()
        assert not out["refgrad:v.weight"].any() and not out["refgrad:v.bias"].any()
    if full:
        for k, v in sd.items():
            out["sd:" + k] = v
    fin = np.isfinite(out["pred"])
    scale = max(float(np.abs(out["pred"][fin]).max()), 1e-30) if fin.any() else 1.0
    assert np.array_equal(np.isfinite(out["pred32"]), fin), "fp32 and fp64 NaN in different samples"
    err = float(np.abs(out["pred32"][fin] - out["pred"][fin]).max()) / scale if fin.any() else 0.0
    assert err < 1e-5, err
    o = SO.forward_backward(sd, x_np, y.numpy(), cfg, want_grads=False)
    assert float(np.abs(o["pred"][fin] - out["pred"][fin]).max()) < 1e-9 * scale
    margin = SO.kink_margin(o)
    assert margin > 1.0, ("kink margin", margin)
    moved = float(np.abs(pred_zero[fin] - out["pred_eval"][fin]).max()) / scale
    assert moved > 100 * TOL, ("the gat stage does not matter", moved)
    out["kink_margin"], out["gat_matters"] = np.float64(margin), np.float64(moved)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1 << 20, (path, os.path.getsize(path))
    print("wrote", name, os.path.getsize(path), "bytes", out["pred"].ravel()[:4], "loss", out["loss"], "fp32-fp64", err, "kink margin", margin,
          "zeroed gat moves pred by", moved)


def case_nan(name, cfg, seed):
    """A batch of 3: sample 1 holds one NaN reading (sensor 4, in the second patch), samples 0 and 2 are clean."""
    x = SO.seeded_input(cfg, 3, seed)
    x[1, 4, cfg["patch_size"]] = np.nan
    case_forward_backward(name, cfg, 3, seed, True, x)
    z = np.load(os.path.join(HERE, name + ".npz"))
    assert np.isnan(z["pred_eval"]).reshape(-1).tolist() == [False, True, False] and np.isnan(z["pred32"]).reshape(-1).tolist() == [False, True, False]
    assert np.isnan(z["tap:lstm"][1]).all() and not np.isnan(z["tap:lstm"][[0, 2]]).any()       # poisoned from step 0 (the singleton softmax)


def case_training_curve(name, cfg, bs, steps, seed, lr, wd):
    """The reference's own STFA.update (algorithms.py:183-192) on fixed batches, dropout 0 in the config, from perturbed weights."""
    torch.manual_seed(seed)
    given = dict(cfg)
    algo = get_algorithm_class("STFA")(given, {"learning_rate": lr, "weight_decay": wd}, "cpu")
    assert given["device"] == "cuda:0"                      # the reference writes into the dictionary it is given
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        algo.model.load_state_dict({k: v + torch.empty_like(v).uniform_(-0.1, 0.1, generator=g) for k, v in algo.model.state_dict().items()})
    sd0 = {k: v.detach().numpy().copy() for k, v in algo.model.state_dict().items()}
    xs = np.stack([SO.seeded_input(cfg, bs, seed + 31 * s) for s in range(steps)])
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
    assert np.abs(out["sd20:v.weight"] - sd0["v.weight"]).max() > 0      # zero gradient, yet the weight decay moves it
    # the kink margin, as a condition, at every state the fixture holds together with the batch that meets it: steps 0, 1 and 10
    margins = []
    for s in (0, 1, 10):
        sd_s = {k: out[f"sd{s}:" + k] for k in sd0}
        margins.append(SO.kink_margin(SO.forward_backward(sd_s, xs[s], None, cfg)))
    assert min(margins) > 1.0, ("kink margin", margins)
    out["kink_margin"] = np.asarray(margins, np.float64)
    algo.eval()
    with torch.no_grad():
        out["eval_pred_end"] = algo.model(torch.tensor(xs[0])).numpy().copy()
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print("wrote", name, losses[:3], "...", losses[-1])


def case_trainer_cmapss(name, seed, n_train=250, n_test=80, epochs=3):
    """The reference's OWN harness with --GNN_method STFA on the synthetic C-MAPSS FD001 dataset of synth.py, its own hparams and its own
    shuffling DataLoader; num_epochs patched, the row's dropout set to 0."""
    import argparse
    import tempfile
    import trainer as ref_trainer
    from synth import synthetic_cmapss
    _orig_load = torch.load
    torch.load = lambda *a, **k: _orig_load(*a, **{**k, "weights_only": False})
    (xtr, ytr), (xte, yte) = synthetic_cmapss(seed, n_train, n_test)
    with tempfile.TemporaryDirectory() as tmp:
        d = os.path.join(tmp, "data", "CMAPSS", "FD001")
        os.makedirs(d)
        torch.save({"samples": xtr, "labels": ytr, "max_ruls": 125}, os.path.join(d, "train.pt"))
        torch.save({"samples": xte, "labels": yte, "max_ruls": 125}, os.path.join(d, "test.pt"))
        cwd = os.getcwd()
        os.chdir(tmp)
        try:
            args = argparse.Namespace(save_dir=os.path.join(tmp, "logs"), experiment_description="exp", run_description="r",
                                      GNN_method="STFA", data_path=os.path.join(tmp, "data"), dataset="CMAPSS",
                                      dataset_id="FD001", bearing_id="Testing_bearing_1", num_runs=1, device="cpu")
            tr = ref_trainer.GNN_RUL_trainer(args)
            tr.train_configs["num_epochs"] = epochs
            tr.model_configs["dropout"] = 0.0
            per_epoch = []
            orig = tr.calc_results_per_run

            def spy(run_id):
                per_epoch.append(mg.ref_utils._calc_metrics(tr.pred_labels, tr.true_labels, tr.max_ruls))
                return orig(run_id)
            tr.calc_results_per_run = spy
            start = {}
            ref_get = ref_trainer.get_algorithm_class

            def capturing(method):                           # the model as the harness constructs it, before its first step
                def make(*a, **k):
                    algo = ref_get(method)(*a, **k)
                    start.update({n: v.detach().numpy().copy() for n, v in algo.model.state_dict().items()})
                    return algo
                return make
            ref_trainer.get_algorithm_class = capturing
            tr.train()
            ref_trainer.get_algorithm_class = ref_get
            final = {k: v.detach().numpy().copy() for k, v in tr.algorithm.model.state_dict().items()}
        finally:
            os.chdir(cwd)
            torch.load = _orig_load
    out = {"seed": np.int64(seed), "n_train": np.int64(n_train), "n_test": np.int64(n_test), "epochs": np.int64(epochs),
           "per_epoch": np.asarray(per_epoch, np.float64), "x_train_checksum": np.float64(xtr.astype(np.float64).sum()),
           "batch_size": np.int64(tr.train_configs["batch_size"]), "lr": np.float64(tr.train_configs["learning_rate"])}
    for k in ("gat.attention_0.linear.weight", "gat.attention_9.attention.weight", "v.weight", "lstm.bias_hh_l0", "fc.weight"):
        out["final:" + k] = final[k]
    # the kink margin of the starting point: the constructed model on every window of the run (a graph's kink arguments do not depend on
    # how the windows are batched or shuffled)
    cfg = dict(tr.model_configs)
    cfg.pop("device", None)
    xall = np.concatenate([xtr, xte]).transpose(0, 2, 1)
    margin = SO.kink_margin(SO.forward_backward(start, xall, None, cfg))
    print("      harness start: kink margin", margin)
    out["kink_margin_start"] = np.float64(margin)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print("wrote", name, np.asarray(per_epoch))


def case_hparams(name):
    rows = {}
    for did in ("FD001", "FD002", "FD003", "FD004"):
        hp = get_hparams_class("CMAPSS")(did)
        rows[f"CMAPSS/{did}"] = {"train_params": hp.train_params["STFA"], "alg_hparams": hp.alg_hparams["STFA"]}
    hp = get_hparams_class("NCMAPSS")()
    assert "STFA" not in hp.alg_hparams
    absent = ["NCMAPSS/None"]
    for ds in ("PHM2012", "XJTU_SY"):
        for did in ("Condition_1", "Condition_2", "Condition_3"):
            assert "STFA" not in get_hparams_class(ds)(did).alg_hparams
            absent.append(f"{ds}/{did}")
    np.savez_compressed(os.path.join(HERE, name + ".npz"), rows_json=np.array(json.dumps(rows, sort_keys=True)),
                        absent_json=np.array(json.dumps(absent)))
    print("wrote", name, rows)


if __name__ == "__main__":
    row = dict(patch_size=2, num_patch=25, num_nodes=14, hidden_dim=16, output_dim=5, encoder_hidden_dim=64, num_heads=10, dropout=0.2)
    tiny = dict(row, patch_size=3, num_patch=2, output_dim=2, encoder_hidden_dim=3, num_heads=2)
    odd = dict(row, patch_size=5, num_patch=3, output_dim=3, encoder_hidden_dim=5, num_heads=3)
    case_hparams("stfa_hparams_rows")
    assert get_hparams_class("CMAPSS")("FD001").alg_hparams["STFA"] == row
    case_forward_backward("stfa_small_t2_p3_bs3", tiny, 3, pick_seed(tiny, 3, 61), True)
    case_forward_backward("stfa_small_t3_p5_bs4", odd, 4, pick_seed(odd, 4, 62), True)
    nan_seed = 66
    case_nan("stfa_nan_t3_p5_bs3", odd, nan_seed)
    case_forward_backward("stfa_row_t25_p2_bs2", row, 2, pick_seed(row, 2, 63), False)
    hp = get_hparams_class("CMAPSS")("FD001").train_params["STFA"]
    case_training_curve("stfa_train_curve_t3_p5_bs8", dict(odd, dropout=0.0), 8, 20, 67, hp["learning_rate"], hp["weight_decay"])
    if "--no-trainer" not in sys.argv:
        case_trainer_cmapss("stfa_trainer_fd001_reference_run", 68)
