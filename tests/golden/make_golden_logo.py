"""Golden fixtures for the LOGO path, produced by RUNNING THE REFERENCE on the CPU.

    python tests/golden/make_golden_logo.py [--trainer]     # needs the reference checkout (read-only import)

Only data is written (inputs, weights, the outputs / taps / gradients the reference produced, each file far under 1 MB; hidden widths
reduced); see make_golden.py for the shims, plus ``torch.Tensor.cuda`` = identity as in make_golden_hiercorrpool.py.  The reference's
gradients are stored under ``refgrad:``.  The two dropouts (``TD.drop2``, ``TD.drop3``) are set to 0 on the constructed model: their
masks come from torch's generator, which the kernels do not restate.  Weights are moved away from init (SURVEY.md section 4 hazard 5).

A forward fixture is only kept when at least half of its samples reach the prediction through an open ReLU of fc1 and of fc2 --
otherwise most gradients are exact zeros and the fixture tests little; the seed is advanced until that holds and recorded.

With ``--trainer`` also the reference's own harness for three epochs on synth.py's synthetic C-MAPSS (FD001 wiring), with the same
dropout switch on the constructed model.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                                   # noqa: E402  (installs the shims, sets sys.path)
torch.Tensor.cuda = lambda self, *a, **k: self             # dot_graph_construction hard-codes .cuda() (models/LOGO/Model.py:48,186)
from models.LOGO import Model as ref_model                 # noqa: E402
from algorithms.algorithms import get_algorithm_class      # noqa: E402
from configs.hparams import get_hparams_class              # noqa: E402

THETA = 0.01


def _dropouts_off(m):
    m.TD.drop2.p = 0.0
    m.TD.drop3.p = 0.0


def _perturbed(cfg, seed):
    torch.manual_seed(seed)
    m = ref_model.LOGO_model(**cfg)
    _dropouts_off(m)
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for _, p in m.named_parameters():
            p.add_(torch.empty_like(p).uniform_(-0.1, 0.1, generator=g))
    return m


def _run(cfg, bs, seed):
    m = _perturbed(cfg, seed)
    x = torch.rand(bs, cfg["num_nodes"], cfg["num_patch"] * cfg["patch_size"], generator=torch.Generator().manual_seed(seed + 7))
    y = torch.rand(bs, 1, generator=torch.Generator().manual_seed(seed + 8))
    out = {"x": x.numpy().copy(), "y": y.numpy().copy(), "seed": np.int64(seed), "theta": np.float64(THETA)}
    for k, v in cfg.items():
        out["cfg:" + k] = np.asarray(v, np.int64)
    for k, v in mg.state_np(m, "sd:").items():
        out[k] = v
    Q = cfg["num_patch"] * cfg["num_nodes"]
    t = {}
    hs = [m.MPNN.register_forward_hook(lambda mod, i, o: t.__setitem__("mpnn", o.detach().reshape(bs, Q, -1).transpose(0, 1).numpy().copy())),
          m.TD.register_forward_hook(lambda mod, i, o: t.__setitem__("lstm", o.detach().numpy().copy())),
          m.fc.fc1.register_forward_hook(lambda mod, i, o: t.__setitem__("fc1_pre", o.detach().numpy().copy())),
          m.fc.fc2.register_forward_hook(lambda mod, i, o: t.__setitem__("fc2_pre", o.detach().numpy().copy()))]
    m.train()
    pred, gl = m(x, GL=True)
    for h in hs:
        h.remove()
    loss = torch.nn.functional.mse_loss(pred, y) + THETA * gl
    m.zero_grad()
    loss.backward()
    out["pred"], out["loss_gl"], out["loss"] = pred.detach().numpy().copy(), np.float64(gl.item()), np.float64(loss.item())
    out.update(t)
    for n_, p in m.named_parameters():
        out["refgrad:" + n_] = p.grad.numpy().copy()
    m.eval()
    with torch.no_grad():
        out["pred_eval"] = m(x).numpy().copy()
    return out


def _open(out):
    return int(((out["fc1_pre"] > 0).any(1) & (out["fc2_pre"] > 0).any(1)).sum())


def case_forward_backward(name, cfg, bs, seed):
    while True:
        out = _run(cfg, bs, seed)
        if 2 * _open(out) >= bs:
            break
        seed += 1
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print("wrote", name, "seed", seed, out["pred"].ravel()[:3], "loss", out["loss"], "gl", out["loss_gl"], "open", _open(out), "/", bs,
          os.path.getsize(os.path.join(HERE, name + ".npz")))


def case_training_curve(name, cfg, bs, steps, seed, lr, wd):
    """The reference's own LOGO.update (algorithms.py:125-136) for a few steps on fixed batches, dropouts 0, theta 0.01."""
    while True:
        torch.manual_seed(seed)
        algo = get_algorithm_class("LOGO")(cfg, {"learning_rate": lr, "weight_decay": wd, "theta": THETA}, "cpu")
        _dropouts_off(algo.model)
        g = torch.Generator().manual_seed(seed + 1000)
        with torch.no_grad():
            for _, p in algo.model.named_parameters():
                p.add_(torch.empty_like(p).uniform_(-0.1, 0.1, generator=g))
        xs = torch.rand(steps, bs, cfg["num_nodes"], cfg["num_patch"] * cfg["patch_size"], generator=torch.Generator().manual_seed(seed + 20))
        ys = torch.rand(steps, bs, 1, generator=torch.Generator().manual_seed(seed + 9))
        out = {"xs": xs.numpy().copy(), "ys": ys.numpy().copy(), "lr": np.float64(lr), "wd": np.float64(wd), "seed": np.int64(seed),
               "theta": np.float64(THETA)}
        for k, v in cfg.items():
            out["cfg:" + k] = np.asarray(v, np.int64)
        for k, v in mg.state_np(algo.model, "sd0:").items():
            out[k] = v
        algo.train()
        losses = [algo.update(xs[s], ys[s], 1)["loss"] for s in range(steps)]
        if abs(losses[-1] - losses[0]) > 1e-3 * abs(losses[0]):          # a dead head trains nothing: take another seed
            break
        seed += 1
    out["losses"] = np.asarray(losses, dtype=np.float64)
    algo.eval()
    with torch.no_grad():
        out["eval_pred_end"] = algo.model(xs[0]).numpy().copy()
    for k, v in mg.state_np(algo.model, "sd_end:").items():
        out[k] = v
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print("wrote", name, "seed", seed, losses[:3], "...", losses[-1], os.path.getsize(os.path.join(HERE, name + ".npz")))


def case_hparams(name):
    rows = {}
    for ds, ids in (("CMAPSS", ("FD001", "FD002", "FD003", "FD004")), ("NCMAPSS", (None,))):
        for did in ids:
            hp = get_hparams_class(ds)(did)
            rows[f"{ds}/{did}"] = {"train_params": hp.train_params["LOGO"], "alg_hparams": hp.alg_hparams["LOGO"]}
    np.savez_compressed(os.path.join(HERE, name + ".npz"), rows_json=np.array(json.dumps(rows, sort_keys=True)))
    print("wrote", name, rows)


def case_trainer_cmapss(name, seed, fd="FD001", n_train=300, n_test=80, epochs=3):
    """The reference's OWN harness with --GNN_method LOGO on the synthetic C-MAPSS dataset of synth.py, its own hparams
    (configs/hparams.py:18,37: FD001 -> 5 patches of 10, hidden 8, batch 100, lr 1e-3, wd 1e-4, theta 0.001) and its own shuffling
    DataLoader.  num_epochs is patched, and the algorithm class handed to the trainer switches the two dropouts off after construction
    (torch's Bernoulli stream cannot be reproduced by any other implementation); nothing in the reference tree is modified."""
    import argparse
    import tempfile
    import trainer as ref_trainer
    from synth import synthetic_cmapss
    _orig_load = torch.load
    torch.load = lambda *a, **k: _orig_load(*a, **{**k, "weights_only": False})
    base = get_algorithm_class("LOGO")

    class NoDropout(base):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            _dropouts_off(self.model)
    NoDropout.__name__ = "LOGO"
    _orig_get = ref_trainer.get_algorithm_class
    ref_trainer.get_algorithm_class = lambda n: NoDropout if n == "LOGO" else _orig_get(n)
    (xtr, ytr), (xte, yte) = synthetic_cmapss(seed, n_train, n_test)
    with tempfile.TemporaryDirectory() as tmp:
        d = os.path.join(tmp, "data", "CMAPSS", fd)
        os.makedirs(d)
        torch.save({"samples": xtr, "labels": ytr, "max_ruls": 125}, os.path.join(d, "train.pt"))
        torch.save({"samples": xte, "labels": yte, "max_ruls": 125}, os.path.join(d, "test.pt"))
        cwd = os.getcwd()
        os.chdir(tmp)
        try:
            args = argparse.Namespace(save_dir=os.path.join(tmp, "logs"), experiment_description="exp", run_description="r",
                                      GNN_method="LOGO", data_path=os.path.join(tmp, "data"), dataset="CMAPSS",
                                      dataset_id=fd, bearing_id=None, num_runs=1, device="cpu")
            tr = ref_trainer.GNN_RUL_trainer(args)
            tr.train_configs["num_epochs"] = epochs
            per_epoch = []
            orig = tr.calc_results_per_run

            def spy(run_id):
                per_epoch.append(mg.ref_utils._calc_metrics(tr.pred_labels, tr.true_labels, tr.max_ruls))
                return orig(run_id)
            tr.calc_results_per_run = spy
            tr.train()
            final = {k: v.detach().numpy().copy() for k, v in tr.algorithm.state_dict().items()}
        finally:
            os.chdir(cwd)
            torch.load = _orig_load
            ref_trainer.get_algorithm_class = _orig_get
    out = {"seed": np.int64(seed), "n_train": np.int64(n_train), "n_test": np.int64(n_test), "epochs": np.int64(epochs), "fd": np.array(fd),
           "per_epoch": np.asarray(per_epoch, np.float64), "x_train_checksum": np.float64(xtr.astype(np.float64).sum()),
           "batch_size": np.int64(tr.train_configs["batch_size"]), "lr": np.float64(tr.train_configs["learning_rate"]),
           "theta": np.float64(tr.train_configs["theta"])}
    for k in ("model.cls.weight", "model.fc.fc2.weight", "model.fc.fc1.bias", "model.graph_attn_blk.W_h.weight", "model.graph_attn_blk.W_Z_G.bias",
              "model.MPNN.theta.0.weight", "model.nonlin_map.weight", "model.TD.bi_lstm2.weight_hh_l0_reverse", "model.TD.bi_lstm1.bias_ih_l0"):
        out["final:" + k] = final[k]
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print("wrote", name, "per-epoch (Score_v1, Score_v2, MAE, RMSE):\n", np.asarray(per_epoch), os.path.getsize(os.path.join(HERE, name + ".npz")))


def _cfg(p, T, N, h):
    return dict(patch_size=p, num_patch=T, num_nodes=N, hidden_dim=h)


if __name__ == "__main__":
    case_forward_backward("logo_small_3x2x2_h1_bs4", _cfg(2, 2, 3, 1), 4, 41)
    case_forward_backward("logo_fd001geom_bs5", _cfg(10, 5, 14, 2), 5, 42)
    case_forward_backward("logo_fd002geom_bs4", _cfg(2, 25, 14, 2), 4, 43)
    case_forward_backward("logo_ncmapssgeom_bs3", _cfg(5, 10, 20, 2), 3, 44)
    case_training_curve("logo_train_curve_3x2x2_h1_bs8", _cfg(2, 2, 3, 1), 8, 12, 5, 1e-3, 1e-4)
    case_hparams("logo_hparams_rows")
    if "--trainer" in sys.argv:
        case_trainer_cmapss("logo_trainer_fd001_reference_run", 13)
