"""Golden fixtures for the HierCorrPool path, produced by RUNNING THE REFERENCE on the CPU.

    python tests/golden/make_golden_hiercorrpool.py [--trainer]     # needs the reference checkout (read-only import)

Only data is written (inputs, weights, the outputs / gradients / BatchNorm buffers the reference produced, each file under 1 MB); see
make_golden.py for the shims, plus ``torch.Tensor.cuda`` = identity as in make_golden_fcstgnn.py.  The reference's gradients are stored under ``refgrad:``.
Dropout (the reference's ``conv_block1[4]``) is set to 0: its mask comes from torch's generator, which the kernels do not restate.

A fixture is only kept when at least half of its samples have a positive ``fc_1`` pre-activation -- otherwise every gradient is
scaled by the final leaky slope 0.01 and the fixture tests little; the seed is advanced until that holds and recorded.

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
torch.Tensor.cuda = lambda self, *a, **k: self             # dot_graph_construction hard-codes .cuda() (Model_Base.py:18)
from models.HierCorrPool import Model as ref_model         # noqa: E402
from algorithms.algorithms import get_algorithm_class      # noqa: E402
from configs.hparams import get_hparams_class              # noqa: E402


def _run(cfg, bs, seed):
    torch.manual_seed(seed)
    m = ref_model.HierCorrPool_model(**cfg)
    m.Time_Preprocessing.conv_block1[4].p = 0.0
    x = torch.rand(bs, cfg["num_nodes"], cfg["num_patch"] * cfg["patch_size"], generator=torch.Generator().manual_seed(seed + 7))
    y = torch.rand(bs, 1, generator=torch.Generator().manual_seed(seed + 8))
    out = {"x": x.numpy().copy(), "y": y.numpy().copy(), "seed": np.int64(seed)}
    for k, v in cfg.items():
        out["cfg:" + k] = np.asarray(v, np.int64)
    for k, v in mg.state_np(m, "sd:").items():             # the state dict straight after construction under the seed
        out[k] = v
    t = {}
    hs = [m.Time_Preprocessing.register_forward_hook(lambda mod, i, o: t.__setitem__("encoder", o.detach().transpose(1, 2).numpy().copy())),
          m.gc1.Message_Passing.register_forward_hook(lambda mod, i, o: t.update(pooled_x=i[0].detach().numpy().copy(),
                                                                                 pooled_adj=i[1].detach().numpy().copy(),
                                                                                 H=o.detach().numpy().copy())),
          m.fc_1.register_forward_hook(lambda mod, i, o: t.__setitem__("fc1_pre", o.detach().numpy().copy()))]
    m.train()
    pred = m(x)
    for h in hs:
        h.remove()
    loss = torch.nn.functional.mse_loss(pred, y)
    m.zero_grad()
    loss.backward()
    out["pred"], out["loss"] = pred.detach().numpy().copy(), np.float64(loss.item())
    out.update(t)
    for n_, p in m.named_parameters():
        out["refgrad:" + n_] = p.grad.numpy().copy()
    for k, v in m.state_dict().items():                    # the BatchNorm buffers after the one train-mode forward
        if "running_" in k or "num_batches_tracked" in k:
            out["bn_after:" + k] = v.numpy().copy()
    return out


def case_forward_backward(name, cfg, bs, seed):
    while True:
        out = _run(cfg, bs, seed)
        if 2 * int((out["fc1_pre"] > 0).sum()) >= bs:
            break
        seed += 1
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print("wrote", name, "seed", seed, out["pred"].ravel()[:3], "loss", out["loss"], "positive", int((out["fc1_pre"] > 0).sum()), "/", bs,
          os.path.getsize(os.path.join(HERE, name + ".npz")))


def case_training_curve(name, cfg, bs, steps, seed, lr, wd):
    """The reference's own HierCorrPool.update (algorithms.py:95-104) for a few steps on fixed batches, dropout 0."""
    torch.manual_seed(seed)
    algo = get_algorithm_class("HierCorrPool")(cfg, {"learning_rate": lr, "weight_decay": wd}, "cpu")
    algo.model.Time_Preprocessing.conv_block1[4].p = 0.0
    xs = torch.rand(steps, bs, cfg["num_nodes"], cfg["num_patch"] * cfg["patch_size"], generator=torch.Generator().manual_seed(seed + 20))
    ys = torch.rand(steps, bs, 1, generator=torch.Generator().manual_seed(seed + 9))
    out = {"xs": xs.numpy().copy(), "ys": ys.numpy().copy(), "lr": np.float64(lr), "wd": np.float64(wd), "seed": np.int64(seed)}
    for k, v in cfg.items():
        out["cfg:" + k] = np.asarray(v, np.int64)
    for k, v in mg.state_np(algo.model, "sd0:").items():
        out[k] = v
    algo.train()
    losses = [algo.update(xs[s], ys[s], 1)["loss"] for s in range(steps)]
    out["losses"] = np.asarray(losses, dtype=np.float64)
    algo.eval()
    with torch.no_grad():
        out["eval_pred_end"] = algo.model(xs[0]).numpy().copy()
    for k, v in mg.state_np(algo.model, "sd_end:").items():
        out[k] = v
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print("wrote", name, losses[:3], "...", losses[-1], os.path.getsize(os.path.join(HERE, name + ".npz")))


def case_hparams(name):
    rows = {}
    for ds, ids in (("CMAPSS", ("FD001", "FD002", "FD003", "FD004")), ("NCMAPSS", (None,))):
        for did in ids:
            hp = get_hparams_class(ds)(did)
            rows[f"{ds}/{did}"] = {"train_params": hp.train_params["HierCorrPool"], "alg_hparams": hp.alg_hparams["HierCorrPool"]}
    np.savez_compressed(os.path.join(HERE, name + ".npz"), rows_json=np.array(json.dumps(rows, sort_keys=True)))
    print("wrote", name, rows)


def case_trainer_cmapss(name, seed, fd="FD001", n_train=300, n_test=80, epochs=3):
    """The reference's OWN harness with --GNN_method HierCorrPool on the synthetic C-MAPSS dataset of synth.py, its own hparams
    (configs/hparams.py:17,35: FD001 -> 2 patches of 25, kernel 8, batch 100, lr 1e-3, wd 1e-4) and its own shuffling DataLoader.
    num_epochs is patched, and the algorithm class handed to the trainer switches the encoder's dropout off after construction (torch's
    Bernoulli stream cannot be reproduced by any other implementation); nothing in the reference tree is modified."""
    import argparse
    import tempfile
    import trainer as ref_trainer
    from synth import synthetic_cmapss
    _orig_load = torch.load
    torch.load = lambda *a, **k: _orig_load(*a, **{**k, "weights_only": False})
    base = get_algorithm_class("HierCorrPool")

    class NoDropout(base):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.model.Time_Preprocessing.conv_block1[4].p = 0.0
    NoDropout.__name__ = "HierCorrPool"
    _orig_get = ref_trainer.get_algorithm_class
    ref_trainer.get_algorithm_class = lambda n: NoDropout if n == "HierCorrPool" else _orig_get(n)
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
                                      GNN_method="HierCorrPool", data_path=os.path.join(tmp, "data"), dataset="CMAPSS",
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
           "batch_size": np.int64(tr.train_configs["batch_size"]), "lr": np.float64(tr.train_configs["learning_rate"])}
    for k in ("model.fc_1.weight", "model.fc_0.bias", "model.gc1.Graph_Clustering.matrix.weight", "model.gc1.Message_Passing.theta.0.bias",
              "model.Time_Preprocessing.conv_block2.1.weight", "model.Time_Preprocessing.conv_block3.1.running_var",
              "model.Time_Preprocessing.conv_block1.1.num_batches_tracked"):
        out["final:" + k] = final[k]
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print("wrote", name, "per-epoch (Score_v1, Score_v2, MAE, RMSE):\n", np.asarray(per_epoch), os.path.getsize(os.path.join(HERE, name + ".npz")))


def _cfg(p, P, N, h, e, K, M):
    return dict(patch_size=p, num_patch=P, input_dim=10, hidden_dim=h, embedding_dim=e, num_nodes=N, encoder_conv_kernel=K, num_nodes_out=M)


if __name__ == "__main__":
    case_forward_backward("hiercorrpool_small_7x3_n5_bs6", _cfg(3, 7, 5, 2, 2, 12, 3), 6, 41)
    case_forward_backward("hiercorrpool_fd001geom_bs4", _cfg(25, 2, 14, 1, 1, 8, 6), 4, 42)
    case_forward_backward("hiercorrpool_fd004geom_bs4", _cfg(10, 5, 14, 1, 1, 12, 6), 4, 43)
    case_forward_backward("hiercorrpool_ncmapssgeom_bs3", _cfg(1, 50, 20, 1, 1, 32, 6), 3, 44)
    case_training_curve("hiercorrpool_train_curve_7x3_n5_bs8", _cfg(3, 7, 5, 2, 2, 12, 3), 8, 12, 5, 1e-3, 1e-4)
    case_hparams("hiercorrpool_hparams_rows")
    if "--trainer" in sys.argv:
        case_trainer_cmapss("hiercorrpool_trainer_fd001_reference_run", 13)
