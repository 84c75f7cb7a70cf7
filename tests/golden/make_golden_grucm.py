"""Golden fixtures for the GRU_CM path, produced by RUNNING THE REFERENCE on the CPU.

    python tests/golden/make_golden_grucm.py     # needs /root/reference (read-only import)

Only data is written (inputs, weights, the outputs / gradients the reference produced, its hparams rows); see make_golden.py for the
shims.  Shapes: the reference's C-MAPSS wiring (configs/hparams.py:46: 14 nodes x 50 steps, GRU hidden 64), its N-CMAPSS wiring
(:210: 20 nodes) and one odd shape (9 nodes x 21 steps).  The reference's nn.Dropout draws from torch's Bernoulli stream, which no other
implementation reproduces: the train-mode cases set the three rates to 0.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                                   # noqa: E402  (installs the shims, sets sys.path)
from models.GRU_CM import Model as ref_model               # noqa: E402
from algorithms.algorithms import get_algorithm_class      # noqa: E402
from configs.hparams import get_hparams_class              # noqa: E402


def no_dropout(m):
    for d in (m.dropout1, m.dropout2, m.dropout3):
        d.p = 0.0


def case_forward_backward(name, cfg, bs, seed, lo=0.0, hi=1.0):
    """State dict straight after construction under torch.manual_seed(seed) (pins the initialisation order too), eval prediction,
    and the train-mode prediction / loss / gradients with p = 0."""
    torch.manual_seed(seed)
    m = ref_model.GRU_CM_model(**cfg)
    g = torch.Generator().manual_seed(seed + 7)
    x = torch.rand(bs, cfg["num_nodes"], cfg["time_length"], generator=g) * (hi - lo) + lo
    y = torch.rand(bs, 1, generator=g)
    out = {"x": x.numpy().copy(), "y": y.numpy().copy(), "seed": np.int64(seed)}
    for k, v in cfg.items():
        out["cfg:" + k] = np.int64(v)
    for k, v in mg.state_np(m, "sd:").items():
        out[k] = v
    m.eval()
    with torch.no_grad():
        out["eval_pred"] = m(x).numpy().copy()
    m.train()
    no_dropout(m)
    pred = m(x)
    loss = torch.nn.functional.mse_loss(pred, y)
    m.zero_grad()
    loss.backward()
    out["pred"] = pred.detach().numpy().copy()
    out["loss"] = np.float64(loss.item())
    for n_, p in m.named_parameters():
        out["grad:" + n_] = p.grad.numpy().copy()
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print("wrote", name, out["pred"].ravel()[:3], "loss", out["loss"])


def case_training_curve(name, cfg, bs, steps, seed, lr, wd):
    """The reference's own GRU_CM.update (algorithms.py:371-380) for a few steps on fixed batches, p = 0."""
    torch.manual_seed(seed)
    algo = get_algorithm_class("GRU_CM")(cfg, {"learning_rate": lr, "weight_decay": wd}, "cpu")
    no_dropout(algo.model)
    g = torch.Generator().manual_seed(seed + 7)
    xs = torch.rand(steps, bs, cfg["num_nodes"], cfg["time_length"], generator=g)
    ys = torch.rand(steps, bs, 1, generator=g)
    out = {"xs": xs.numpy().copy(), "ys": ys.numpy().copy(), "lr": np.float64(lr), "wd": np.float64(wd), "seed": np.int64(seed)}
    for k, v in cfg.items():
        out["cfg:" + k] = np.int64(v)
    for k, v in mg.state_np(algo, "sd0:").items():
        out[k] = v
    algo.train()
    losses = [algo.update(xs[s], ys[s], 1)["loss"] for s in range(steps)]
    out["losses"] = np.asarray(losses, dtype=np.float64)
    algo.eval()
    with torch.no_grad():
        out["eval_pred_end"] = algo.model(xs[0]).numpy().copy()
    for k, v in mg.state_np(algo, "sd_end:").items():
        out[k] = v
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print("wrote", name, losses[:3], "...", losses[-1])


def case_hparams(name):
    rows = {}
    for ds, ids in (("CMAPSS", ["FD001", "FD002", "FD003", "FD004"]), ("NCMAPSS", [None])):
        for did in ids:
            hp = get_hparams_class(ds)(did) if did is not None else get_hparams_class(ds)()
            rows[f"{ds}/{did}"] = {"train_params": hp.train_params["GRU_CM"], "alg_hparams": hp.alg_hparams["GRU_CM"]}
    np.savez_compressed(os.path.join(HERE, name + ".npz"), rows_json=np.array(json.dumps(rows, sort_keys=True)))
    print("wrote", name, rows)


if __name__ == "__main__":
    cmapss = dict(time_length=50, num_nodes=14, gru_hidden_dim=64)
    ncmapss = dict(time_length=50, num_nodes=20, gru_hidden_dim=64)
    odd = dict(time_length=21, num_nodes=9, gru_hidden_dim=64)
    case_forward_backward("grucm_cmapss_14x50_bs8", cmapss, 8, 21)
    case_forward_backward("grucm_ncmapss_20x50_bs5", ncmapss, 5, 22, lo=-1.0, hi=1.0)
    case_forward_backward("grucm_odd_9x21_bs6", odd, 6, 23)
    hp = get_hparams_class("CMAPSS")("FD004").train_params["GRU_CM"]
    case_training_curve("grucm_train_curve_14x50_bs16", cmapss, 16, 12, 3, hp["learning_rate"], hp["weight_decay"])
    case_hparams("grucm_hparams_rows")
