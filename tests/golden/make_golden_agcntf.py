"""Golden fixtures for the AGCN_TF path, produced by RUNNING THE REFERENCE on the CPU.

    python tests/golden/make_golden_agcntf.py [--trainer]     # needs the reference checkout (read-only import)

Only data is written (inputs, weights, the outputs / gradients the reference produced, each file well under 1 MB); see make_golden.py
for the shims.  Wherever patch_size > 16 the reference runs inside make_golden_sagcn.stable_argsort() -- its `median_freq` comes from
an unstable torch.argsort of an exactly mirrored spectrum; the stable order is the rule this package documents -- and the fixture
records that as `argsort_pinned_stable`.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                                   # noqa: E402  (installs the shims, sets sys.path)
from make_golden_sagcn import signal, stable_argsort       # noqa: E402
from models.AGCN_TF import Model as ref_model              # noqa: E402
from algorithms.algorithms import get_algorithm_class      # noqa: E402
from configs.hparams import get_hparams_class              # noqa: E402


class maybe_pinned:
    def __init__(self, patch_size):
        self.ctx = stable_argsort() if patch_size > 16 else None

    def __enter__(self):
        if self.ctx:
            self.ctx.__enter__()

    def __exit__(self, *exc):
        if self.ctx:
            self.ctx.__exit__(*exc)


def pinned_now():
    return np.bool_(torch.argsort.__name__ == "<lambda>")


def case_forward_backward(name, cfg, bs, seed):
    with maybe_pinned(cfg["patch_size"]):
        torch.manual_seed(seed)
        m = ref_model.AGCN_TF_model(**cfg)
        x = torch.from_numpy(signal(bs, cfg["num_patch"] * cfg["patch_size"], seed + 7))
        y = torch.rand(bs, 1, generator=torch.Generator().manual_seed(seed + 8))
        out = {"x": x.numpy().copy(), "y": y.numpy().copy(), "argsort_pinned_stable": pinned_now(), "seed": np.int64(seed)}
        for k, v in cfg.items():
            out["cfg:" + k] = np.asarray(v, np.int64)
        for k, v in mg.state_np(m, "sd:").items():         # the state dict straight after construction under the seed
            out[k] = v
        t = {}
        hs = [m.temporal_gnn.register_forward_hook(lambda mod, i, o: t.__setitem__("feat", i[0].detach().numpy().copy())),
              m.self_attention.register_forward_hook(lambda mod, i, o: t.update(H=i[0].detach().numpy().copy(),
                                                                                attn_out=o.detach().numpy().copy()))]
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
            out["grad:" + n_] = p.grad.numpy().copy()
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print("wrote", name, out["pred"].ravel()[:3], "loss", out["loss"], "pinned", out["argsort_pinned_stable"],
          os.path.getsize(os.path.join(HERE, name + ".npz")))


def case_training_curve(name, cfg, bs, steps, seed, lr, wd):
    """The reference's own AGCN_TF.update (algorithms.py:589-599) for a few steps on fixed batches."""
    with maybe_pinned(cfg["patch_size"]):
        torch.manual_seed(seed)
        algo = get_algorithm_class("AGCN_TF")(cfg, {"learning_rate": lr, "weight_decay": wd}, "cpu")
        xs = torch.from_numpy(np.stack([signal(bs, cfg["num_patch"] * cfg["patch_size"], seed + 20 + s) for s in range(steps)]))
        ys = torch.rand(steps, bs, 1, generator=torch.Generator().manual_seed(seed + 9))
        out = {"xs": xs.numpy().copy(), "ys": ys.numpy().copy(), "lr": np.float64(lr), "wd": np.float64(wd), "seed": np.int64(seed),
               "argsort_pinned_stable": pinned_now()}
        for k, v in cfg.items():
            out["cfg:" + k] = np.asarray(v, np.int64)
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
    for ds in ("PHM2012", "XJTU_SY"):
        for did in ("Condition_1", "Condition_2", "Condition_3"):
            hp = get_hparams_class(ds)(did)
            rows[f"{ds}/{did}"] = {"train_params": hp.train_params["AGCN_TF"], "alg_hparams": hp.alg_hparams["AGCN_TF"]}
    np.savez_compressed(os.path.join(HERE, name + ".npz"), rows_json=np.array(json.dumps(rows, sort_keys=True)))
    print("wrote", name, rows)


def case_trainer_phm2012(name, seed, n_train=200, n_test=60, epochs=3):
    """The reference's OWN harness with --GNN_method AGCN_TF on the synthetic PHM2012 Condition_1 dataset of synth.py with its own hparams
    (configs/hparams.py:227,243: 40 patches of 64, hidden 100 / 100, batch 100, lr 1e-4, wd 1e-4; no shuffling); num_epochs patched;
    patches of 64 points: the argsort is pinned to the stable order."""
    import argparse
    import tempfile
    import trainer as ref_trainer
    from synth import synthetic_phm2012
    _orig_load = torch.load
    torch.load = lambda *a, **k: _orig_load(*a, **{**k, "weights_only": False})
    (xtr, ytr), (xte, yte) = synthetic_phm2012(seed, n_train, n_test)
    with tempfile.TemporaryDirectory() as tmp, stable_argsort():
        d = os.path.join(tmp, "data", "PHM2012", "Condition_1")
        os.makedirs(d)
        torch.save({"samples": xtr, "labels": ytr, "max_ruls": 1.0}, os.path.join(d, "train.pt"))
        torch.save({"samples": xte, "labels": yte, "max_ruls": 1.0}, os.path.join(d, "test.pt"))
        cwd = os.getcwd()
        os.chdir(tmp)
        try:
            args = argparse.Namespace(save_dir=os.path.join(tmp, "logs"), experiment_description="exp", run_description="r",
                                      GNN_method="AGCN_TF", data_path=os.path.join(tmp, "data"), dataset="PHM2012",
                                      dataset_id="Condition_1", bearing_id="Testing_bearing_1", num_runs=1, device="cpu")
            tr = ref_trainer.GNN_RUL_trainer(args)
            tr.train_configs["num_epochs"] = epochs
            per_epoch = []
            orig = tr.calc_results_per_run

            def spy(run_id):
                per_epoch.append(mg.ref_utils._calc_metrics(tr.pred_labels, tr.true_labels, tr.max_ruls))
                return orig(run_id)
            tr.calc_results_per_run = spy
            tr.train()
            csv_text = open(os.path.join(tmp, "logs", "exp", "r", "AGCN_TF_run_0", "results.csv")).read()
            pinned = pinned_now()
        finally:
            os.chdir(cwd)
            torch.load = _orig_load
    out = {"seed": np.int64(seed), "n_train": np.int64(n_train), "n_test": np.int64(n_test), "epochs": np.int64(epochs),
           "per_epoch": np.asarray(per_epoch, np.float64), "csv_text": np.array(csv_text), "argsort_pinned_stable": pinned,
           "x_train_checksum": np.float64(xtr.astype(np.float64).sum())}
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print("wrote", name, np.asarray(per_epoch))


if __name__ == "__main__":
    case_forward_backward("agcntf_phm_40x64_bs4", dict(num_patch=40, patch_size=64, hidden_adj_dim=100, hidden_gnn_dim=100), 4, 31)
    case_forward_backward("agcntf_small_5x7_bs6", dict(num_patch=5, patch_size=7, hidden_adj_dim=6, hidden_gnn_dim=7, num_heads=2), 6, 32)
    case_forward_backward("agcntf_xjtu_like_20x256_bs3", dict(num_patch=20, patch_size=256, hidden_adj_dim=100, hidden_gnn_dim=100), 3, 33)
    case_training_curve("agcntf_train_curve_12x16_bs8", dict(num_patch=12, patch_size=16, hidden_adj_dim=24, hidden_gnn_dim=20), 8, 12, 5, 1e-3,
                        1e-4)
    case_hparams("agcntf_hparams_rows")
    if "--trainer" in sys.argv:
        case_trainer_phm2012("agcntf_trainer_phm2012_c1_reference_run", 11)
