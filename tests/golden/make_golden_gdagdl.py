"""Golden fixtures for the GDAGDL path, produced by RUNNING THE REFERENCE on the CPU.

    python tests/golden/make_golden_gdagdl.py     # needs /root/reference (read-only import)

Only data is written (inputs, weights, the outputs / gradients the reference produced, its hparams rows); see make_golden.py for the
shims.  Weights are the constructor's under torch.manual_seed(seed), moved away from init by uniform(-0.1, 0.1) from
torch.Generator().manual_seed(seed + 1000) in state_dict order.  The reference's F.dropout draws from torch's Bernoulli stream, which no
other implementation reproduces: the train-mode cases set the layers' ``dropout`` attribute to 0 on the constructed instance.

Inputs.  Every patch is ``amp * randn + dc`` with amp log-uniform in [0.03, 3] and dc normal(0, amp): the mix of scales is what makes
the node-importance sign differ between nodes and graphs.  The maker asserts, and keeps drawing patches until they hold:

  * mask margin: on every graph without a NaN, |ni_i| >= 1e-3 * sum_j |pcc_ij| |lin_j| (the absolute-sum scale of its own dot product),
    which puts every sign decision three orders above fp32 rounding -- decided on the fp64 oracle's restatement of the front end, then
  * mask agreement: the reference's fp32 mask equals the fp64 oracle's on every node (asserted on the reference's run), and
  * graph kinds: every small / full fixture holds a graph with all nodes live (graph 0), with exactly one node live (graph 1), with
    some but not all live (graph 2) and one all-zero patch (graph 3): the NaN graph, whose ni is stored as NaN.

The small cases hold everything; the full-geometry cases (230 k - 596 k weights) hold the seed and a checksum of the weights instead --
the tests rebuild the weights from the seed, assert the checksum and take the gradients from the fp64 oracle.  Gradients are stored
under ``refgrad:`` keys (tests/grad_cases.py globs for ``grad:``).
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
from models.GDAGDL import Model as ref_model               # noqa: E402
from algorithms.algorithms import get_algorithm_class      # noqa: E402
from configs.hparams import get_hparams_class              # noqa: E402
import gdagdl_oracle as GO                                 # noqa: E402

MARGIN = GO.MASK_MARGIN


def seeded_model(cfg, seed):
    torch.manual_seed(seed)
    m = ref_model.GDAGDL_model(**cfg)
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        m.load_state_dict({k: v + torch.empty_like(v).uniform_(-0.1, 0.1, generator=g) for k, v in m.state_dict().items()})
    return m


def dropout_off(m):
    for layer in m.gat_layers:
        layer.dropout = 0.0


classify, draw_inputs = GO.classify_patches, GO.draw_inputs


def run_with_taps(m, x):
    taps = {}
    hs = [m.node_importance_linear.register_forward_hook(lambda mod, a, out: taps.update(lin=out.detach())),
          m.gat_layers[0].register_forward_pre_hook(lambda mod, a: taps.update(mag=a[0].detach().numpy().copy(),
                                                                                   adj=a[1].detach().numpy().copy())),
          m.encoder.register_forward_hook(lambda mod, a, out: taps.update(yo=a[0].detach().numpy().copy(), H=out.detach().numpy().copy()))]
    pred, recon = m(x, train=True)
    for h in hs:
        h.remove()
    bs, T = x.shape[0], m.num_patch
    mag = torch.tensor(taps["mag"])
    ni = (ref_model.pcc_graph_construction(mag.reshape(bs, T, *mag.shape[1:])).reshape(bs * T, mag.shape[1], mag.shape[1])
          @ taps.pop("lin").reshape(bs * T, -1, 1)).reshape(bs, T, -1)
    taps["ni"] = ni.numpy().copy()
    taps["mask"] = (ni > 0).float().numpy().copy()
    assert np.array_equal(taps.pop("adj"), (taps["mask"][..., :, None] * taps["mask"][..., None, :]).reshape(bs * T, mag.shape[1], -1))
    taps["mag"] = taps["mag"].reshape(bs, T, *mag.shape[1:])
    return pred, recon, taps


def cfg_entries(cfg):
    return {"cfg_json": np.array(json.dumps(cfg, sort_keys=True))}


def case_forward_backward(name, cfg, bs, seed, full):
    m = seeded_model(cfg, seed)
    sd = {k: v.detach().numpy() for k, v in m.state_dict().items()}
    x_np = draw_inputs(cfg, bs, seed, sd["node_importance_linear.weight"].astype(np.float64), sd["node_importance_linear.bias"].astype(np.float64))
    x = torch.tensor(x_np)
    y = torch.rand(bs, 1, generator=torch.Generator().manual_seed(seed + 8))
    out = {"x": x_np, "y": y.numpy().copy(), "seed": np.int64(seed), "margin": np.float64(MARGIN), **cfg_entries(cfg)}
    flat = np.concatenate([v.astype(np.float64).ravel() for v in sd.values()])
    out["checksum"] = np.array([flat.sum(), (flat * flat).sum()], np.float64)
    m.eval()
    with torch.no_grad():
        out["pred_eval"] = m(x).numpy().copy()
    m.train()
    dropout_off(m)
    pred, recon, taps = run_with_taps(m, x)
    mse = torch.nn.functional.mse_loss(pred, y)
    m.zero_grad()
    (mse + recon).backward()
    # mask agreement with the fp64 oracle, graph kinds
    o = GO.forward_backward({k: v for k, v in sd.items()}, x_np, y.numpy(), cfg, want_grads=False)
    assert np.array_equal(o["mask"], taps["mask"]), "fp32 reference mask differs from the fp64 oracle's"
    assert np.array_equal(np.isnan(o["ni"]), np.isnan(taps["ni"]))
    live = taps["mask"].reshape(-1, cfg["num_nodes"]).sum(-1)
    N = cfg["num_nodes"]
    assert live[0] == N and live[1] == 1 and 1 < live[2] < N, live[:4]
    assert live[3] == 0 and np.isnan(taps["ni"].reshape(-1, N)[3]).all() and not np.isnan(taps["ni"].reshape(-1, N)[:3]).any()
    assert np.isfinite(pred.detach().numpy()).all()
    out["graph_kinds"] = np.array([0, 1, 2, 3], np.int64)              # graphs holding: all live, one live, some live, the zero patch
    out["pred"] = pred.detach().numpy().copy()
    out["mse"], out["recon"] = np.float64(mse.item()), np.float64(recon.item())
    out["loss"] = np.float64((mse + recon).item())
    for k in ("ni", "mask") + (("mag", "yo", "H") if full else ()):
        out["tap:" + k] = taps[k]
    if full:
        for k, v in mg.state_np(m, "sd:").items():
            out[k] = v
        for n_, p in m.named_parameters():
            assert (p.grad is None) == (n_ in GO.GRADLESS), n_
            if p.grad is not None:
                out["refgrad:" + n_] = p.grad.numpy().copy()
    else:                                                   # a sample of the reference's gradients: the small tensors
        for n_, p in m.named_parameters():
            if p.grad is not None and p.numel() <= 1200:
                out["refgrad:" + n_] = p.grad.numpy().copy()
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1 << 20
    print("wrote", name, out["pred"].ravel()[:3], "loss", out["loss"], "live", live[:6], os.path.getsize(path), "bytes")


def case_training_curve(name, cfg, bs, steps, seed, lr, wd):
    """The reference's own GDAGDL.update (algorithms.py:535-544) on fixed batches, dropout off.  node_importance_linear never moves, so
    the masks of every batch are fixed for the run: each batch holds the mask margin and agrees with the fp64 oracle."""
    torch.manual_seed(seed)
    algo = get_algorithm_class("GDAGDL")(cfg, {"learning_rate": lr, "weight_decay": wd}, "cpu")
    dropout_off(algo.model)
    sd0 = {k: v.detach().numpy().copy() for k, v in algo.model.state_dict().items()}
    w, b = sd0["node_importance_linear.weight"].astype(np.float64), sd0["node_importance_linear.bias"].astype(np.float64)
    xs = np.stack([draw_inputs(cfg, bs, seed + 31 * s, w, b, planted=False) for s in range(steps)])
    ys = torch.rand(steps, bs, 1, generator=torch.Generator().manual_seed(seed + 8))
    for s in range(steps):
        _, _, taps = run_with_taps(algo.model, torch.tensor(xs[s]))
        o = GO.forward_backward(sd0, xs[s], None, cfg)
        assert np.array_equal(o["mask"], taps["mask"])
    out = {"xs": xs, "ys": ys.numpy().copy(), "lr": np.float64(lr), "wd": np.float64(wd), "seed": np.int64(seed), **cfg_entries(cfg)}
    for k, v in sd0.items():
        out["sd0:" + k] = v
    algo.train()
    losses = [algo.update(torch.tensor(xs[s]), ys[s], 1)["loss"] for s in range(steps)]
    out["losses"] = np.asarray(losses, dtype=np.float64)
    algo.eval()
    with torch.no_grad():
        out["eval_pred_end"] = algo.model(torch.tensor(xs[0])).numpy().copy()
    end = algo.model.state_dict()
    assert all(np.array_equal(end[k].numpy(), sd0[k]) for k in GO.GRADLESS)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print("wrote", name, losses[:3], "...", losses[-1])


def case_trainer_phm2012(name, seed, n_train=200, n_test=60, epochs=3):
    """The reference's OWN harness with --GNN_method GDAGDL on the synthetic PHM2012 Condition_1 dataset of synth.py with its own hparams
    (128 patches of 20 points, batch 100, lr 1e-3, wd 1e-4; no shuffling); num_epochs patched, the layers' ``dropout`` attribute set to 0
    on the constructed model."""
    import argparse
    import tempfile
    import trainer as ref_trainer
    from synth import synthetic_phm2012
    _orig_load = torch.load
    torch.load = lambda *a, **k: _orig_load(*a, **{**k, "weights_only": False})
    (xtr, ytr), (xte, yte) = synthetic_phm2012(seed, n_train, n_test)
    orig_init = ref_model.GDAGDL_model.__init__

    def init_without_dropout(self, *a, **k):
        orig_init(self, *a, **k)
        dropout_off(self)
    ref_model.GDAGDL_model.__init__ = init_without_dropout
    with tempfile.TemporaryDirectory() as tmp:
        d = os.path.join(tmp, "data", "PHM2012", "Condition_1")
        os.makedirs(d)
        torch.save({"samples": xtr, "labels": ytr, "max_ruls": 1.0}, os.path.join(d, "train.pt"))
        torch.save({"samples": xte, "labels": yte, "max_ruls": 1.0}, os.path.join(d, "test.pt"))
        cwd = os.getcwd()
        os.chdir(tmp)
        try:
            args = argparse.Namespace(save_dir=os.path.join(tmp, "logs"), experiment_description="exp", run_description="r",
                                      GNN_method="GDAGDL", data_path=os.path.join(tmp, "data"), dataset="PHM2012",
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
            final = {k: v.detach().numpy().copy() for k, v in tr.algorithm.model.state_dict().items()}
        finally:
            os.chdir(cwd)
            torch.load = _orig_load
            ref_model.GDAGDL_model.__init__ = orig_init
    out = {"seed": np.int64(seed), "n_train": np.int64(n_train), "n_test": np.int64(n_test), "epochs": np.int64(epochs),
           "per_epoch": np.asarray(per_epoch, np.float64), "x_train_checksum": np.float64(xtr.astype(np.float64).sum()),
           "batch_size": np.int64(tr.train_configs["batch_size"]), "lr": np.float64(tr.train_configs["learning_rate"])}
    for k in ("gat_layers.0.linear.bias", "gat_layers.2.attention.weight", "node_importance_linear.weight", "encoder.6.bias", "linear.weight"):
        out["final:" + k] = final[k]                        # (the whole state would be 0.9 MB)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print("wrote", name, np.asarray(per_epoch))


def case_hparams(name):
    rows = {}
    for ds in ("PHM2012", "XJTU_SY"):
        for did in ("Condition_1", "Condition_2", "Condition_3"):
            hp = get_hparams_class(ds)(did)
            rows[f"{ds}/{did}"] = {"train_params": hp.train_params["GDAGDL"], "alg_hparams": hp.alg_hparams["GDAGDL"]}
    absent = []
    for ds, ids in (("CMAPSS", ["FD001", "FD002", "FD003", "FD004"]), ("NCMAPSS", [None])):
        for did in ids:
            hp = get_hparams_class(ds)(did) if did is not None else get_hparams_class(ds)()
            assert "GDAGDL" not in hp.alg_hparams
            absent.append(f"{ds}/{did}")
    np.savez_compressed(os.path.join(HERE, name + ".npz"), rows_json=np.array(json.dumps(rows, sort_keys=True)),
                        absent_json=np.array(json.dumps(absent)))
    print("wrote", name, rows)


if __name__ == "__main__":
    base = dict(gat_layer_dim=[300, 150, 50], lstm_hidden_dim=20, autoencoder_hidden_dim=256, autoencoder_out_dim=50)
    small = dict(num_patch=3, patch_size=8, num_nodes=3, nperseg=4, input_dim=3, gat_layer_dim=[5, 4, 3], lstm_hidden_dim=3,
                 autoencoder_hidden_dim=8, autoencoder_out_dim=4)
    odd = dict(num_patch=2, patch_size=32, num_nodes=5, nperseg=8, input_dim=5, gat_layer_dim=[7, 6, 5], lstm_hidden_dim=3,
               autoencoder_hidden_dim=8, autoencoder_out_dim=4)
    case_forward_backward("gdagdl_small_n3_t3_bs4", small, 4, 41, True)
    case_forward_backward("gdagdl_small_n5_t2_bs3", odd, 3, 42, True)
    case_forward_backward("gdagdl_phmc1geom_bs2", dict(base, num_patch=128, patch_size=20, num_nodes=3, nperseg=4, input_dim=6), 2, 43, False)
    case_forward_backward("gdagdl_phmc3geom_bs2", dict(base, num_patch=80, patch_size=32, num_nodes=5, nperseg=8, input_dim=5), 2, 44, False)
    case_forward_backward("gdagdl_xjtugeom_bs2", dict(base, num_patch=32, patch_size=1024, num_nodes=17, nperseg=32, input_dim=33), 2, 45, False)
    hp = get_hparams_class("PHM2012")("Condition_1").train_params["GDAGDL"]
    case_training_curve("gdagdl_train_curve_n5_t2_bs8", odd, 8, 20, 46, hp["learning_rate"], hp["weight_decay"])
    case_hparams("gdagdl_hparams_rows")
    if "--no-trainer" not in sys.argv:
        case_trainer_phm2012("gdagdl_trainer_phm2012_c1_reference_run", 47)
