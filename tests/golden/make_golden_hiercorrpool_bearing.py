"""Golden fixtures for the HierCorrPool_bearing path, produced by RUNNING THE REFERENCE on the CPU.

    python tests/golden/make_golden_hiercorrpool_bearing.py     # needs the reference checkout (read-only import)

Only data is written; see make_golden.py for the shims and make_golden_hiercorrpool.py / make_golden_logo_bearing.py for the rules kept
here: ``torch.Tensor.cuda`` = identity, the encoder's dropout (``conv_block1[4]``) set to 0 on the constructed model, weights moved away
from init, the seed advanced until at least half of the samples have a positive ``fc_1`` pre-activation, the reference's gradients
under ``refgrad:`` (never ``grad:``).  One more condition on the seed, measured on the reference alone: its fp32 taps and predictions lie
within 1e-6 of ITS OWN fp64 run of the same forward -- the bar tests/test_hiercorrpool_bearing_oracle_golden.py holds the fp64 oracle to
against them; a fixture further from exact than that can be met by no oracle.
The files are named ``hcpb_*`` (tests/test_hiercorrpool_cpu.py counts the ``hiercorrpool_*`` ones) and stay under 1 MiB each.

The spectrogram ``spec`` is what ``torch.stft(...).abs()`` returned inside the reference's forward.

The N = 2 case stores no gradients: with two nodes the off-diagonal softmax makes A the all-ones matrix and S constant for every input,
so several gradients are zero in exact arithmetic and the reference's fp32 run holds only noise there.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                                   # noqa: E402  (installs the shims, sets sys.path)
torch.Tensor.cuda = lambda self, *a, **k: self             # dot_graph_construction hard-codes .cuda()
from models.HierCorrPool_bearing import Model as ref_model  # noqa: E402
from algorithms.algorithms import get_algorithm_class      # noqa: E402
from configs.hparams import get_hparams_class              # noqa: E402

ORACLE_BAR = 1e-6
TAPS = ("encoder", "pooled_x", "pooled_adj", "H")


def _dropout_off(m):
    m.Time_Preprocessing.conv_block1[4].p = 0.0


def _perturb(m, seed):
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for _, p in m.named_parameters():
            p.add_(torch.empty_like(p).uniform_(-0.1, 0.1, generator=g))


def _hooks(m, t, suffix=""):
    return [m.Time_Preprocessing.register_forward_hook(lambda mod, i, o: t.__setitem__("encoder" + suffix, o.detach().transpose(1, 2).numpy().copy())),
            m.gc1.Message_Passing.register_forward_hook(lambda mod, i, o: t.update({"pooled_x" + suffix: i[0].detach().numpy().copy(),
                                                                                    "pooled_adj" + suffix: i[1].detach().numpy().copy(),
                                                                                    "H" + suffix: o.detach().numpy().copy()})),
            m.fc_1.register_forward_hook(lambda mod, i, o: t.__setitem__("fc1_pre" + suffix, o.detach().numpy().copy()))]


def _run(cfg, bs, seed, gradients):
    torch.manual_seed(seed)
    m = ref_model.HierCorrPool_bearing_model(**cfg)
    _dropout_off(m)
    _perturb(m, seed)
    x = torch.randn(bs, cfg["num_patch"] * cfg["patch_size"], generator=torch.Generator().manual_seed(seed + 7))
    y = torch.rand(bs, 1, generator=torch.Generator().manual_seed(seed + 8))
    out = {"x": x.numpy().copy(), "y": y.numpy().copy(), "seed": np.int64(seed)}
    for k, v in cfg.items():
        out["cfg:" + k] = np.asarray(v, np.int64)
    out.update(mg.state_np(m, "sd:"))                      # the perturbed weights and the BatchNorm buffers before the forward
    t = {}
    hs = _hooks(m, t)
    orig_stft = torch.stft

    def spy_stft(*a, **k):
        z = orig_stft(*a, **k)
        t["spec"] = z.abs().detach().reshape(bs, cfg["num_patch"], z.shape[-2], z.shape[-1]).numpy().copy()
        return z
    torch.stft = spy_stft
    try:
        m.train()
        pred = m(x)
    finally:
        torch.stft = orig_stft
    for h in hs:
        h.remove()
    loss = torch.nn.functional.mse_loss(pred, y)
    m.zero_grad()
    loss.backward()
    out["pred"], out["loss"] = pred.detach().numpy().copy(), np.float64(loss.item())
    out.update(t)
    for k, v in m.state_dict().items():                    # the BatchNorm buffers after the one train-mode forward
        if "running_" in k or "num_batches_tracked" in k:
            out["bn_after:" + k] = v.numpy().copy()
    m.eval()
    with torch.no_grad():
        out["pred_eval"] = m(x).numpy().copy()
    if gradients:
        for n_, p in m.named_parameters():
            out["refgrad:" + n_] = p.grad.numpy().copy()
    # the reference's own fp64 run (kept out of the fixture): the eval forward on the buffers as they stand, then the train forward
    torch.set_default_dtype(torch.float64)
    try:
        m.double()
        with torch.no_grad():
            pred_eval64 = m(x.double()).numpy()
            m.train()
            hs = _hooks(m, t, "64")
            pred64 = m(x.double()).numpy()
        for h in hs:
            h.remove()
    finally:
        torch.set_default_dtype(torch.float32)
    rel = lambda a, b: float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())      # noqa: E731
    err = max([rel(out[k], t.pop(k + "64")) for k in TAPS] + [rel(out["pred"], pred64), rel(out["pred_eval"], pred_eval64)])
    return out, err


def case_forward_backward(name, cfg, bs, seed, gradients=True):
    while True:
        out, err = _run(cfg, bs, seed, gradients)
        if 2 * int((out["fc1_pre"] > 0).sum()) >= bs and err < ORACLE_BAR:
            break
        seed += 1
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1 << 20, path
    print("wrote", name, "seed", seed, out["pred"].ravel()[:3], "loss", out["loss"], "positive", int((out["fc1_pre"] > 0).sum()), "/", bs,
          "fp32 error", err, os.path.getsize(path))


def case_training_curve(name, cfg, bs, steps, seed, lr, wd):
    """The reference's own HierCorrPool_bearing.update (algorithms.py:649-658) for a few steps on fixed batches, dropout 0."""
    while True:
        torch.manual_seed(seed)
        algo = get_algorithm_class("HierCorrPool_bearing")(cfg, {"learning_rate": lr, "weight_decay": wd}, "cpu")
        _dropout_off(algo.model)
        _perturb(algo.model, seed)
        xs = torch.randn(steps, bs, cfg["num_patch"] * cfg["patch_size"], generator=torch.Generator().manual_seed(seed + 20))
        ys = torch.rand(steps, bs, 1, generator=torch.Generator().manual_seed(seed + 9))
        out = {"xs": xs.numpy().copy(), "ys": ys.numpy().copy(), "lr": np.float64(lr), "wd": np.float64(wd), "seed": np.int64(seed)}
        for k, v in cfg.items():
            out["cfg:" + k] = np.asarray(v, np.int64)
        out.update(mg.state_np(algo.model, "sd0:"))
        algo.train()
        losses = [algo.update(xs[s], ys[s], 1)["loss"] for s in range(steps)]
        if abs(losses[-1] - losses[0]) > 1e-3 * abs(losses[0]):          # a dead head trains nothing: take another seed
            break
        seed += 1
    out["losses"] = np.asarray(losses, dtype=np.float64)
    algo.eval()
    with torch.no_grad():
        out["eval_pred_end"] = algo.model(xs[0]).numpy().copy()
    out.update(mg.state_np(algo.model, "sd_end:"))
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1 << 20, path
    print("wrote", name, "seed", seed, losses[:3], "...", losses[-1], os.path.getsize(path))


def case_hparams(name):
    rows = {}
    for ds in ("PHM2012", "XJTU_SY"):
        for did in ("Condition_1", "Condition_2", "Condition_3"):
            hp = get_hparams_class(ds)(did)
            rows[f"{ds}/{did}"] = {"train_params": hp.train_params["HierCorrPool_bearing"], "alg_hparams": hp.alg_hparams["HierCorrPool_bearing"]}
    np.savez_compressed(os.path.join(HERE, name + ".npz"), rows_json=np.array(json.dumps(rows, sort_keys=True)))
    print("wrote", name, rows)


def _cfg(p, P, ns, h, e, K, M):
    return dict(patch_size=p, num_patch=P, input_dim=1 + p // ns, hidden_dim=h, embedding_dim=e, num_nodes=ns // 2 + 1, nperseg=ns,
                encoder_conv_kernel=K, num_nodes_out=M)


if __name__ == "__main__":
    case_forward_backward("hcpb_small_ns4_p8_t7_bs6", _cfg(8, 7, 4, 2, 2, 12, 3), 6, 61)
    case_forward_backward("hcpb_ragged_ns4_p10_t3_bs3", _cfg(10, 3, 4, 2, 2, 12, 2), 3, 62)     # patch_size no multiple of nperseg
    case_forward_backward("hcpb_ns2_p6_t3_bs3", _cfg(6, 3, 2, 1, 1, 12, 2), 3, 63, gradients=False)      # N = 2, nperseg = 2
    case_forward_backward("hcpb_p65_ns4_bs2", _cfg(4, 65, 4, 1, 1, 40, 4), 2, 64)               # num_patch past HierCorrPool's 64
    case_training_curve("hcpb_train_curve_ns4_p8_t7_bs8", _cfg(8, 7, 4, 2, 2, 12, 3), 8, 12, 5, 1e-3, 1e-4)
    case_hparams("hcpb_hparams_rows")
