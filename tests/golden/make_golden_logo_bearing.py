"""Golden fixtures for the LOGO_bearing path, produced by RUNNING THE REFERENCE on the CPU.

    python tests/golden/make_golden_logo_bearing.py     # needs the reference checkout (read-only import)

Only data is written; see make_golden.py for the shims and make_golden_logo.py for the rules kept here: ``torch.Tensor.cuda`` = identity,
the two dropouts (``TD.drop2``, ``TD.drop3``) set to 0 on the constructed model, weights moved away from init, the seed advanced until
at least half of the samples reach the prediction through an open ReLU of fc1 and of fc2, the reference's gradients under ``refgrad:``.
One more condition on the seed, measured on the reference alone: its fp32 taps, predictions and L_GL lie within 1e-6 of ITS OWN fp64 run
of the same forward.  A fixture whose fp32 values are further from exact than the bar an fp64 oracle is held to against them (1e-6, LOGO's)
cannot be met by any oracle; fc1 sums 16 320 products at XJTU_SY, and there one seed in a few lands at 1.05e-6.
The files are named ``logob_*`` (tests/test_logo_cpu.py counts the ``logo_*`` ones).

Every file stays under 1 MiB.  The two full-width cases (the reference's PHM2012 and XJTU_SY rows, whose fc1 alone is 1 MB at XJTU_SY)
store no weights -- the tests rebuild them from the recorded seed, which tests/test_logo_bearing_cpu.py holds to the reference's
initial values on the small cases -- and their arrays are spread over ``<name>.npz``, ``<name>.p1.npz``, ...

The spectrogram ``spec`` is what ``torch.stft(...).abs()`` returned inside the reference's forward.
"""
import glob
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                                   # noqa: E402  (installs the shims, sets sys.path)
torch.Tensor.cuda = lambda self, *a, **k: self             # dot_graph_construction hard-codes .cuda()
from models.LOGO_bearing import Model as ref_model         # noqa: E402
from algorithms.algorithms import get_algorithm_class      # noqa: E402
from configs.hparams import get_hparams_class              # noqa: E402

THETA = 0.01
PART_BYTES = 900 * 1024
ORACLE_BAR = 1e-6           # tests/test_logo_oracle_golden.py holds the fp64 oracle to this against the reference's fp32 outputs
KEYS = "patch_size num_patch input_dim num_nodes nperseg hidden_dim".split()


def _dropouts_off(m):
    m.TD.drop2.p = 0.0
    m.TD.drop3.p = 0.0


def _perturb(m, seed):
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for _, p in m.named_parameters():
            p.add_(torch.empty_like(p).uniform_(-0.1, 0.1, generator=g))


def _save_parts(name, out):
    """Greedy packing in insertion order: a part is closed before it would pass PART_BYTES."""
    for old in glob.glob(os.path.join(HERE, name + ".npz")) + glob.glob(os.path.join(HERE, name + ".p*.npz")):
        os.remove(old)
    parts, size = [{}], 0
    for k, v in out.items():
        n = np.asarray(v).nbytes
        if parts[-1] and size + n > PART_BYTES:
            parts.append({})
            size = 0
        parts[-1][k] = v
        size += n
    sizes = []
    for i, part in enumerate(parts):
        path = os.path.join(HERE, name + (".npz" if i == 0 else f".p{i}.npz"))
        np.savez_compressed(path, **part)
        sizes.append(os.path.getsize(path))
        assert sizes[-1] < 1 << 20, (path, sizes[-1])
    return sizes


def _run(cfg, bs, seed, store_weights):
    torch.manual_seed(seed)
    m = ref_model.LOGO_bearing_model(**cfg)
    _dropouts_off(m)
    _perturb(m, seed)
    x = torch.randn(bs, cfg["num_patch"] * cfg["patch_size"], generator=torch.Generator().manual_seed(seed + 7))
    y = torch.rand(bs, 1, generator=torch.Generator().manual_seed(seed + 8))
    out = {"x": x.numpy().copy(), "y": y.numpy().copy(), "seed": np.int64(seed), "theta": np.float64(THETA)}
    for k, v in cfg.items():
        out["cfg:" + k] = np.asarray(v, np.int64)
    if store_weights:
        out.update(mg.state_np(m, "sd:"))
    Q = cfg["num_patch"] * cfg["num_nodes"]
    t = {}
    hs = [m.MPNN.register_forward_hook(lambda mod, i, o: t.__setitem__("mpnn", o.detach().reshape(bs, Q, -1).transpose(0, 1).numpy().copy())),
          m.TD.register_forward_hook(lambda mod, i, o: t.__setitem__("lstm", o.detach().numpy().copy())),
          m.fc.fc1.register_forward_hook(lambda mod, i, o: t.__setitem__("fc1_pre", o.detach().numpy().copy())),
          m.fc.fc2.register_forward_hook(lambda mod, i, o: t.__setitem__("fc2_pre", o.detach().numpy().copy()))]
    orig_stft = torch.stft

    def spy_stft(*a, **k):
        z = orig_stft(*a, **k)
        t["spec"] = z.abs().detach().reshape(bs, cfg["num_patch"], z.shape[-2], z.shape[-1]).numpy().copy()
        return z
    torch.stft = spy_stft
    try:
        m.train()
        pred, gl = m(x, GL=True)
    finally:
        torch.stft = orig_stft
    for h in hs:
        h.remove()
    loss = torch.nn.functional.mse_loss(pred, y) + THETA * gl
    m.zero_grad()
    loss.backward()
    out["pred"], out["loss_gl"], out["loss"] = pred.detach().numpy().copy(), np.float64(gl.item()), np.float64(loss.item())
    out.update(t)
    m.eval()
    with torch.no_grad():
        out["pred_eval"] = m(x).numpy().copy()
    for n_, p in m.named_parameters():
        out["refgrad:" + n_] = p.grad.numpy().copy()
    # the reference's own fp64 run of the same forward: how far its fp32 outputs are from exact (kept out of the fixture)
    torch.set_default_dtype(torch.float64)
    try:
        m.double().train()
        hs = [m.MPNN.register_forward_hook(lambda mod, i, o: t.__setitem__("mpnn64", o.detach().reshape(bs, Q, -1).transpose(0, 1).numpy().copy())),
              m.TD.register_forward_hook(lambda mod, i, o: t.__setitem__("lstm64", o.detach().numpy().copy()))]
        with torch.no_grad():
            pred64, gl64 = m(x.double(), GL=True)
        for h in hs:
            h.remove()
    finally:
        torch.set_default_dtype(torch.float32)
    rel = lambda a, b: float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())      # noqa: E731
    out["_fp32_error"] = max(rel(out["mpnn"], t["mpnn64"]), rel(out["lstm"], t["lstm64"]), rel(out["pred"], pred64.numpy()),
                             rel(out["pred_eval"], pred64.numpy()), abs(gl.item() - gl64.item()) / abs(gl64.item()))
    return out


def _open(out):
    return int(((out["fc1_pre"] > 0).any(1) & (out["fc2_pre"] > 0).any(1)).sum())


def case_forward_backward(name, cfg, bs, seed, store_weights=True):
    while True:
        out = _run(cfg, bs, seed, store_weights)
        err = out.pop("_fp32_error")
        if 2 * _open(out) >= bs and err < ORACLE_BAR:
            break
        seed += 1
    sizes = _save_parts(name, out)
    print("wrote", name, "seed", seed, out["pred"].ravel()[:3], "loss", out["loss"], "gl", out["loss_gl"], "open", _open(out), "/", bs, sizes)


def case_training_curve(name, cfg, bs, steps, seed, lr, wd):
    """The reference's own LOGO_bearing.update (algorithms.py:619-629) on fixed batches, dropouts 0: the losses, the optimizer's
    learning rate behind every update (its MultiStepLR steps per update) and the end state."""
    while True:
        torch.manual_seed(seed)
        algo = get_algorithm_class("LOGO_bearing")(cfg, {"learning_rate": lr, "weight_decay": wd, "theta": THETA}, "cpu")
        _dropouts_off(algo.model)
        _perturb(algo.model, seed)
        xs = torch.randn(steps, bs, cfg["num_patch"] * cfg["patch_size"], generator=torch.Generator().manual_seed(seed + 20))
        ys = torch.rand(steps, bs, 1, generator=torch.Generator().manual_seed(seed + 9))
        out = {"xs": xs.numpy().copy(), "ys": ys.numpy().copy(), "lr": np.float64(lr), "wd": np.float64(wd), "seed": np.int64(seed),
               "theta": np.float64(THETA)}
        for k, v in cfg.items():
            out["cfg:" + k] = np.asarray(v, np.int64)
        out.update(mg.state_np(algo.model, "sd0:"))
        algo.train()
        losses, lrs = [], []
        for s in range(steps):
            losses.append(algo.update(xs[s], ys[s], 1)["loss"])
            lrs.append(algo.optimizer.param_groups[0]["lr"])
        if abs(losses[-1] - losses[0]) > 1e-3 * abs(losses[0]):          # a dead head trains nothing: take another seed
            break
        seed += 1
    out["losses"], out["lrs"] = np.asarray(losses, dtype=np.float64), np.asarray(lrs, dtype=np.float64)
    algo.eval()
    with torch.no_grad():
        out["eval_pred_end"] = algo.model(xs[0]).numpy().copy()
    out.update(mg.state_np(algo.model, "sd_end:"))
    sizes = _save_parts(name, out)
    print("wrote", name, "seed", seed, losses[:3], "...", losses[-1], "lrs", sorted(set(lrs), reverse=True), sizes)


def case_hparams(name):
    rows = {}
    for ds in ("PHM2012", "XJTU_SY"):
        for did in ("Condition_1", "Condition_2", "Condition_3"):
            hp = get_hparams_class(ds)(did)
            rows[f"{ds}/{did}"] = {"train_params": hp.train_params["LOGO_bearing"], "alg_hparams": hp.alg_hparams["LOGO_bearing"]}
    np.savez_compressed(os.path.join(HERE, name + ".npz"), rows_json=np.array(json.dumps(rows, sort_keys=True)))
    print("wrote", name, rows)


def _cfg(P, T, ns, h):
    return dict(patch_size=P, num_patch=T, input_dim=1 + P // ns, num_nodes=ns // 2 + 1, nperseg=ns, hidden_dim=h)


if __name__ == "__main__":
    case_forward_backward("logob_tiny_ns4_p8_t2_h1_bs3", _cfg(8, 2, 4, 1), 3, 51)
    # N = 2, nperseg = 2: both lower limits
    case_forward_backward("logob_ns2_p6_t3_h1_bs2", _cfg(6, 3, 2, 1), 2, 52)
    case_forward_backward("logob_ragged_ns4_p10_t3_h2_bs2", _cfg(10, 3, 4, 2), 2, 53)   # patch_size no multiple of nperseg
    case_forward_backward("logob_onepatch_ns4_p8_t1_h1_bs2", _cfg(8, 1, 4, 1), 2, 54)   # T = 1
    case_forward_backward("logob_phm2012_full_bs2", _cfg(64, 40, 8, 10), 2, 55, store_weights=False)
    case_forward_backward("logob_xjtu_full_bs2", _cfg(1024, 32, 32, 10), 2, 56, store_weights=False)
    case_training_curve("logob_train_curve_ns4_p8_t2_h1_bs4", _cfg(8, 2, 4, 1), 4, 28, 5, 1e-3, 1e-4)
    case_hparams("logob_hparams_rows")
