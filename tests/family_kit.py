"""One kit for the fused families' tests (LOGO, HierCorrPool, DVGTformer, GDAGDL, GAT_LSTM, LOGO_bearing, HierCorrPool_bearing, STFA;
AGCN_TF and GRU_CM, an older lineage, take grads_of, the harness run and the CPU checks): the leaf helpers, the element-wise gradient gate loop, the forward gate, the twin-model
Adam procedure, the training curve, the reference-harness run and the coverage refusals, each stated once.  A plain module: no
fixtures, no plugins.  Every tolerance, rtol, ladder and seed is the calling family's and is passed in: nothing here has a default for
one.  tests/test_family_kit_cpu.py plants faults into the numpy parts (check_grads, check_forward, assert_harness, adam_step_check).
Section 9, the stale-workspace check, serves every FlatModule family (tests/test_stale_workspace_gpu.py; its faults:
tests/test_stale_workspace_cpu.py)."""
import argparse
import json
import os
import sys
from typing import Callable, NamedTuple

import numpy as np
import torch

import adam_reference as R
import grad_gate as GG

GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"


# ---- 1. leaf helpers ---------------------------------------------------------------------------------------------------------------------
def rel(a, b):
    """max |a - b| relative to b's largest magnitude."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def rel_same_shape(a, b):
    """``rel`` that refuses to broadcast."""
    assert np.shape(a) == np.shape(b), (np.shape(a), np.shape(b))
    return rel(a, b)


def rel_finite(a, b):
    """``rel`` over the entries where ``b`` is finite; NaN must sit in the same places."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64).reshape(np.asarray(a).shape)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(b)
    return rel(a[ok], b[ok]) if ok.any() else 0.0


def load_case(name, prefix="sd:"):
    """(fixture, cfg of ints from its ``cfg:`` entries, the state dict stored under ``prefix``)."""
    z = np.load(os.path.join(GOLD, name + ".npz"))
    cfg = {k[4:]: int(z[k]) for k in z.files if k.startswith("cfg:")}
    sd = {k[len(prefix):]: z[k] for k in z.files if k.startswith(prefix)}
    return z, cfg, sd


def dev(a):
    return torch.from_numpy(np.asarray(a, np.float32)).to(DEV)


def grads_of(m, bucket=None):
    """name -> fp64 gradient, from the model's own flat gradient or from ``bucket`` (a sum of shards)."""
    flat = (m._grad_flat if bucket is None else bucket)[:m.num_live].detach().cpu().numpy().astype(np.float64)
    return {name: flat[off:off + int(np.prod(shape))].reshape(shape) for name, (off, shape) in m._layout.items()}


def _construct(cls, cfg, keys):
    return cls(**(cfg if keys is None else {k: cfg[k] for k in keys}))


def build_model(cls, cfg, sd, dropout=0.0, keys=None):
    """The module under a strict load of ``sd`` (float entries as fp32, integer buffers as they are), on the device."""
    m = _construct(cls, cfg, keys)
    as_f32 = lambda v: np.asarray(v, np.float32) if np.asarray(v).dtype.kind == "f" else np.asarray(v)      # noqa: E731
    m.load_state_dict({k: torch.from_numpy(as_f32(v)) for k, v in sd.items()}, strict=True)
    m.dropout_p = dropout
    return m.to(DEV)


def seeded_state(cls, cfg, seed, keys=None):
    """The fixtures' makers' recipe: the constructor's weights under ``seed``, moved by uniform(-0.1, 0.1) under Generator(seed + 1000)."""
    torch.manual_seed(seed)
    sd = _construct(cls, cfg, keys).state_dict()
    g = torch.Generator().manual_seed(seed + 1000)
    return {k: (v.clone() + torch.empty_like(v).uniform_(-0.1, 0.1, generator=g)).numpy() for k, v in sd.items()}


# ---- 2. the element-wise gradient gate -------------------------------------------------------------------------------------------------------
class ZeroRule(NamedTuple):
    """What a family asks of the tensors whose gradient is zero in exact arithmetic: how they are found, the largest magnitude the
    kernels may leave there, and what the printed line says about them."""
    detect: Callable        # (g64, ref32) -> names
    bound: Callable         # (name, g64, ref32) -> float
    note: Callable          # (names) -> the tail of the "<TAG>-GATE" line


def residue_bound(name, g64, ref32):
    """16 x max(the reference's own residue, 2^-23 x the model's largest gradient): the rounding residue of a sum that cancels."""
    gmax = max(float(np.abs(v).max()) for v in g64.values())
    return 16 * max(float(np.abs(ref32[name]).max()) if ref32.get(name) is not None else 0.0, 2.0 ** -23 * gmax)


def exact_zero_bound(name, g64, ref32):
    """Exactly zero in the oracle, so exactly zero in the reference and in the kernels."""
    assert not np.asarray(ref32[name]).any(), f"{name} must be exactly zero"
    return 0.0


RESIDUE = ZeroRule(GG.zero_in_exact_arithmetic, residue_bound, lambda zero: f"; zero in exact arithmetic: {zero}")
EXACT_ZERO = ZeroRule(lambda g64, ref32: sorted(k for k, v in g64.items() if not v.any()), exact_zero_bound, lambda zero: "")


def check_grads(what, tag, got, g64, ref32, rtol, zero_rule=None, exact_zero=(), noise_partner=None, ladder=None, verbose=False):
    """Every tensor of ``g64`` through grad_gate at ``rtol``, its floor from the reference's own fp32 gradient ``ref32`` (and from its
    ``noise_partner``'s, where it names one).  ``exact_zero`` names must be exact zeros in ``got``; the tensors ``zero_rule`` detects
    are held to its bound.  Prints "<tag>-GATE" (and "<tag>-LADDER", the worst ratio at each rtol of ``ladder``); ``verbose`` prints
    every tensor's ratio, not only those above 0.25.  Returns the detected names."""
    assert set(got) - set(exact_zero) == set(g64) - set(exact_zero), sorted(set(got) ^ set(g64))
    for k in exact_zero:
        assert not got[k].any(), f"{k} must be exactly zero"
    zero = zero_rule.detect(g64, ref32) if zero_rule else []
    rungs = np.zeros(len(ladder or ()))
    worst = (0.0, None)
    for k in g64:
        assert got[k].shape == g64[k].shape, k
        if k in exact_zero:
            continue
        if k in zero:
            bound = zero_rule.bound(k, g64, ref32)
            assert np.abs(got[k]).max() <= bound, (k, np.abs(got[k]).max(), bound)
            continue
        floor = GG.floor_for(ref32[k], g64[k])
        partner = noise_partner(k) if noise_partner else None
        if partner:                     # a one-element tensor shares the noise of the tensor it is summed from
            floor = max(floor, GG.floor_for(ref32[partner], g64[partner]))
        if ladder:
            rungs = np.maximum(rungs, [GG.gate(got[k], g64[k], r, floor)[0] for r in ladder])
        ratio, where = GG.gate(got[k], g64[k], rtol, floor)
        if verbose or ratio > 0.25:
            print(f"  grad {k}: gate {ratio:.3f} at {where}  rel {rel(got[k], g64[k]):.2e}  max|g| {np.abs(g64[k]).max():.2e}")
        worst = max(worst, (ratio, k))
    print(f"{tag}-GATE {what}: worst gradient gate ratio {worst[0]:.3f} ({worst[1]})" + (zero_rule.note(zero) if zero_rule else ""))
    if ladder:
        print(f"{tag}-LADDER {what}: " + " ".join(f"{v:.3f}" for v in rungs))
    assert worst[0] <= 1.0, worst
    return zero


# ---- 3. the forward gate -------------------------------------------------------------------------------------------------------------------
def tap_errs(m, bs, want, taps, cmp=rel, same_shape=True):
    """{tap: error} over ``taps``.  ``same_shape``: the reference's tensor has the tap's shape; without it (a reference that keeps
    another grouping of the same axes) the same elements in the same order."""
    errs = {}
    for k in taps:
        got, w = m.tap(bs, k).cpu().numpy(), np.asarray(want[k])
        assert got.shape == w.shape if same_shape else got.size == w.size, (k, got.shape, w.shape)
        errs[k] = cmp(got, w.reshape(got.shape))
    return errs


def pred_err(pred, want, cmp=rel):
    return {"pred": cmp(pred.detach().cpu().numpy().reshape(-1), np.asarray(want["pred"]).reshape(-1))}


def loss_err(loss, want_loss):
    """{} where there is no loss to compare (an eval forward)."""
    return {"loss": abs(float(loss) - want_loss) / abs(want_loss)} if loss is not None else {}


def check_forward(what, tag, errs, tol):
    """Print the family's "<tag>-GATE ...: forward" line and hold every error below ``tol``."""
    print(f"{tag}-GATE {what}: forward " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < tol, (k, v)


# ---- 4. the optimizer inside the fused step ----------------------------------------------------------------------------------------------------
def adam_step_check(after, before, g, k, wd, what, first=0):
    """One fused Adam step in numpy: (p, m, v) ``after`` against fp64 Adam of ``before`` and the step's own gradient ``g`` within
    adam_reference's bounds on every element from ``first`` on; below ``first`` (a gradless range) the gradient is zero and nothing
    moved, bit for bit.  Returns the error/bound ratios."""
    assert not g[:first].any()
    for got, was in zip(after, before):
        assert np.array_equal(np.ascontiguousarray(got[:first]).view(np.uint32), np.ascontiguousarray(was[:first]).view(np.uint32))
    return R.check(tuple(t[first:] for t in after), before[0][first:], g[first:], before[1][first:], before[2][first:], k, wd, 1.0,
                   what=f"{what}, step {k}")


def adam_twin_check(ready, x, y, family, first=0, prepare_moments=None, after_step=None, **step_kw):
    """The twin-model procedure of tests/test_fused_adam_families_gpu.py (its LR, WD, STEP0 and SEED; bounds from
    tests/adam_reference.py).  ``ready()`` builds the model; twin A takes one step without an optimizer, twin B three with FusedAdam
    from moments on the gradient's scale.  ``prepare_moments(m0, v0, model)`` may edit the moments in place;
    ``after_step(before, after, g)`` sees every step's (p, m, v) pair and gradient.  Prints "ADAM-RATIO family ..."; returns twin B."""
    from gnn_rul_benchmarking_amd.optim import FusedAdam
    from test_fused_adam_families_gpu import LR, SEED, STEP0, WD, _bits, _np
    assert WD > 0

    def twin():
        m = ready()
        m._seed = SEED
        return m
    a = twin()
    p0 = _np(a.flat_params)
    _, loss_a = a.fused_mse_step(x, y, **step_kw)
    g_a, loss_a = _np(a.bucket[:a.num_live]), float(loss_a)
    assert np.isfinite(g_a).all() and np.array_equal(_bits(_np(a.flat_params)), _bits(p0))
    b = twin()
    opt = FusedAdam(b, lr=LR, weight_decay=WD)
    m0, v0 = R.moments_like(g_a, np.random.default_rng(12))
    if prepare_moments:
        prepare_moments(m0, v0, b)
    s = opt.state_dict()
    s.update(step=STEP0, exp_avg=torch.from_numpy(m0).to(DEV), exp_avg_sq=torch.from_numpy(v0).to(DEV))
    opt.load_state_dict(s)
    worst = dict(p=0.0, m=0.0, v=0.0)
    for k in (STEP0 + 1, STEP0 + 2, STEP0 + 3):
        before = tuple(_np(t) for t in (b.flat_params, opt._exp_avg, opt._exp_avg_sq))
        _, loss_b = b.fused_mse_step(x, y, opt, **step_kw)
        g = _np(b.bucket[:b.num_live])
        after = tuple(_np(t) for t in (b.flat_params, opt._exp_avg, opt._exp_avg_sq))
        if k == STEP0 + 1:
            assert np.array_equal(_bits(g), _bits(g_a)) and float(loss_b) == loss_a
        r = adam_step_check(after, before, g, k, WD, family, first)
        worst = {q: max(worst[q], r[q]) for q in worst}
        if after_step:
            after_step(before, after, g)
    assert opt._steps == STEP0 + 3
    print(f"ADAM-RATIO family {family}: " + " ".join(f"{q}={worst[q]:.3f}" for q in "pmv"))
    return b


# ---- 5. the training curve ---------------------------------------------------------------------------------------------------------------------
def curve_check(method, tag, cfg, z, sd0, bars, dropout_off):
    """len(z["losses"]) update() steps of the registry's ``method`` from ``sd0`` against the reference's own (fixture ``z``).  ``bars``
    holds the family's bars: "steps" (the fixture's length), "first3" and "every" (the losses, relative; None: not asked), "eval" (the
    eval prediction at the end) and, where the family gates them, "params" (every end-state tensor the fixture stores, as
    ``sd_end:`` or ``sd<steps>:``; a num_batches_tracked must equal the step count).  ``dropout_off`` sets the model's dropout to 0;
    without it the configuration must already say 0.  Returns (algorithm, its end state dict)."""
    from gnn_rul_benchmarking_amd.algorithms import get_algorithm_class
    hp = {"learning_rate": float(z["lr"]), "weight_decay": float(z["wd"])}
    if "theta" in z.files:
        hp["theta"] = float(z["theta"])
    algo = get_algorithm_class(method)(cfg, hp, DEV)
    algo.model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd0.items()}, strict=True)
    if dropout_off:
        algo.model.dropout_p = 0.0
    assert algo.model.dropout_p == 0.0
    algo.to(DEV).train()
    xs, ys = torch.from_numpy(z["xs"]).to(DEV), torch.from_numpy(z["ys"]).to(DEV)
    ref, steps = z["losses"], bars["steps"]
    assert xs.size(0) == len(ref) == steps
    losses = np.asarray([algo.update(xs[s], ys[s], 1)["loss"] for s in range(steps)])
    print(f"{tag}-GATE curve: worst loss ratio", np.abs(losses / ref - 1).max())
    if bars["first3"] is not None:
        assert np.max(np.abs(losses[:3] - ref[:3]) / ref[:3]) < bars["first3"]
    assert np.max(np.abs(losses - ref) / ref) < bars["every"], (losses.tolist(), ref.tolist())
    sd = algo.model.state_dict()
    if "params" in bars:
        prefix = "sd_end:" if any(k.startswith("sd_end:") for k in z.files) else f"sd{steps}:"
        assert sorted(k[len(prefix):] for k in z.files if k.startswith(prefix)) == sorted(sd)
        for k in sd:
            if k.endswith("num_batches_tracked"):
                assert int(sd[k]) == int(z[prefix + k]) == steps
            else:
                assert rel_same_shape(sd[k].cpu().numpy(), z[prefix + k]) < bars["params"], k
    algo.eval()
    with torch.no_grad():
        assert rel(algo.model(xs[0]).cpu().numpy(), z["eval_pred_end"]) < bars["eval"]
    return algo, sd


# ---- 6. the reference-harness run ----------------------------------------------------------------------------------------------------------------
MAX_RULS = {"CMAPSS": 125, "PHM2012": 1.0}


def synthetic_data(z, dataset, n_test=None):
    """The synthetic data set a harness fixture was made on ((x_train, y_train), (x_test, y_test)), checked against its checksum."""
    if GOLD not in sys.path:
        sys.path.insert(0, GOLD)
    import synth
    make = {"CMAPSS": synth.synthetic_cmapss, "PHM2012": synth.synthetic_phm2012}[dataset]
    data = make(int(z["seed"]), int(z["n_train"]), int(z["n_test"]) if n_test is None else n_test)
    assert abs(data[0][0].astype(np.float64).sum() - float(z["x_train_checksum"])) < 1e-6
    return data


def model_dropout_off(algo):
    algo.model.dropout_p = 0.0


def harness_run(tmp_path, monkeypatch, method, dataset, dataset_id, z, data=None, no_dropout=None, configure=None):
    """--GNN_method ``method`` through this package's harness on the GPU, on the data set the reference's harness run ``z`` was made
    on.  ``data``: (train.pt's dict, test.pt's dict) where the default -- ``synthetic_data`` as numpy with the data set's max_ruls -- is
    not what the fixture used.  ``no_dropout(algorithm)`` switches dropout off on the constructed algorithm; ``configure(trainer)``
    runs before train(): the checks and switches that belong to one hparams row.  Returns (trainer, per-epoch metrics)."""
    from gnn_rul_benchmarking_amd import trainer as T
    if data is None:
        (xtr, ytr), (xte, yte) = synthetic_data(z, dataset)
        data = ({"samples": xtr, "labels": ytr, "max_ruls": MAX_RULS[dataset]}, {"samples": xte, "labels": yte, "max_ruls": MAX_RULS[dataset]})
    d = tmp_path / "data" / dataset / dataset_id
    os.makedirs(d)
    torch.save(data[0], d / "train.pt")
    torch.save(data[1], d / "test.pt")
    monkeypatch.chdir(tmp_path)
    if no_dropout:
        base = T.get_algorithm_class(method)

        class NoDropout(base):
            def __init__(self, *a, **k):
                super().__init__(*a, **k)
                no_dropout(self)
        monkeypatch.setattr(T, "get_algorithm_class", lambda n: NoDropout)
    args = argparse.Namespace(save_dir=str(tmp_path / "logs"), experiment_description="exp", run_description="r", GNN_method=method,
                              data_path=str(tmp_path / "data"), dataset=dataset, dataset_id=dataset_id,
                              bearing_id="Testing_bearing_1", num_runs=1, device=DEV)
    tr = T.GNN_RUL_trainer(args)
    tr.train_configs["num_epochs"] = int(z["epochs"])
    if configure:
        configure(tr)
    per_epoch = []
    orig = tr.calc_results_per_run

    def spy(run_id):
        if isinstance(tr.pred_labels, dict):
            per_epoch.append({k: T._calc_metrics(tr.pred_labels[k], tr.true_labels[k], tr.max_ruls[k]) for k in tr.pred_labels})
        else:
            per_epoch.append(T._calc_metrics(tr.pred_labels, tr.true_labels, tr.max_ruls))
        return orig(run_id)
    tr.calc_results_per_run = spy
    tr.train()
    return tr, per_epoch


def assert_harness(what, per_epoch, sd, z, bars):
    """The three comparisons of a harness run against the reference's (fixture ``z``; columns Score_v1, Score_v2, MAE, RMSE), each
    asked where ``bars`` names it:  "rmse_abs": max |RMSE - ref| / "rmse_scale" (125 on C-MAPSS: the normalised scale);  "rel": the
    relative error of the columns from "rel_from" on (2: MAE and RMSE; 0: all four);  "final": every ``final:`` tensor of the fixture
    against the state dict ``sd`` (None: not compared) relative to its largest element, the key behind "final_prefix" (the older
    fixtures store the algorithm's key, the newer ones the model's).  ``what`` heads the printed metrics (None: nothing is printed)."""
    got, ref = np.asarray(per_epoch, np.float64), z["per_epoch"]
    if what:
        print(f"{what} harness per-epoch got/ref:\n", got, "\n", ref)
    assert got.shape == ref.shape == (int(z["epochs"]), 4)
    if "rmse_abs" in bars:
        assert np.max(np.abs(got[:, 3] - ref[:, 3]) / bars["rmse_scale"]) < bars["rmse_abs"]
    c = bars["rel_from"]
    assert np.max(np.abs(got[:, c:] - ref[:, c:]) / np.abs(ref[:, c:])) < bars["rel"]
    if "final" in bars:
        finals = [k for k in z.files if k.startswith("final:")]
        assert finals
        for k in finals:
            a, b = np.asarray(sd[bars["final_prefix"] + k[6:]], np.float64), z[k].astype(np.float64)
            assert a.shape == b.shape, k
            assert np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30) < bars["final"], k


def state_of(trainer):
    """The trained algorithm's state dict as numpy (what ``assert_harness`` compares ``final:`` tensors against)."""
    return {k: v.cpu().numpy() for k, v in trainer.algorithm.state_dict().items()}


# ---- 7. coverage: outside the limits nothing is launched ------------------------------------------------------------------------------------------
def refused_outside_limits(m, x, **step_kw):
    """A model outside its kernels' limits refuses the forward and the fused step, makes no workspace and writes nothing."""
    import pytest
    m = m.to(x.device)
    with pytest.raises(RuntimeError, match="do not cover this configuration"):
        m(x)
    with pytest.raises(RuntimeError, match="do not cover this configuration"):
        m.fused_mse_step(x, torch.zeros(x.size(0), device=x.device), **step_kw)
    assert not m._bufs and not m._grad_flat.any() and not m.bucket.any()


# ---- 8. without a GPU ---------------------------------------------------------------------------------------------------------------------------
def registry_check(method, needs_train_mode="dropout"):
    """The registry serves the algorithm under the reference's name and refuses the model's."""
    import pytest
    from gnn_rul_benchmarking_amd import algorithms as A
    cls = A.get_algorithm_class(method)
    assert cls is getattr(A, method)
    with pytest.raises(NotImplementedError, match=f"Algorithm not found: {method}_model"):
        A.get_algorithm_class(method + "_model")
    assert cls.needs_train_mode == needs_train_mode and cls.supports_graphs is False
    return cls


def cpu_input_raises(m, x, **step_kw):
    import pytest
    with pytest.raises(RuntimeError, match="HIP path only"):
        m(x)
    with pytest.raises(RuntimeError, match="HIP path only"):
        m.fused_mse_step(x, torch.zeros(x.size(0)), **step_kw)


def hparams_rows_check(method, npz, present, absent, absent_is_all=False):
    """The fixture ``npz`` (the reference's hparams rows, read by the fixtures' maker) against this package's hparams.  ``present``: the
    "<dataset>/<id>" keys that serve the method -- a mapping to (train_params, alg_hparams) where the family's file states the rows
    itself; ``absent``: keys that must not serve it (``absent_is_all``: they are the fixture's whole ``absent_json`` list).  Returns
    the fixture's rows."""
    from gnn_rul_benchmarking_amd.hparams import get_hparams_class

    def row(key):
        ds, did = key.split("/")
        return get_hparams_class(ds)(None if did == "None" else did)
    z = np.load(os.path.join(GOLD, npz))
    rows = json.loads(str(z["rows_json"]))
    assert sorted(rows) == sorted(present)
    for key, ref in rows.items():
        h = row(key)
        assert h.train_params[method] == ref["train_params"] and h.alg_hparams[method] == ref["alg_hparams"], key
        if isinstance(present, dict):
            assert (ref["train_params"], ref["alg_hparams"]) == present[key], key
    if absent_is_all:
        assert sorted(json.loads(str(z["absent_json"]))) == sorted(absent)
    for key in absent:
        h = row(key)
        assert method not in h.alg_hparams and method not in h.train_params, key
    return rows


# ---- 9. a call on a stale workspace ------------------------------------------------------------------------------------------------------------
# A workspace need not be initialised and need not be preserved between calls (include/rulgnn.h).  ``stale_run`` makes one fresh model and
# one fresh optimizer, primes the workspaces, puts one of STALE_FILLS into the workspace of the batch immediately before every call and
# returns everything the call produced; ``stale_compare`` holds a fill's run to the "zero" run.  Nothing here imports the package: the
# model only has to look like a FlatModule (tests/test_stale_workspace_cpu.py plants faults into a numpy one).
STALE_FILLS = ("zero", "nan", "other-batch", "same-batch")
STALE_CALLS = ("step", "eval", "autograd")
STALE_B_BIG = 37
QUIET_NAN = 0x7FC00000


class StaleCase(NamedTuple):
    """One family for the stale-workspace check.  ``ready()``: a fresh model from the family's state dict, in train mode, dropout at the
    family's own rate, a fixed ``_seed``;  ``make_opt(model)``: a fresh optimizer over it;  ``draw(B, seed)``: (x, y) of batch ``B`` on the
    model's device, the same for the same arguments;  ``other_state(model)``: another state dict for the same model;  ``step_kw``: what
    the family's ``fused_mse_step`` takes beyond (x, y, optimizer);  ``bar``: None for equal bit patterns, else the largest |difference|
    relative to the tensor's largest magnitude."""
    ready: Callable
    make_opt: Callable
    draw: Callable
    other_state: Callable
    step_kw: dict
    bar: object


def _host(t):
    return t.detach().cpu().numpy().copy()


def _words(ws):
    return ws.view(torch.int32)


def _state_of(m, opt):
    """Everything a call may move, as host arrays: parameters, moments, the state dict's buffers, the batch statistics, the counters."""
    out = {"flat_params": _host(m.flat_params)}
    sd = opt.state_dict()
    out["exp_avg"], out["exp_avg_sq"], out["adam_steps"] = _host(sd["exp_avg"]), _host(sd["exp_avg_sq"]), np.asarray(int(sd["step"]))
    for k, v in m.state_dict().items():
        out["sd:" + k] = _host(v)
    if getattr(m, "_bn_batch", None) is not None:
        out["_bn_batch"] = _host(m._bn_batch)
    out["_step"] = np.asarray(int(getattr(m, "_step", 0)))
    return out


def _same_state(a, b):
    return a.keys() == b.keys() and all(a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes() for k in a)


def _load(m, sd):
    m.state_dict()                               # (brings pending BatchNorm counters up to date before they are overwritten)
    m.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)


def _stale_fill(m, B, fill, source):
    """Put ``fill`` into the workspace of batch ``B`` and return how many of its fp32 words are non-zero behind it."""
    ws = m._bufs[B][0]
    assert ws.numel() % 256 == 0, "workspace sizes are 256-byte multiples: no partial word"
    w = _words(ws)
    if fill == "zero":
        ws.zero_()
    elif fill == "nan":
        w.fill_(QUIET_NAN)
        probe = w[[0, w.numel() // 2, w.numel() - 1]].tolist()
        assert probe == [QUIET_NAN] * 3, probe
    elif fill == "other-batch":
        n = min(ws.numel(), source.numel())
        ws[:n].copy_(source[:n])
        at = [0, n // 8, n // 4 - 1]
        assert w[at].tolist() == _words(source[:n])[at].tolist()
    else:
        assert fill == "same-batch" and source is None               # what the step before left: no explicit fill
    return int(torch.count_nonzero(w))


def stale_run(case, B, fill, call):
    """One fresh model and optimizer of ``case`` through ``call`` at batch ``B`` with ``fill`` in the workspace before every launch of it.
    Returns {name: host array} of everything the call produced, "filled:<i>" among it: the non-zero words of the workspace before call i."""
    assert fill in STALE_FILLS and call in STALE_CALLS
    m = case.ready()
    opt = case.make_opt(m)
    x, y = case.draw(B, B)
    m._pin_bufs = True                                                  # nothing is evicted: the workspace filled is the one the call uses
    before = _state_of(m, opt)
    m.eval()
    with torch.no_grad():
        for b in (B, STALE_B_BIG) if fill == "other-batch" else (B,):   # the workspace of a batch size exists only after a call at it
            m(case.draw(b, 1000 + b)[0])
    m.train()
    assert _same_state(before, _state_of(m, opt)), "priming moved the model or the optimizer"
    source = None
    if fill in ("other-batch", "same-batch"):                           # a training step on other data under another state dict
        b = STALE_B_BIG if fill == "other-batch" else B
        home, step = {k: v.clone() for k, v in m.state_dict().items()}, getattr(m, "_step", None)
        _load(m, case.other_state(m))
        xo, yo = case.draw(b, 2000 + b)
        m.fused_mse_step(xo, yo, **case.step_kw)
        _load(m, home)
        if step is not None:
            m._step = step
        if getattr(m, "_bn_batch", None) is not None:
            m._bn_batch.copy_(torch.from_numpy(before["_bn_batch"]))
        m.bucket.zero_()
        assert _same_state(before, _state_of(m, opt)), "the step that made the stale workspace left its mark outside it"
        if fill == "other-batch":
            source = m._bufs[b][0].clone()
    out = {}

    def collect(tag, **more):
        for k, v in more.items():
            out[f"{tag}:{k}"] = _host(v)
        for k, v in _state_of(m, opt).items():
            out[f"{tag}:{k}"] = v

    if call == "step":
        for i in (1, 2):                                                # the second starts from what the first left and from moved parameters
            out[f"filled:{i}"] = np.asarray(_stale_fill(m, B, fill, source))
            pred, loss = m.fused_mse_step(x, y, opt, **case.step_kw)
            collect(f"step{i}", pred=pred, loss=loss, bucket=m.bucket[:m.num_live + 1])
    elif call == "eval":
        m.eval()
        out["filled:1"] = np.asarray(_stale_fill(m, B, fill, source))
        with torch.no_grad():
            pred = m(x)
        collect("eval", pred=pred)
    else:
        out["filled:1"] = np.asarray(_stale_fill(m, B, fill, source))   # before the forward only: the backward is entitled to its tape
        pred = m(x)
        loss = torch.nn.functional.mse_loss(pred, y.reshape(-1, 1))
        loss.backward()
        grads = [p.grad.reshape(-1) for p in m._named() if p.grad is not None]
        collect("autograd", pred=pred, loss=loss, grad=torch.cat(grads), bucket=m.bucket[:m.num_live])
    return out


def stale_baseline_ok(base, call):
    """The "zero" run can be trusted: its workspace held zeros, everything it produced is finite and its gradient is not all zero."""
    for k, v in base.items():
        if k.startswith("filled:"):
            assert int(v) == 0, k
        elif v.dtype.kind == "f":
            assert np.isfinite(v).all(), k
    if call != "eval":
        for k in [k for k in base if k.endswith(":bucket") or k.endswith(":grad")]:
            assert base[k].any(), f"{k} is all zero"


def stale_compare(base, got, fill, bar):
    """``got`` (the run under ``fill``) against ``base`` (the "zero" run), tensor by tensor: equal bit patterns where ``bar`` is None, else
    finite and within ``bar`` of the tensor's largest magnitude (integer tensors always equal).  The fill must have taken."""
    assert fill != "zero" and base.keys() == got.keys(), sorted(set(base) ^ set(got))
    for k, want in base.items():
        have = got[k]
        if k.startswith("filled:"):
            assert int(have) > 0, f"{k}: the {fill} fill left the workspace as the baseline's"
            continue
        assert have.shape == want.shape and have.dtype == want.dtype, k
        if bar is None or want.dtype.kind != "f":
            if have.tobytes() != want.tobytes():
                a, b = have.astype(np.float64).reshape(-1), want.astype(np.float64).reshape(-1)
                bad = np.flatnonzero(~((a == b) | (np.isnan(a) & np.isnan(b))))
                raise AssertionError(f"{k} under the {fill} fill: {bad.size} of {a.size} elements differ from the zero fill's, first at "
                                     f"{bad[:8].tolist()}: {a[bad[:4]].tolist()} against {b[bad[:4]].tolist()}")
        else:
            assert np.isfinite(have).all(), f"{k} under the {fill} fill is not finite"
            err = rel_same_shape(have, want)
            assert err <= bar, f"{k} under the {fill} fill: {err:.3e} of the tensor's largest magnitude, the bar is {bar:.1e}"
