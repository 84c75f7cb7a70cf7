"""HierCorrPool_bearing HIP path vs the reference's golden outputs and vs the fp64 oracle (GPU).

Gates (HierCorrPool's, tests/test_hiercorrpool_gpu.py: it is the same chain behind another front end).  The block-1 input, predictions,
taps, the loss and the BatchNorm running statistics after a step: TOL = 1e-4 relative to the tensor's largest value.  Gradients: element
by element through tests/grad_gate.py at rtol 5e-4 and margin 16; the floor's noise term is the REFERENCE's fp32 gradient against the
fp64 oracle (the fixture's ``refgrad:`` entries; without a fixture an fp32 run of the torch restatement, ``torch.stft`` included, on the
CPU), never the kernels' output.  ``matrix.bias`` (constant along the softmax axis) must be exactly 0.  Every test prints its worst gate
ratio ("HCP-GATE ...").

Worst figures on an MI355X (profiles/r30_hiercorrpool_bearing.md): block-1 input 2.0e-7 (nperseg 32); gradient gate ratios (1 passes)
0.042 over the fixtures, 0.224 over the five reference geometries (PHM2012 Condition_2) and 0.267 at batch 1, 0.160 at the limit
shapes; training curve: losses within 4.5e-7, end state within 9.6e-7."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import family_kit as K
import hiercorrpool_bearing_oracle as O
from family_kit import DEV, grads_of, rel_same_shape as rel
from test_hiercorrpool_bearing_cpu import ROWS, make_cfg
from test_hiercorrpool_bearing_oracle_golden import CURVE, FORWARD_ONLY, SMALL, TAPS, load_case
from test_hiercorrpool_gpu import check_forward, check_grads, keep_mask

pytestmark = pytest.mark.gpu
TOL, RTOL = 1e-4, 5e-4
KEYS = O.KEYS
STFT_GRID = 2048           # csrc/hiercorrpool.hip HCPB_GRID: the packing kernel's workgroups, one output row (sample, padded step) at a time


def build_model(cfg, sd, dropout=0.0):
    from gnn_rul_benchmarking_amd.hiercorrpool_bearing import HierCorrPool_bearing_model
    return K.build_model(HierCorrPool_bearing_model, cfg, sd, dropout, KEYS)


def seeded_state(cfg, seed):
    """The state dict the constructor gives under ``seed`` (numpy)."""
    from gnn_rul_benchmarking_amd.hiercorrpool_bearing import HierCorrPool_bearing_model
    torch.manual_seed(seed)
    return {k: v.numpy().copy() for k, v in HierCorrPool_bearing_model(**{k: cfg[k] for k in KEYS}).state_dict().items()}


@functools.lru_cache(maxsize=None)
def fixture_oracle(name):
    z, cfg, sd = load_case(name)
    loss, g, fw = O.loss_and_grads(sd, z["x"], z["y"], cfg)
    return z, cfg, sd, loss, g, fw


def signal(bs, cfg, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((bs, cfg["num_patch"] * cfg["patch_size"])).astype(np.float32), rng.uniform(0, 1, bs).astype(np.float32)


# ---- 3a. the front end alone ---------------------------------------------------------------------------------------------------------------
FRONT = {"ns4-p8": make_cfg(8, 7, 4, 2, 2, 12, 3), "ns4-p10-ragged": make_cfg(10, 3, 4, 2, 2, 12, 2), "ns2-p6": make_cfg(6, 3, 2, 1, 1, 12, 2),
         "ns8-p5-reflect-both-sides": make_cfg(5, 7, 8, 2, 2, 12, 3), "ns32-p512-xjtu": make_cfg(512, 2, 32, 1, 1, 8, 2)}


@pytest.mark.parametrize("wrap", [False, True], ids=["bs3", "grid-wraps"])
@pytest.mark.parametrize("tag", sorted(FRONT))
def test_stft_input_matches_oracle_and_does_not_depend_on_the_workspace(tag, wrap):
    from gnn_rul_benchmarking_amd import _lib
    cfg = FRONT[tag]
    rows, C0 = cfg["num_patch"] + 8, cfg["num_nodes"] * cfg["input_dim"]
    bs = STFT_GRID // rows + 5 if wrap else 3                # more rows than workgroups: every workgroup walks on to a second row
    assert (bs * rows > STFT_GRID) == wrap
    x, _ = signal(bs, cfg, 11)
    m = build_model(cfg, seeded_state(cfg, 3)).eval()
    xd = torch.from_numpy(x).to(DEV)
    with torch.no_grad():
        pred = m(xd.reshape(bs, cfg["num_patch"], -1)).clone()          # (any shape with numel / bs == num_patch * patch_size)
    got = m.tap(bs, "stft")
    want = O.block1_input(x, cfg)
    assert got.shape == want.shape == (bs, rows, C0)
    assert not got[:, :4].any() and not got[:, -4:].any(), "the pad rows are exactly zero"
    err = rel(got.cpu().numpy(), want)
    print(f"HCP-GATE stft {tag} bs {bs}: {err:.2e}")
    assert err < TOL
    # nothing may rely on what the workspace held: NaN over the region, the same forward, the same bits
    off = _lib.load().rulgnn_hcpb_tap_offset(C.byref(m._shape(bs)), 4)
    ws = m._bufs[bs][0].view(torch.float32)
    ws[off:off + bs * rows * C0] = float("nan")
    assert torch.isnan(m.tap(bs, "stft")).all()
    with torch.no_grad():
        again = m(xd)
    assert torch.equal(m.tap(bs, "stft"), got) and torch.equal(again, pred) and torch.isfinite(pred).all()


# ---- 3b. the reference's fixtures ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL + FORWARD_ONLY)
def test_fixture_forward_taps_statistics_and_gradients(name):
    z, cfg, sd, loss64, g64, fw = fixture_oracle(name)
    m = build_model(cfg, sd).train()
    x, y = torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(z["y"]).to(DEV)
    bs = x.size(0)
    pred, loss = m.fused_mse_step(x, y)
    running = {k[9:]: z[k] for k in z.files if k.startswith("bn_after:") and "running" in k}
    check_forward(name, m, bs, pred, loss, {**{t: z[t] for t in TAPS}, "pred": z["pred"]}, float(z["loss"]), running)   # the reference itself ...
    check_forward(name + "-oracle", m, bs, pred, loss, fw, loss64, O.running_after(sd, fw))                               # ... and the fp64 oracle
    spec = m.tap(bs, "stft")[:, 4:-4].reshape(bs, cfg["num_patch"], cfg["num_nodes"], cfg["input_dim"]).cpu().numpy()
    assert rel(spec, z["spec"]) < TOL
    for l in (1, 2, 3):
        assert int(m.state_dict()[O.ENC.format(l) + "1.num_batches_tracked"]) == 1
    if name in SMALL:
        check_grads(name, grads_of(m), g64, {k: z["refgrad:" + k] for k in O.param_names()})
    m.eval()
    with torch.no_grad():
        ev = m(x)
    want = O.forward({k: v.cpu().numpy() for k, v in m.state_dict().items()}, z["x"], cfg, training=False)["pred"]
    assert ev.shape == (bs, 1) and rel(ev.cpu().numpy(), want) < TOL and rel(ev.cpu().numpy(), z["pred_eval"]) < TOL


# ---- 3c. full width against the fp64 oracle --------------------------------------------------------------------------------------------
def step_against_oracle(what, cfg, bs, seed):
    sd = seeded_state(cfg, seed)
    x, y = signal(bs, cfg, seed)
    loss64, g64, fw = O.loss_and_grads(sd, x, y, cfg)
    _, _, g32 = O.torch_grads(sd, x, y, cfg, torch.float32)
    m = build_model(cfg, sd).train()
    pred, loss = m.fused_mse_step(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV))
    check_forward(what, m, bs, pred, loss, fw, loss64, O.running_after(sd, fw))
    assert rel(m.tap(bs, "stft").cpu().numpy(), O.block1_input(x, cfg)) < TOL
    check_grads(what, grads_of(m), g64, g32)


@pytest.mark.parametrize("key,bs", [("PHM2012/Condition_1", 3), ("PHM2012/Condition_2", 3), ("PHM2012/Condition_3", 3), ("XJTU_SY/Condition_1", 2),
                                    ("XJTU_SY/Condition_2", 2), ("PHM2012/Condition_2", 1)])
def test_full_width_step_matches_oracle(key, bs):
    """The five reference geometries (XJTU_SY's second and third rows are one): num_patch 80 and 128, d 480 and 720 among them."""
    step_against_oracle(f"{key}-full-bs{bs}", ROWS[key], bs, 100 + bs)


# ---- 3d. limits ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [make_cfg(8, 128, 4, 1, 1, 72, 16), make_cfg(32, 80, 32, 15, 10, 72, 16)], ids=["P128-M16", "N17-d720-C3-1020-M16"])
def test_just_inside_the_limits_matches_oracle(cfg):
    """num_patch = 128 beside M = 16; and N = 17, d = 720, C3 = 1020, M = 16 together: the largest LDS the gate admits (113 212 B)."""
    step_against_oracle("limits-" + "-".join(str(cfg[k]) for k in KEYS), cfg, 2, 7)


@pytest.mark.parametrize("cfg", [make_cfg(8, 129, 4, 1, 1, 72, 2), make_cfg(8, 128, 4, 181, 1, 724, 2), make_cfg(64, 2, 34, 1, 1, 8, 2),
                                 make_cfg(32, 2, 32, 16, 16, 8, 2)], ids=["P129", "d724", "nperseg34", "C3-1088"])
def test_just_outside_each_limit_is_not_covered_and_launches_nothing(cfg):
    from gnn_rul_benchmarking_amd.hiercorrpool_bearing import HierCorrPool_bearing_model
    if cfg["encoder_conv_kernel"] == 724:      # (no L' 4 h equals 724: the constructor's reshape check is not what is under test)
        m = HierCorrPool_bearing_model(**dict(cfg, hidden_dim=10, embedding_dim=10, encoder_conv_kernel=72))
        m.encoder_conv_kernel, m.embedding_dim = 724, 1
    else:
        m = HierCorrPool_bearing_model(**cfg)
    K.refused_outside_limits(m, torch.zeros(2, cfg["num_patch"] * cfg["patch_size"], device=DEV))


# ---- 3e. dropout -----------------------------------------------------------------------------------------------------------------------
def test_training_with_dropout_matches_oracle():
    name = SMALL[0]
    z, cfg, sd, _, _, fw0 = fixture_oracle(name)
    bs, C1, L1 = z["x"].shape[0], cfg["hidden_dim"] * cfg["num_nodes"], O.lengths(cfg["num_patch"])[0]
    m = build_model(cfg, sd, dropout=0.35).train()
    keep = keep_mask(bs, C1, L1, m._seed, m._step + 1, 0.35)
    assert 0.4 < keep.mean() < 0.9
    loss64, g64, fw = O.loss_and_grads(sd, z["x"], z["y"], cfg, keep_mask=keep)
    _, _, g32 = O.torch_grads(sd, z["x"], z["y"], cfg, torch.float32, keep_scale=(keep / 0.65).astype(np.float32))
    x, y = torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(z["y"]).to(DEV)
    pred, loss = m.fused_mse_step(x, y)
    check_forward(name + "-dropout", m, bs, pred, loss, fw, loss64)
    check_grads(name + "-dropout", grads_of(m), g64, g32)
    assert rel(pred.cpu().numpy().reshape(-1, 1), fw0["pred"]) > 10 * TOL, "the mask must reach the prediction"
    # a shard that starts at global sample 3 draws rows 3... of the unsharded mask
    assert np.array_equal(keep_mask(bs - 3, C1, L1, m._seed, 1, 0.35, offset=3), keep_mask(bs, C1, L1, m._seed, 1, 0.35)[3:])
    m2 = build_model(cfg, sd, dropout=0.35).train()
    m2._seed = m._seed
    m2.fused_mse_step(x[3:], y[3:], sample_offset=3)
    sh = O.forward(sd, z["x"][3:], cfg, True, keep[3:])         # (batch statistics of the shard, the whole batch's mask rows)
    assert rel(m2.tap(bs - 3, "encoder").cpu().numpy(), sh["encoder"]) < TOL


# ---- 3f. entry and path equalities -----------------------------------------------------------------------------------------------------
def _case(name=SMALL[0]):
    z, cfg, sd = load_case(name)
    return cfg, sd, torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(z["y"]).to(DEV)


@pytest.mark.parametrize("name", [SMALL[0], SMALL[2]])
def test_forward_then_backward_equals_fwdbwd_bit_for_bit(name):
    cfg, sd, x, y = _case(name)
    m = build_model(cfg, sd, dropout=0.35).train()
    m.fused_mse_step(x, y)
    fused = m.bucket[:m.num_live + 1].clone()
    assert not fused[m._layout[O.ZERO_GRAD][0]:m._layout[O.ZERO_GRAD][0] + cfg["num_nodes_out"]].any()
    m._step = 0
    m.fused_mse_step(x, y)
    assert torch.equal(m.bucket[:m.num_live + 1], fused)                      # twice the same step: the same bits
    m2 = build_model(cfg, sd, dropout=0.35).train()
    m2._seed = m._seed
    x2, yv = m2._step_inputs(x, y)
    shp = m2._shape(x2.size(0))
    a = m2._args(shp, x2, True, 1, y=yv)
    m2._call("forward", shp, a)
    m2._call("backward", shp, a)
    assert torch.equal(m2.bucket[:m2.num_live + 1], fused)


def _algorithm(cfg, sd, lr=1e-3, wd=1e-4):
    from gnn_rul_benchmarking_amd.algorithms import HierCorrPool_bearing
    algo = HierCorrPool_bearing({k: cfg[k] for k in KEYS}, {"learning_rate": lr, "weight_decay": wd}, DEV)
    algo.model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    algo.model.dropout_p = 0.0
    return algo.to(DEV).train()


def test_autograd_path_equals_fused_path_and_update_reference_style_equals_update():
    cfg, sd, x, y = _case()
    m = build_model(cfg, sd).train()
    m.fused_mse_step(x, y)
    fused = m._grad_flat[:m.num_live].clone()
    m2 = build_model(cfg, sd).train()
    torch.nn.functional.mse_loss(m2(x), y).backward()
    auto = torch.cat([t.grad.reshape(-1) for t in m2._named()])
    assert torch.equal(auto, fused)
    assert torch.equal(m2._bn, m._bn) and int(m2.state_dict()[O.ENC.format(1) + "1.num_batches_tracked"]) == 1
    algos = [_algorithm(cfg, sd) for _ in range(2)]
    la = algos[0].update(x, y, 1)["loss"]
    lb = algos[1].update_reference_style(x, y, 1)["loss"]
    assert abs(la - lb) <= 1e-6 * abs(la)
    sa, sb = algos[0].state_dict(), algos[1].state_dict()
    for k in sa:
        assert rel(sb[k].cpu().numpy(), sa[k].cpu().numpy()) < 1e-6, k       # one Adam step from the same gradient bits
    assert not torch.equal(sa["model.fc_0.weight"].cpu(), torch.from_numpy(np.asarray(sd["fc_0.weight"])))


# ---- 3g. training curve ----------------------------------------------------------------------------------------------------------------
def test_training_curve_matches_reference_algorithm():
    """Twelve update() steps of algorithms.HierCorrPool_bearing, constructed directly, against the reference's own: every loss within
    TOL relative, the end state within 3e-3 (tests/test_hiercorrpool_gpu.py's bar for a trained state)."""
    z, cfg, sd0 = load_case(CURVE, "sd0:")
    algo = _algorithm(cfg, sd0, float(z["lr"]), float(z["wd"]))
    xs, ys = torch.from_numpy(z["xs"]).to(DEV), torch.from_numpy(z["ys"]).to(DEV)
    assert xs.size(0) == 12
    losses = [algo.update(xs[s], ys[s], 1)["loss"] for s in range(12)]
    print("HCP-GATE hcpb curve: worst loss ratio", np.abs(np.asarray(losses) / z["losses"] - 1).max())
    assert np.abs(np.asarray(losses) / z["losses"] - 1).max() < TOL, (losses, z["losses"].tolist())
    algo.eval()
    with torch.no_grad():
        assert rel(algo.model(xs[0]).cpu().numpy(), z["eval_pred_end"]) < 3e-3
    sd = algo.model.state_dict()
    assert list(sd) == O.state_keys()
    worst = 0.0
    for k in sd:
        if k.endswith("num_batches_tracked"):
            assert int(sd[k]) == int(z["sd_end:" + k]) == 12
        else:
            worst = max(worst, rel(sd[k].cpu().numpy(), z["sd_end:" + k]))
            assert rel(sd[k].cpu().numpy(), z["sd_end:" + k]) < 3e-3, k
    print("HCP-GATE hcpb curve: worst end-state error", worst)


# ---- 3h. the optimizer inside the fused step -------------------------------------------------------------------------------------------
def test_fused_step_applies_adam_to_every_element_exactly_once():
    """The twin-model procedure (family_kit.adam_twin_check: steps 7-9), dropout on."""
    z, cfg, sd = load_case(SMALL[0])
    b = K.adam_twin_check(lambda: build_model(cfg, sd, dropout=0.35).train(), torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(z["y"]).to(DEV),
                          "HierCorrPool_bearing")
    assert int(b.state_dict()[O.ENC.format(3) + "1.num_batches_tracked"]) == 3
