"""The HierCorrPool_bearing oracle (tests/hiercorrpool_bearing_oracle.py) against outputs of the reference itself
(tests/golden/hcpb_*.npz, written by tests/golden/make_golden_hiercorrpool_bearing.py running the reference on the CPU, dropout 0): the
spectrogram ``torch.stft`` returned inside the forward, the encoder output, X', A', H, the train and eval predictions, the loss and the
BatchNorm buffers at 1e-6 relative to the tensor's largest value (tests/test_hiercorrpool_oracle_golden.py's bar; the maker keeps a seed
only when the reference's own fp32 outputs lie within it of its own fp64 run), every parameter gradient element by element
(tests/grad_gate.py), and the reference's own twelve-step training curve against the torch restatement's ``torch_step`` in fp64."""
import numpy as np
import pytest

import grad_gate as GG
import hiercorrpool_bearing_oracle as O
from family_kit import load_case, rel_same_shape as rel

SMALL = ["hcpb_small_ns4_p8_t7_bs6", "hcpb_ragged_ns4_p10_t3_bs3", "hcpb_p65_ns4_bs2"]
FORWARD_ONLY = ["hcpb_ns2_p6_t3_bs3"]          # N = 2: several gradients are zero in exact arithmetic, the fixture holds none
CURVE = "hcpb_train_curve_ns4_p8_t7_bs8"
TAPS = ("encoder", "pooled_x", "pooled_adj", "H")
BAR = 1e-6
RTOL = 5e-4          # the family's gradient gate (tests/test_hiercorrpool_bearing_gpu.py); the oracle stays far inside


@pytest.mark.parametrize("name", SMALL + FORWARD_ONLY)
def test_forward_matches_reference(name):
    z, cfg, sd = load_case(name)
    assert list(sd) == O.state_keys() and list(cfg) == O.KEYS
    bs = z["x"].shape[0]
    assert 2 * int((z["fc1_pre"] > 0).sum()) >= bs           # the maker's condition: the final leaky ReLU is open on half the samples
    N, f = O.stft_shape(cfg)
    assert (cfg["num_nodes"], cfg["input_dim"]) == (N, f) and z["spec"].shape == (bs, cfg["num_patch"], N, f)
    assert rel(O.stft_mag(z["x"], cfg), z["spec"]) < BAR
    inp = O.block1_input(z["x"], cfg)                         # channel n f + j, four zero rows on each side
    assert inp.shape == (bs, cfg["num_patch"] + 8, N * f) and not inp[:, :4].any() and not inp[:, -4:].any()
    assert np.array_equal(inp[:, 4:-4].reshape(bs, -1, N, f), O.stft_mag(z["x"], cfg))
    loss, g, fw = O.loss_and_grads(sd, z["x"], z["y"], cfg)
    assert fw["encoder"].shape[1] == O.lengths(cfg["num_patch"])[-1]
    for tap in TAPS:
        assert rel(fw[tap], z[tap]) < BAR, tap
    assert rel(fw["pred"], z["pred"]) < BAR
    assert abs(loss - float(z["loss"])) < BAR * abs(float(z["loss"]))
    after = O.running_after(sd, fw)
    for k, v in after.items():
        assert rel(v, z["bn_after:" + k]) < BAR, k
    for l in (1, 2, 3):
        assert int(z["bn_after:" + O.ENC.format(l) + "1.num_batches_tracked"]) == 1
    ev = O.forward({**sd, **after}, z["x"], cfg, training=False)
    assert rel(ev["pred"], z["pred_eval"]) < BAR
    assert bool([k for k in z.files if k.startswith("refgrad:")]) == (name in SMALL)


@pytest.mark.parametrize("name", SMALL)
def test_gradients_match_reference(name):
    z, cfg, sd = load_case(name)
    _, g, _ = O.loss_and_grads(sd, z["x"], z["y"], cfg)
    ref32 = {k: z["refgrad:" + k] for k in O.param_names()}
    assert GG.zero_in_exact_arithmetic(g, ref32) == [O.ZERO_GRAD]
    gmax = max(np.abs(v).max() for v in g.values())
    assert np.abs(g[O.ZERO_GRAD]).max() <= 1e-12 * gmax and np.abs(ref32[O.ZERO_GRAD]).max() <= 1e-5 * gmax
    for k in O.param_names():
        if k == O.ZERO_GRAD:
            continue
        assert g[k].shape == ref32[k].shape, k
        # the reference's fp32 gradient against the fp64 oracle under the gate the kernels face; the floor is grad_gate's for a reference
        # without noise of its own: MARGIN fp32 ulps of the tensor's largest element
        ratio, where = GG.gate(ref32[k], g[k], RTOL, GG.floor_for(g[k], g[k]))
        assert ratio <= 1.0, (k, ratio, where)
        assert rel(ref32[k], g[k]) < 1e-4, k


def test_torch_restatement_equals_the_oracle():
    import torch
    z, cfg, sd = load_case(SMALL[1])                          # the ragged patch: torch.stft's framing against the formula's
    loss, g, fw = O.loss_and_grads(sd, z["x"], z["y"], cfg)
    pred, loss_t, g_t = O.torch_grads(sd, z["x"], z["y"], cfg, torch.float64)
    assert rel(pred, fw["pred"]) < 1e-10 and abs(loss - loss_t) < 1e-10 * loss
    for k in O.param_names():
        if k != O.ZERO_GRAD:
            assert rel(g_t[k], g[k]) < 1e-8, k
    assert rel(O.torch_window(torch.tensor(z["x"].astype(np.float64)), cfg).numpy(), O.window(z["x"], cfg)) < 1e-12


def test_training_curve_matches_torch_step():
    """Twelve steps of ``torch_step`` (the restatement, fp64, torch's Adam, no dropout) against the reference's own
    HierCorrPool_bearing.update in fp32."""
    import torch
    z, cfg, sd0 = load_case(CURVE, "sd0:")
    assert list(sd0) == O.state_keys()
    sd = {k: torch.tensor(np.asarray(v, np.float64)) if v.dtype.kind == "f" else torch.tensor(v) for k, v in sd0.items()}
    names = O.param_names()
    for k in names:
        sd[k].requires_grad_(True)
    opt = torch.optim.Adam([sd[k] for k in names], lr=float(z["lr"]), weight_decay=float(z["wd"]))
    xs, ys = torch.tensor(z["xs"].astype(np.float64)), torch.tensor(z["ys"].astype(np.float64))
    losses = [float(O.torch_step(sd, opt, xs[s], ys[s], cfg, dropout_p=0.0).detach()) for s in range(len(z["losses"]))]
    assert len(losses) == 12 and np.abs(np.asarray(losses) / z["losses"] - 1).max() < 1e-5
    for k in O.state_keys():
        if k.endswith("num_batches_tracked"):
            assert int(z["sd_end:" + k]) == 12
        else:
            assert rel(sd[k].detach().numpy(), z["sd_end:" + k]) < 2e-4, k
    with torch.no_grad():
        ev = O.torch_forward(sd, xs[0], cfg, training=False).numpy()
    assert rel(ev, z["eval_pred_end"]) < 1e-4
