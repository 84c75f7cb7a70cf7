"""tests/family_kit.py on synthetic data, without a GPU: the gate loop, the forward gate, the harness comparison and the Adam step
comparison each pass on clean data and raise AssertionError on each planted fault.  The numbers below are this file's own (a gate of
rtol 1e-3, a forward tolerance of 1e-4, harness bars of 1e-3 and 2e-3); the families pass theirs."""
import copy

import numpy as np
import pytest
import torch

import adam_reference as R
import family_kit as K
import grad_gate as GG

RTOL, TOL = 1e-3, 1e-4


def grads():
    """(got, g64, ref32): three ordinary tensors, a one-element one ("s", summed from "a") and one that is zero in exact arithmetic
    ("z": 1e-12 of the model's largest gradient, the reference holds 1e-8 of residue there)."""
    rng = np.random.default_rng(0)
    g64 = {"a": rng.standard_normal((3, 4)), "b": rng.standard_normal(5), "c": rng.standard_normal((2, 2, 2)), "s": np.array([1e-6]),
           "z": 1e-12 * rng.standard_normal(4)}
    ref32 = {k: v + 1e-7 * rng.standard_normal(v.shape) for k, v in g64.items()}
    ref32["s"] = g64["s"] + 1e-12
    ref32["z"] = 1e-8 * np.array([1.0, -0.5, 0.25, 0.0])
    got = {k: v + 1e-8 * rng.standard_normal(v.shape) for k, v in g64.items()}
    got["s"] = g64["s"] + 1e-13
    got["z"] = 1e-8 * rng.uniform(-1, 1, 4)
    return got, g64, ref32


def gate(got, g64, ref32, **kw):
    return K.check_grads("case", "KIT", got, g64, ref32, RTOL, **dict(dict(zero_rule=K.RESIDUE), **kw))


def bound_of(k, g64, ref32, e):
    return RTOL * abs(g64[k][e]) + GG.floor_for(ref32[k], g64[k])


def test_check_grads_passes_on_clean_data_prints_its_lines_and_returns_the_detected_names(capsys):
    got, g64, ref32 = grads()
    assert gate(got, g64, ref32, ladder=[RTOL, RTOL / 2]) == ["z"]
    out = capsys.readouterr().out
    assert "KIT-GATE case: worst gradient gate ratio 0." in out and "; zero in exact arithmetic: ['z']" in out
    assert "KIT-LADDER case: 0." in out and "  grad " not in out
    gate(got, g64, ref32, verbose=True)
    assert capsys.readouterr().out.count("  grad ") == 4            # every gated tensor, not only the ratios above 0.25


@pytest.mark.parametrize("k,e", [("a", (1, 2)), ("b", (4,)), ("c", (0, 1, 1))])
def test_one_element_off_by_twice_its_bound_fails_and_by_half_passes(k, e):
    got, g64, ref32 = grads()
    got[k][e] = g64[k][e] + 0.5 * bound_of(k, g64, ref32, e)
    gate(got, g64, ref32)
    got[k][e] = g64[k][e] - 2 * bound_of(k, g64, ref32, e)
    with pytest.raises(AssertionError):
        gate(got, g64, ref32)


def test_a_nan_element_a_wrong_shape_a_missing_and_an_extra_name_fail():
    got, g64, ref32 = grads()
    bad = copy.deepcopy(got)
    bad["b"][2] = np.nan
    with pytest.raises(AssertionError):
        gate(bad, g64, ref32)
    bad = dict(got, c=got["c"].reshape(4, 2))
    with pytest.raises(AssertionError):
        gate(bad, g64, ref32)
    with pytest.raises(AssertionError):
        gate({k: v for k, v in got.items() if k != "b"}, g64, ref32)
    with pytest.raises(AssertionError):
        gate(dict(got, extra=np.zeros(2)), g64, ref32)


def test_exactly_zero_names_must_be_exact_zeros():
    got, g64, ref32 = grads()
    got["v"] = np.zeros(3)                                           # a tensor the oracle does not hold (a gradless parameter)
    gate(got, g64, ref32, exact_zero=("v",))
    got["v"][1] = 1e-30
    with pytest.raises(AssertionError):
        gate(got, g64, ref32, exact_zero=("v",))
    got, g64, ref32 = grads()                                        # ... and one it holds: not gated, held to zero
    got["b"] = np.zeros(5)
    gate(got, g64, ref32, exact_zero=("b",))
    got["b"][0] = 1e-30
    with pytest.raises(AssertionError):
        gate(got, g64, ref32, exact_zero=("b",))


def test_a_tensor_zero_in_exact_arithmetic_just_under_and_just_over_its_bound():
    got, g64, ref32 = grads()
    gmax = max(np.abs(v).max() for v in g64.values())
    bound = 16 * max(1e-8, 2.0 ** -23 * gmax)
    assert K.residue_bound("z", g64, ref32) == bound
    got["z"] = np.array([0.0, 0.99 * bound, 0.0, 0.0])
    gate(got, g64, ref32)
    got["z"][1] = -1.01 * bound
    with pytest.raises(AssertionError):
        gate(got, g64, ref32)
    # a family's own rule goes in as a ZeroRule: here a bound of half the residue rule's
    half = K.ZeroRule(GG.zero_in_exact_arithmetic, lambda k, g, r: 0.5 * K.residue_bound(k, g, r), lambda zero: f": {len(zero)} tensors")
    got["z"][1] = 0.6 * bound
    gate(got, g64, ref32)
    with pytest.raises(AssertionError):
        gate(got, g64, ref32, zero_rule=half)
    # without a rule nothing is detected: the tensor goes through the gate like any other, where a residue of 1e-8 is far too much
    with pytest.raises(AssertionError):
        gate(got, g64, ref32, zero_rule=None)


def test_the_exact_zero_rule_asks_zeros_of_the_oracle_the_reference_and_the_kernels(capsys):
    got, g64, ref32 = grads()
    for d in (got, g64, ref32):
        d["z"] = np.zeros(4)
    assert gate(got, g64, ref32, zero_rule=K.EXACT_ZERO) == ["z"]
    assert capsys.readouterr().out.strip().endswith(")")            # LOGO's line: nothing behind the worst tensor's name
    with pytest.raises(AssertionError):
        gate(dict(got, z=np.array([0, 0, 1e-30, 0])), g64, ref32, zero_rule=K.EXACT_ZERO)
    with pytest.raises(AssertionError, match="must be exactly zero"):
        gate(got, g64, dict(ref32, z=np.array([0, 0, 1e-30, 0])), zero_rule=K.EXACT_ZERO)


def test_a_noise_partner_floor_admits_what_the_tensors_own_floor_refuses():
    got, g64, ref32 = grads()
    own, partner = GG.floor_for(ref32["s"], g64["s"]), GG.floor_for(ref32["a"], g64["a"])
    assert partner > 4 * (RTOL * 1e-6 + own)
    got["s"] = g64["s"] + 2 * (RTOL * 1e-6 + own)
    with pytest.raises(AssertionError):
        gate(got, g64, ref32)
    gate(got, g64, ref32, noise_partner=lambda k: "a" if k == "s" else None)
    got["s"] = g64["s"] + 2 * (RTOL * 1e-6 + partner)
    with pytest.raises(AssertionError):
        gate(got, g64, ref32, noise_partner=lambda k: "a" if k == "s" else None)


# ---- the forward gate --------------------------------------------------------------------------------------------------------------------------
class Taps:
    """A model's tap(): what the kernels left, as tensors."""
    def __init__(self, taps):
        self.taps = taps

    def tap(self, bs, k):
        return torch.from_numpy(self.taps[k])


def forward(m, pred, loss, want, cmp=K.rel, same_shape=True):
    errs = {**K.pred_err(pred, want, cmp), **K.tap_errs(m, 2, want, [k for k in ("h", "lstm") if k in want], cmp, same_shape), **K.loss_err(loss, 0.25)}
    K.check_forward("case", "KIT", errs, TOL)
    return errs


def test_check_forward_clean_a_tap_off_by_twice_the_tolerance_a_prediction_and_a_loss(capsys):
    rng = np.random.default_rng(1)
    want = {"pred": rng.uniform(0, 1, (2, 1)), "h": rng.standard_normal((2, 3, 4)), "lstm": rng.standard_normal((2, 5))}
    m, pred = Taps({k: want[k].copy() for k in ("h", "lstm")}), torch.from_numpy(want["pred"].reshape(-1).copy())
    assert list(forward(m, pred, 0.25, want)) == ["pred", "h", "lstm", "loss"]
    assert capsys.readouterr().out.startswith("KIT-GATE case: forward pred=0.00e+00 h=0.00e+00 lstm=0.00e+00 loss=0.00e+00")
    assert list(forward(m, pred, None, want)) == ["pred", "h", "lstm"]                    # an eval forward has no loss
    m.taps["h"][1, 2, 3] += 0.5 * TOL * np.abs(want["h"]).max()
    forward(m, pred, 0.25, want)
    m.taps["h"][1, 2, 3] += 1.5 * TOL * np.abs(want["h"]).max()
    with pytest.raises(AssertionError):
        forward(m, pred, 0.25, want)
    m.taps["h"] = want["h"].copy()
    with pytest.raises(AssertionError):
        forward(m, pred + 2 * TOL, 0.25, want)
    with pytest.raises(AssertionError):
        forward(m, pred, 0.25 * (1 + 2 * TOL), want)
    m.taps["h"] = want["h"].reshape(2, 12).copy()                                         # the same elements under another grouping
    with pytest.raises(AssertionError):
        forward(m, pred, 0.25, want)
    forward(m, pred, 0.25, want, same_shape=False)


def test_nan_must_sit_where_the_references_is():
    want = {"pred": np.array([0.5, np.nan, 0.25]), "h": np.array([[1.0, np.nan], [2.0, 3.0], [np.nan, np.nan]])}
    m, pred = Taps({"h": want["h"].copy()}), torch.from_numpy(want["pred"].copy())
    forward(m, pred, None, want, K.rel_finite)
    m.taps["h"] = np.array([[1.0, 1.0], [2.0, 3.0], [np.nan, np.nan]])                    # a number where the reference has NaN
    with pytest.raises(AssertionError):
        forward(m, pred, None, want, K.rel_finite)
    m.taps["h"] = np.array([[1.0, np.nan], [np.nan, 3.0], [np.nan, np.nan]])              # NaN in another place
    with pytest.raises(AssertionError):
        forward(m, pred, None, want, K.rel_finite)
    m.taps["h"] = want["h"].copy()
    with pytest.raises(AssertionError):
        forward(m, torch.tensor([0.5, 0.5, np.nan]), None, want, K.rel_finite)
    with pytest.raises(AssertionError):
        K.rel_same_shape(np.zeros((2, 1)), np.zeros(2))


# ---- the harness comparison ----------------------------------------------------------------------------------------------------------------
class Fixture(dict):
    files = property(lambda self: list(self))


CMAPSS_BARS = dict(rmse_abs=1e-3, rmse_scale=125.0, rel=1e-3, rel_from=2, final=2e-3, final_prefix="model.")


def harness():
    rng = np.random.default_rng(2)
    z = Fixture(epochs=3, per_epoch=rng.uniform(20, 40, (3, 4)), **{"final:fc.weight": rng.standard_normal((2, 3)), "final:fc.bias": rng.standard_normal(2)})
    sd = {"model." + k[6:]: z[k].astype(np.float32) for k in z if k.startswith("final:")}
    return z, [tuple(r) for r in z["per_epoch"]], sd


def test_assert_harness_clean_a_metric_and_a_final_tensor_off_by_twice_their_bars(capsys):
    z, per_epoch, sd = harness()
    K.assert_harness("KIT", per_epoch, sd, z, CMAPSS_BARS)
    assert capsys.readouterr().out.startswith("KIT harness per-epoch got/ref:\n")
    for col, off in ((2, 2e-3 * z["per_epoch"][1, 2]), (3, 2e-3 * z["per_epoch"][1, 3]), (3, 2e-3 * 125.0)):
        bad = [list(r) for r in per_epoch]
        bad[1][col] += off
        with pytest.raises(AssertionError):
            K.assert_harness("KIT", bad, sd, z, CMAPSS_BARS)
    bad = [list(r) for r in per_epoch]
    bad[1][0] *= 1.5                                                  # a score column: not among the columns from rel_from on ...
    K.assert_harness("KIT", bad, sd, z, CMAPSS_BARS)
    with pytest.raises(AssertionError):                               # ... unless the family asks all four
        K.assert_harness("KIT", bad, sd, z, dict(CMAPSS_BARS, rel_from=0))
    with pytest.raises(AssertionError):
        K.assert_harness("KIT", per_epoch[:2], sd, z, CMAPSS_BARS)    # an epoch short
    bad = {k: v.copy() for k, v in sd.items()}
    bad["model.fc.weight"][1, 1] += 1e-3 * np.abs(z["final:fc.weight"]).max()
    K.assert_harness("KIT", per_epoch, bad, z, CMAPSS_BARS)
    bad["model.fc.weight"][1, 1] += 3e-3 * np.abs(z["final:fc.weight"]).max()
    with pytest.raises(AssertionError):
        K.assert_harness("KIT", per_epoch, bad, z, CMAPSS_BARS)
    K.assert_harness("KIT", per_epoch, None, z, {k: v for k, v in CMAPSS_BARS.items() if not k.startswith("final")})


# ---- the Adam step comparison ------------------------------------------------------------------------------------------------------------------
def adam_step(n=64, k=7, wd=1e-4):
    p, g, m0, v0 = R.inputs(n, 5)
    hp = R.DEFAULT
    after = tuple(t.astype(np.float32) for t in R.reference(p, g, m0, v0, k, hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], wd, 1.0))
    return after, (p, m0, v0), g, k, wd


def test_adam_step_check_clean_an_element_stepped_twice_one_never_stepped_and_a_gradless_range():
    after, before, g, k, wd = adam_step()
    hp = R.DEFAULT
    r = K.adam_step_check(after, before, g, k, wd, "KIT")
    assert set(r) == set("pmv") and max(r.values()) <= 1.0
    i = int(np.argmax(np.abs(g) > 1e-3))
    twice = tuple(t.copy() for t in after)
    again = R.reference(after[0][i], g[i], after[1][i], after[2][i], k + 1, hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], wd, 1.0)
    for t, v in zip(twice, again):
        t[i] = v
    with pytest.raises(AssertionError, match="x its error bound"):
        K.adam_step_check(twice, before, g, k, wd, "KIT")
    never = tuple(t.copy() for t in after)
    for t, was in zip(never, before):
        t[i] = was[i]
    with pytest.raises(AssertionError, match="x its error bound"):
        K.adam_step_check(never, before, g, k, wd, "KIT")
    # a gradless range in front: zero gradient, nothing moved, not even by the weight decay
    g0 = g.copy()
    g0[:3] = 0.0
    after0 = tuple(t.copy() for t in adam_step()[0])
    for t, was in zip(after0, before):
        t[:3] = was[:3]
    K.adam_step_check(after0, before, g0, k, wd, "KIT", first=3)
    with pytest.raises(AssertionError):
        K.adam_step_check(after0, before, g0, k, wd, "KIT")           # as optimized elements they were never stepped
    after0[0][1] = np.nextafter(after0[0][1], np.float32(np.inf))
    with pytest.raises(AssertionError):
        K.adam_step_check(after0, before, g0, k, wd, "KIT", first=3)  # one ulp of movement in the gradless range
    with pytest.raises(AssertionError):
        K.adam_step_check(after, before, g, k, wd, "KIT", first=3)    # a gradient there
