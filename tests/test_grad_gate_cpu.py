"""The per-element gradient gate (tests/grad_gate.py) on the CPU, over every golden fixture that holds the reference's gradients:

1. the gate sees what the whole-tensor rules cannot: one element below 1e-3 of its tensor's largest, doubled, passes every family's
   existing max-norm check and fails the gate, at that element;
2. the reference's own fp32 gradients pass by the construction's margin, which pins the name / shape / layout mapping between the
   oracles and the fixtures;
3. the tensors detected as zero in exact arithmetic are the ones each family's ``check_grads`` special-cases (plus, pinned per
   fixture, the ones that are zero on that fixture's data);
4. tests/golden/grad_noise.json (the reference's measured noise, tests/golden/make_grad_noise.py) is reproduced to 1 %.

Writes nothing."""
import importlib.util
import json
import os

import numpy as np
import pytest

import grad_cases as GC
import grad_gate as GG

CASES = GC.all_cases()
IDS = [n for _, n in CASES]


@pytest.fixture(autouse=True)
def _quiet():
    with np.errstate(over="ignore"):          # oracle/stnet_oracle.py's sigmoid on the un-normalised Chebyshev values (1e4..1e8)
        yield


def test_every_family_and_fixture_is_covered():
    wrap = sorted(f for f, n in CASES if "_wrap_" in n)
    assert wrap == sorted(f for f in GC.FAMILIES if f != "HAGCN") and all(GC.case(f, n).wrap == ("_wrap_" in n) for f, n in CASES)
    held = sorted(os.path.basename(p)[:-4] for p in __import__("glob").glob(os.path.join(GC.GOLDEN, "*.npz")) if GC._holds_grads(p))
    assert sorted(IDS) == held                                   # no fixture with grad: keys falls outside the families' patterns
    assert {f for f, _ in CASES} == set(GC.FAMILIES) and len(GC.FAMILIES) == 13 and len(CASES) >= 69


# ---- 1. what the max-norm cannot see ------------------------------------------------------------------------------------------------

# half of what each family's whole-tensor rule allows, as a share of the tensor's largest element (the other half is left to the
# distance between the fixture's fp32 gradient, which that rule compares with, and the fp64 one): 5e-4 / 2; STGNN's atol 2e-4 / 2
BLIND = {"STGNN": 1e-4}


def _small_elements(c, k):
    """Indices of the elements of tensor k that lie in the whole-tensor rule's blind band (below 1e-3 of the tensor's largest, and
    below half of what the family's rule allows) and above twice the floor, smallest first."""
    g = np.abs(c.g64[k]).reshape(-1)
    idx = np.nonzero((g < min(1e-3, BLIND.get(c.family, 2.5e-4)) * g.max()) & (g > 2 * c.floor(k)))[0]
    return idx[np.argsort(g[idx])]


@pytest.mark.parametrize("family", list(GC.FAMILIES))
def test_a_doubled_small_element_passes_the_max_norm_and_fails_the_gate(family):
    took_part = 0
    for name in GC.fixtures(family):
        c = GC.case(family, name)
        for k in c.live:
            idx = _small_elements(c, k)
            if not idx.size:
                continue                                          # no element in the blind band: left out of the demonstration
            i = int(idx[0])
            got = {n: v for n, v in c.g64.items()}
            bad = c.g64[k].copy()
            bad.reshape(-1)[i] *= 2.0
            got[k] = bad
            assert GC.maxnorm_failures(c, got) == [], (name, k)  # the family's existing check does not notice
            r, at = GG.gate(bad, c.g64[k], c.rtol, c.floor(k))
            assert r > 1.0 and at == tuple(int(v) for v in np.unravel_index(i, bad.shape)), (name, k, r, at)
            took_part += 1
    assert took_part >= 1, family


@pytest.mark.parametrize("family,name", CASES, ids=IDS)
def test_zeroing_the_smaller_half_of_a_tensor_fails_the_gate(family, name):
    """A lost contribution (a dropped tile-edge column, a skipped tail) as a stand-in for ``got``: in every live tensor in turn, the
    half of the elements that are smallest in magnitude set to zero.  The gate notices exactly where the largest element lost is above
    what it allows (a tensor that is half zeros, or whose smaller half lies under the reference's own noise, loses nothing that can
    be told), and that is the case for at least one tensor of every fixture, most of them in all but HAGCN."""
    c = GC.case(family, name)
    seen = 0
    for k in c.live:
        g = c.g64[k]
        if g.size < 2:
            continue
        bad = g.copy()
        order = np.argsort(np.abs(g).reshape(-1))
        bad.reshape(-1)[order[:g.size // 2]] = 0.0
        lost = np.abs(g).reshape(-1)[order[g.size // 2 - 1]]
        r, _ = GG.gate(bad, g, c.rtol, c.floor(k))
        assert (r > 1.0) == (lost > c.rtol * lost + c.floor(k)), (k, r)
        seen += r > 1.0
    assert seen >= 1 and (family == "HAGCN" or seen > len(c.live) // 2), (seen, len(c.live))


def test_gate_rejects_a_layout_mismatch_and_reports_the_index():
    g = np.arange(1.0, 13.0).reshape(3, 4)
    with pytest.raises(ValueError):
        GG.gate(g.T, g, 1e-3, 1e-6)                               # a transposed tensor is an error, never a broadcast
    with pytest.raises(ValueError):
        GG.gate(g.reshape(-1), g, 1e-3, 1e-6)
    with pytest.raises(ValueError):
        GG.gate(g, g, 1e-3, 0.0)
    bad = g.copy()
    bad[2, 1] += 1.0
    r, at = GG.gate(bad, g, 1e-3, 1e-6)
    assert at == (2, 1) and abs(r - 1.0 / (1e-3 * g[2, 1] + 1e-6)) < 1e-9 * r
    bad[0, 3] = np.nan
    assert GG.gate(bad, g, 1e-3, 1e-6) == (np.inf, (0, 3))
    assert GG.noise(bad[1:], g[1:]) == 1.0
    assert GG.floor_for(g, g) == 16 * 2.0 ** -23 * 12.0 and GG.floor_for(g + 1e-3, g) == pytest.approx(16e-3)
    assert [tuple(int(v) for v in ij) for ij in zip(*np.nonzero(GG.over_gate(bad, g, 1e-3, 1e-6)))] == [(0, 3), (2, 1)]


def test_a_transposed_gradient_fails_the_gate_where_the_shape_does_not_catch_it():
    """A square weight read in the other order has the right shape: only the values can tell."""
    c = GC.case("ST_GCN", "stgcn_cmapss_14x30_bs32")
    sq = [k for k in c.live if c.g64[k].ndim == 2 and c.g64[k].shape[0] == c.g64[k].shape[1] and c.g64[k].shape[0] > 1]
    assert sq
    for k in sq:
        r, _ = GG.gate(np.ascontiguousarray(c.g64[k].T), c.g64[k], c.rtol, c.floor(k))
        assert r > 1.0, k


# ---- 2. the reference passes by the margin ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family,name", CASES, ids=IDS)
def test_reference_fp32_gradients_pass_by_the_margin(family, name):
    c = GC.case(family, name)
    assert c.live
    for k in c.live:
        assert c.ref32[k].shape == c.g64[k].shape and c.ref32[k].dtype == np.float32, k
        r, at = GG.gate(c.ref32[k], c.g64[k], c.rtol, c.floor(k))
        assert r <= 1.0 / GG.MARGIN, (k, r, at)                   # |err| <= noise = floor / 16, before the rtol term helps
        assert c.floor(k) >= 16 * 2.0 ** -23 * np.abs(c.g64[k]).max()
    # and under the family's existing whole-tensor rule both the reference and the oracle pass, as the golden tests say
    assert GC.maxnorm_failures(c, c.g64) == []


@pytest.mark.parametrize("family,name", CASES, ids=IDS)
def test_the_gpu_tests_comparison_on_stand_ins_for_the_kernels_gradients(family, name):
    """tests/grad_cases.py::check is what tests/test_grad_elementwise_gpu.py asserts with.  The reference's fp32 gradients, flat as
    the kernels hand them over, pass; the same with the smaller half of one tensor lost fail, naming the tensor; a missing tensor or
    a wrong size is an error."""
    c = GC.case(family, name)
    ref = {k: (c.ref32[k] if c.ref32[k] is not None else np.zeros(c.g64[k].shape, np.float32)).reshape(-1) for k in c.g64}
    lines, bad = GC.check(c, ref, name)
    assert bad == [] and len(lines) == len(c.live)
    def stands(n):          # how far the largest element of tensor n's smaller half stands above what the gate allows it
        v = np.sort(np.abs(c.g64[n]).reshape(-1))[max(c.g64[n].size // 2 - 1, 0)] if c.g64[n].size > 1 else 0.0
        return v / (c.rtol * v + c.floor(n))
    k = max(c.live, key=stands)
    assert stands(k) > 1.5
    lost = ref[k].copy()
    lost[np.argsort(np.abs(lost))[:lost.size // 2]] = 0.0
    lines, bad = GC.check(c, {**ref, k: lost}, name)
    assert len(bad) == 1 and bad[0].startswith(f"{name} {k} at "), (k, bad)
    assert GC.maxnorm_failures(c, {**{n: c.ref32[n] for n in c.live}, k: lost.reshape(c.g64[k].shape)}) in ([], [k])
    with pytest.raises(AssertionError):
        GC.check(c, {n: v for n, v in ref.items() if n != k}, name)
    with pytest.raises(AssertionError):
        GC.check(c, {**ref, k: ref[k][:-1]}, name)


# ---- 3. zero in exact arithmetic ------------------------------------------------------------------------------------------------------

# what each family's check_grads / golden test special-cases, as a rule on the name
SPECIAL = {
    "FC_STGNN": lambda k: k in ("nonlin_map2.0.bias", "MPNN1.MPNN.theta.0.bias", "MPNN2.MPNN.theta.0.bias"),   # biases before train-mode BN
    "ST_Conv": lambda k: k == "cnn_layer_1.conv.bias",                                                          # bias before train-mode BN
    "RGCNU": lambda k: k.startswith("fusion.fc2"),                                                              # the std head: not in the loss
    "STAGNN": lambda k: k.endswith(".attention.bias"),                                                          # softmax shift invariance
    "AGCN_TF": lambda k: k.endswith("W_k.bias"),                                                                # rows of a softmax gradient sum to 0
    "HAGCN": lambda k: k.endswith("rank.bias") or (k.startswith("gnn") and k.endswith("mlp.2.bias")),           # softmax shift invariance
    "STNet": lambda k: k.startswith("cnn."),                                                                    # only feeds a threshold
}
# zero on this fixture's data only (they stay under the families' whole-tensor rules, which hold them to the model's scale):
#  HAGCN gnn*.mlp.0.bias: sum over nodes of (softmax gradient) x (ReLU pattern); the fixtures' nodes are near-identical, so a hidden
#    unit is on for all nodes or for none, and the softmax gradient sums to zero over the nodes
#  STGNN gru.weight_hh_l0: one patch = one GRU step from h0 = 0
#  STNet (6 x 128): the LSTM's gates saturate on the un-normalised Chebyshev values; nothing flows through it to the head
_MLP0 = ["gnn2.mlp.0.bias", "gnn3.mlp.0.bias"]
DATA_ZERO = {
    "hagcn_fd001_5x10_bs6": ["gnn3.mlp.0.bias"], "hagcn_fd002_2x25_bs5": _MLP0, "hagcn_fd004_1x50_bs7": _MLP0,
    "hagcn_ncmapss_2x25_bs3": _MLP0, "hagcn_smalllstm_3x6_bs4": _MLP0,
    "stgnn_cmapss_1x50_bs9": ["gru.weight_hh_l0"],
    "stnet_phm_c1like_6x128_bs5": ["encoder.0.bias", "linear.weight", "lstm.bias_hh_l0", "lstm.bias_ih_l0", "lstm.weight_hh_l0", "lstm.weight_ih_l0"],
}


@pytest.mark.parametrize("family,name", CASES, ids=IDS)
def test_detected_zero_tensors_are_the_ones_the_family_special_cases(family, name):
    c = GC.case(family, name)
    want = sorted([k for k in c.g64 if SPECIAL.get(family, lambda k: False)(k)] + DATA_ZERO.get(name, []))
    assert c.zero == want
    assert sorted(c.live + c.zero) == sorted(c.g64) and all(c.ref32[k] is not None for k in c.live)


# ---- 4. the recorded noise --------------------------------------------------------------------------------------------------------------

def _maker():
    spec = importlib.util.spec_from_file_location("make_grad_noise", os.path.join(GC.GOLDEN, "make_grad_noise.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GC.GOLDEN, "grad_noise.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("family,name", CASES, ids=IDS)
def test_recorded_noise_is_reproduced(family, name, recorded):
    c = GC.case(family, name)
    nz, sh = _maker().measure(c)
    rn, rs = recorded["noise_over_max"][family][name], recorded["share_below_1e-3_of_max"][family][name]
    assert sorted(rn) == sorted(rs) == sorted(c.live)
    for k in c.live:
        assert abs(nz[k] - rn[k]) <= 1e-2 * rn[k] + 1e-30, (k, nz[k], rn[k])
        assert abs(sh[k] - rs[k]) <= 1e-2 * rs[k] + 0.5 / c.g64[k].size, (k, sh[k], rs[k])


def test_recorded_tables_hold_exactly_the_cases(recorded):
    for t in ("noise_over_max", "share_below_1e-3_of_max"):
        assert sorted((f, n) for f, fx in recorded[t].items() for n in fx) == sorted(CASES)


def test_the_blind_share_and_the_reference_noise_are_what_the_gate_was_sized_for(recorded):
    """The figures the gate rests on, read off the record: most of a tensor lies below the old gates in most families, and the
    reference's fp32 noise lies two to three decades below them."""
    # (over the fixtures the gate was sized on: a sum over thousands of samples gives the reference's fp32 autograd more noise than the
    #  figures below -- tests/golden/make_golden_wrap.py; each wrap tensor's floor comes from its own entry like every other's)
    recorded = {t: {f: {n: d for n, d in fx.items() if "_wrap_" not in n} for f, fx in recorded[t].items()} for t in recorded}
    share = {f: max(v for d in fx.values() for v in d.values()) for f, fx in recorded["share_below_1e-3_of_max"].items()}
    assert share["STMSGCN"] > 0.9 and share["RGCNU"] > 0.6 and share["ST_GCN"] > 0.5 and share["STAGNN"] >= 0.5
    assert share["ASTGCNN"] < 0.1 and share["ST_Conv"] < 0.06
    for fam, fx in recorded["noise_over_max"].items():
        allv = [v for d in fx.values() for v in d.values()]
        if fam != "HAGCN":                       # HAGCN: alpha = 100 x a KL term of near-equal distributions, gradients that cancel
            assert np.median(allv) < 2e-6 and max(allv) < 1.1e-4, fam
        assert min(allv) >= 0.0
