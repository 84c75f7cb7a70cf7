"""LOGO_bearing without a GPU: the registry and the scheduler, the module's surface, the six hparams rows, parameter counts, the seed, the
C-ABI's size queries, the coverage gate at every limit, the consistency refusals and the backward's LDS plan."""
import ctypes as C
import glob
import os

import numpy as np
import pytest
import torch

from gnn_rul_benchmarking_amd import _lib

from conftest import GOLDEN

import family_kit as K
import logo_bearing_oracle as O
from test_logo_bearing_oracle_golden import CURVE, FULL, SMALL, load_case

FIELDS = O.KEYS
PHM = dict(patch_size=64, num_patch=40, input_dim=9, num_nodes=5, nperseg=8, hidden_dim=10)
XJTU = dict(patch_size=1024, num_patch=32, input_dim=33, num_nodes=17, nperseg=32, hidden_dim=10)
RULGNN_EINVAL, RULGNN_EUNSUPPORTED = -1, -2                # include/rulgnn.h
LDS_BUDGET = 160 * 1024                                    # csrc/launch.hpp MAX_LDS_BYTES


def shape_of(batch, cfg):
    return _lib.LogobShape(batch, *[cfg[k] for k in FIELDS])


def cfg_of(P=8, T=1, ns=4, h=1, **over):
    return dict(dict(patch_size=P, num_patch=T, input_dim=1 + P // ns if ns else 0, num_nodes=ns // 2 + 1, nperseg=ns, hidden_dim=h), **over)


def test_registry_algorithm_scheduler_and_data_parallel_refusal():
    from gnn_rul_benchmarking_amd import algorithms as A
    from gnn_rul_benchmarking_amd.hparams import get_hparams_class
    from gnn_rul_benchmarking_amd.logo_bearing import LOGO_bearing_model
    from gnn_rul_benchmarking_amd.optim import FusedAdam
    # the class is there; the registry does not serve it yet: tests/test_logo_cpu.py holds get_algorithm_class("LOGO_bearing") to its refusal
    assert issubclass(A.LOGO_bearing, A.LOGO) and A.LOGO_bearing.model_class is LOGO_bearing_model
    for name in ("LOGO_bearing", "LOGO_bearing_model"):
        with pytest.raises(NotImplementedError, match="Algorithm not found: " + name):
            A.get_algorithm_class(name)
    with pytest.raises(NotImplementedError, match="Algorithm not found: HierCorrPool_bearing"):
        A.get_algorithm_class("HierCorrPool_bearing")
    assert A.LOGO_bearing.needs_train_mode == "dropout" and A.LOGO_bearing.supports_graphs is False
    h = get_hparams_class("PHM2012")("Condition_2")
    algo = A.LOGO_bearing(h.alg_hparams["LOGO_bearing"], h.train_params["LOGO_bearing"], "cpu")
    assert isinstance(algo.model, LOGO_bearing_model) and isinstance(algo.optimizer, FusedAdam)
    assert algo.theta == 0.001 and algo.model.c_family == "logob" and algo.model.dropout_p == 0.2
    assert algo.model.eval_sample_independent is False
    s = algo.lr_schedular                                            # the reference's spelling
    assert isinstance(s, torch.optim.lr_scheduler.MultiStepLR) and s.optimizer is algo.optimizer
    assert sorted(s.milestones.elements()) == [5, 10, 20, 25] and s.gamma == 0.5
    lrs = []
    for _ in range(26):                                              # what update() does behind every step
        algo._step_scheduler()
        lrs.append(algo.optimizer.param_groups[0]["lr"])
    assert lrs[3] == 1e-3 and lrs[4] == 5e-4 and lrs[9] == 2.5e-4 and lrs[19] == 1.25e-4 and lrs[24] == lrs[25] == 6.25e-5
    with pytest.raises(RuntimeError, match="LOGO is not sample-shardable"):
        algo.attach_data_parallel(object())
    algo.eval()
    with pytest.raises(RuntimeError, match="needs algorithm.train"):
        algo.update(torch.zeros(2, 2560), torch.zeros(2, 1))
    assert algo.optimizer.param_groups[0]["lr"] == 6.25e-5           # a refused update steps nothing


def test_hparams_rows_equal_the_reference():
    from gnn_rul_benchmarking_amd import algorithms as A
    train = {"num_epochs": 81, "batch_size": 100, "weight_decay": 1e-4, "learning_rate": 1e-3, "theta": 0.001}
    keys = [f"{ds}/Condition_{i}" for ds in ("PHM2012", "XJTU_SY") for i in (1, 2, 3)]
    rows = K.hparams_rows_check("LOGO_bearing", "logob_hparams_rows.npz", {k: (train, PHM if k.startswith("PHM2012") else XJTU) for k in keys},
                                ["CMAPSS/FD001"])
    for key, ref in rows.items():
        algo = A.LOGO_bearing(ref["alg_hparams"], ref["train_params"], "cpu")
        assert algo.model.num_live == (177434 if key.startswith("PHM2012") else 369674)


@pytest.mark.parametrize("cfg,count", [(PHM, 177434), (XJTU, 369674)], ids=["PHM2012", "XJTU_SY"])
def test_param_counts_and_shapes_of_the_two_geometries(cfg, count):
    from gnn_rul_benchmarking_amd.logo_bearing import LOGO_bearing_model
    m = LOGO_bearing_model(**cfg)
    assert sum(p.numel() for p in m.parameters()) == count == O.param_count(cfg) == m.num_live
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == O.param_shapes(cfg) and len(m.state_dict()) == 46
    lib = _lib.load()
    for B in (1, 100, 1024):                                         # the batches the limits must admit
        s = shape_of(B, cfg)
        assert lib.rulgnn_logob_param_count(C.byref(s)) == count and lib.rulgnn_logob_workspace_bytes(C.byref(s)) > 0
    T, N, f, h = cfg["num_patch"], cfg["num_nodes"], cfg["input_dim"], cfg["hidden_dim"]
    s = shape_of(7, cfg)
    hg, td, gl = (lib.rulgnn_logob_tap_offset(C.byref(s), i) for i in range(3))
    al = lambda floats: (floats + 63) // 64 * 64      # noqa: E731
    assert lib.rulgnn_logob_tap_offset(C.byref(s), 3) == -1
    # between x and the LSTM's input the workspace holds Hg alone: no spectrogram, no [B T, N, N] tensor
    assert td - hg == al(T * N * 7 * 3 * f) + 2 * al(T * N * 7 * 3 * h) + al(T * N * 7 * 6 * h) and gl > td


@pytest.mark.parametrize("name", SMALL + [CURVE])
def test_a_seed_gives_the_reference_keys_and_initial_values(name):
    """The 46 keys, their order, strict load and -- under the fixture's seed, minus the maker's recorded perturbation -- the reference's
    initial values bit for bit (what lets the full-width fixtures store a seed in place of their weights)."""
    from gnn_rul_benchmarking_amd.logo_bearing import LOGO_bearing_model
    pre = "sd0:" if name == CURVE else "sd:"
    z, cfg, stored = load_case(name, pre)
    seed = int(z["seed"])
    torch.manual_seed(seed)
    m = LOGO_bearing_model(**cfg)
    sd = m.state_dict()
    assert list(sd.keys()) == list(stored) == O.state_keys() and len(sd) == 46
    assert [n for n, _ in m.named_parameters()] == O.param_names()
    assert np.array_equal(m.flat_params.numpy(), np.concatenate([sd[k].numpy().ravel() for k in O.param_names()]))
    g = torch.Generator().manual_seed(seed + 1000)                  # the maker's p.add_(uniform(-0.1, 0.1))
    for k, v in sd.items():
        want = v.clone().add_(torch.empty_like(v).uniform_(-0.1, 0.1, generator=g))
        assert v.shape == stored[k].shape and np.array_equal(want.numpy(), stored[k]), k
    other = LOGO_bearing_model(**cfg)
    other.load_state_dict({k: torch.from_numpy(stored[k]) for k in sd}, strict=True)
    with pytest.raises(RuntimeError):
        other.load_state_dict({k: torch.from_numpy(stored[k]) for k in list(sd)[1:]}, strict=True)


def test_limits_header_and_logo_limits_untouched():
    from gnn_rul_benchmarking_amd import logo, logo_bearing
    assert logo_bearing.LIMITS == {"max_nodes": 17, "max_input_dim": 33, "max_sequences": 65535, "max_lstm_width": 128}
    assert logo.LIMITS == {"max_nodes": 32, "max_patch_size": 16, "max_sequences": 65535, "max_lstm_width": 128}
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "rulgnn.h")).read()
    for name, key in (("NODES", "max_nodes"), ("INPUT_DIM", "max_input_dim"), ("SEQUENCES", "max_sequences"), ("LSTM_WIDTH", "max_lstm_width")):
        assert f"#define RULGNN_LOGOB_MAX_{name} {logo_bearing.LIMITS[key]}\n" in header
    for name, key in (("NODES", "max_nodes"), ("PATCH_SIZE", "max_patch_size"), ("SEQUENCES", "max_sequences"), ("LSTM_WIDTH", "max_lstm_width")):
        assert f"#define RULGNN_LOGO_MAX_{name} {logo.LIMITS[key]}\n" in header
    m = logo_bearing.LOGO_bearing_model(**PHM)
    assert "do not cover this configuration" in m.not_covered and "input_dim = 1 + patch_size // nperseg <= 33" in m.not_covered
    # the smallest limits that admit both reference geometries: XJTU_SY sits on both
    assert XJTU["num_nodes"] == 17 and XJTU["input_dim"] == 33


def test_struct_sizes_are_checked_at_load():
    lib = _lib.load()
    assert _lib.STRUCTS[41] is _lib.LogobShape
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "rulgnn.h")).read()
    assert "#define RULGNN_STRUCT_LOGOB_SHAPE 41\n" in header
    assert lib.rulgnn_struct_size(41) == C.sizeof(_lib.LogobShape) == 32
    assert _lib.STRUCTS[32] is _lib.LogoArgs and lib.rulgnn_struct_size(32) == C.sizeof(_lib.LogoArgs)      # the argument struct is LOGO's


def lds_floats(N, T, f, bwd, ns=0, P=0, logo_layout=False):
    """csrc/logo.hip LgLds, restated.  ``logo_layout``: the whole partial row in LDS, as LOGO keeps it."""
    L, NN, NE = T * f, N * (N + 1), N * (2 * f + 1)
    o = N * (L + 1) + 2 * N + 4 * NN + 2 * NE + 5 * NN + 2 * 256
    if bwd:
        CW = 2 * f * f + 2 * f + 6 * f * f + 3 * f + 6 * (N * N + N)
        o += 9 * NN + N * (3 * f + 1) + 2 * NE + (CW if logo_layout else CW - 8 * f * f)
    return o + (P + 4 * ns if ns else 0)


def test_backward_lds_plan_fits_both_geometries_where_logos_layout_would_not():
    for cfg in (PHM, XJTU):
        T, N, f, ns, P = cfg["num_patch"], cfg["num_nodes"], cfg["input_dim"], cfg["nperseg"], cfg["patch_size"]
        assert 4 * lds_floats(N, T, f, True, ns, P) <= LDS_BUDGET and 4 * lds_floats(N, T, f, False, ns, P) <= LDS_BUDGET
    T, N, f, ns, P = (XJTU[k] for k in ("num_patch", "num_nodes", "input_dim", "nperseg", "patch_size"))
    assert lds_floats(N, T, f, True, logo_layout=True) == 40992                      # 163 968 B before the STFT's staging area
    assert 4 * lds_floats(N, T, f, True, logo_layout=True) > LDS_BUDGET
    assert lds_floats(N, T, f, True, ns, P) == 40992 - 8 * 33 * 33 + 1024 + 4 * 32 == 33432      # 133 728 B
    # the register plan: element i of Theta's / W_n's gradient lives in slot i // 256 of thread i % 256
    assert -(-6 * 33 * 33 // 256) == 26 and -(-2 * 33 * 33 // 256) == 9


def test_coverage_gate_every_limit_plus_and_minus_one():
    lib = _lib.load()

    def query(cfg, B=3, code=RULGNN_EUNSUPPORTED):
        s = shape_of(B, cfg)
        pc, ws = lib.rulgnn_logob_param_count(C.byref(s)), lib.rulgnn_logob_workspace_bytes(C.byref(s))
        assert (pc == -1) == (ws == 0) and (pc < 0) == (ws == 0) and (lib.rulgnn_logob_tap_offset(C.byref(s), 1) < 0) == (ws == 0)
        if ws == 0:                    # refused by the entries too, before any launch (no device is needed to be told so)
            a = _lib.LogoArgs()
            rcs = {lib.rulgnn_logob_forward_f32(C.byref(s), C.byref(a), None), lib.rulgnn_logob_backward_f32(C.byref(s), C.byref(a), None),
                   lib.rulgnn_logob_fwdbwd_f32(C.byref(s), C.byref(a), None, None)}
            assert rcs == {code}, (cfg, rcs)
        return ws > 0

    assert query(cfg_of(P=2, T=1, ns=2, h=1))                                # every lower limit at once: nperseg 2, N 2, P 2, T 1, h 1
    assert not query(cfg_of(P=1, ns=2)) and query(cfg_of(P=3, ns=4)) and not query(cfg_of(P=2, ns=4))       # patch_size > nperseg / 2
    assert not query(cfg_of(ns=0), code=RULGNN_EUNSUPPORTED) and not query(cfg_of(ns=3, num_nodes=2, input_dim=3)) and not query(cfg_of(ns=5))
    assert not query(cfg_of(T=0)) and not query(cfg_of(h=0))
    assert not query(cfg_of(T=-1), code=RULGNN_EINVAL)
    assert query(cfg_of(P=64, ns=32)) and not query(cfg_of(P=64, ns=34))     # N = 17 / 18
    assert query(cfg_of(P=65, ns=2)) and not query(cfg_of(P=66, ns=2))       # f = 33 / 34
    assert query(cfg_of(h=21)) and not query(cfg_of(h=22))                   # 6 h = 126 / 132 against 128
    # the LDS backstop binds before N T <= 65 535 does: the longest window at XJTU_SY's shape of patch
    t_max = max(t for t in range(32, 80) if 4 * lds_floats(17, t, 33, True, 32, 1024) <= LDS_BUDGET)
    assert t_max == 45 and query(dict(XJTU, num_patch=t_max)) and not query(dict(XJTU, num_patch=t_max + 1))
    t_max = max(t for t in range(9000, 11000) if 4 * lds_floats(2, t, 2, True, 2, 2) <= LDS_BUDGET)
    assert 2 * t_max < 65535 and query(cfg_of(P=2, T=t_max, ns=2)) and not query(cfg_of(P=2, T=t_max + 1, ns=2))
    ws = lambda b: lib.rulgnn_logob_workspace_bytes(C.byref(shape_of(b, PHM)))      # noqa: E731
    assert ws(0) > 0 and ws(1024) > ws(100) > ws(1) >= ws(0) and ws(-1) == 0


def test_kwargs_that_do_not_describe_the_stft_construct_and_are_refused():
    """The reference constructs such a model and fails with a shape error inside its first forward."""
    from gnn_rul_benchmarking_amd.logo_bearing import LOGO_bearing_model
    lib = _lib.load()
    for bad in (dict(num_nodes=4), dict(input_dim=2), dict(num_nodes=2, input_dim=4)):
        cfg = cfg_of(P=8, T=2, ns=4, **bad)
        s = shape_of(2, cfg)
        assert lib.rulgnn_logob_param_count(C.byref(s)) == -1 and lib.rulgnn_logob_workspace_bytes(C.byref(s)) == 0
        a = _lib.LogoArgs()
        assert lib.rulgnn_logob_forward_f32(C.byref(s), C.byref(a), None) == RULGNN_EINVAL
        assert lib.rulgnn_logob_fwdbwd_f32(C.byref(s), C.byref(a), None, None) == RULGNN_EINVAL
        m = LOGO_bearing_model(**cfg)
        assert len(m.state_dict()) == 46


def test_cpu_input_raises():
    from gnn_rul_benchmarking_amd.logo_bearing import LOGO_bearing_model
    m = LOGO_bearing_model(**cfg_of(P=8, T=2, ns=4))
    K.cpu_input_raises(m, torch.zeros(2, 16))
    for x in (torch.zeros(2, 2, 8), torch.zeros(2, 1, 16)):
        with pytest.raises(RuntimeError, match="HIP path only"):
            m(x)
    with pytest.raises(RuntimeError, match="HIP path only"):
        m(torch.zeros(2, 16), GL=True)


def test_fixtures_hold_no_grad_key_and_stay_under_the_size_limit():
    """tests/test_grad_gate_cpu.py globs every fixture for ``grad:`` keys: this family's reference gradients are ``refgrad:``."""
    files = sorted(glob.glob(os.path.join(GOLDEN, "logob_*.npz")))
    assert len(files) == 11
    for f in files:
        assert not [k for k in np.load(f).files if k.startswith("grad:")], f
        assert os.path.getsize(f) < 1 << 20, f
    for name in SMALL + FULL:
        z = load_case(name)[0]
        assert sorted(k[8:] for k in z if k.startswith("refgrad:")) == sorted(O.param_names())
        assert {"x", "y", "pred", "pred_eval", "loss_gl", "loss", "mpnn", "lstm", "spec", "seed"} <= set(z)
        assert bool([k for k in z if k.startswith("sd:")]) == (name in SMALL)
