"""LOGO without a GPU: the registry, the module's surface, the hparams rows, the parameter counts of the five wirings, the C-ABI's size
queries, the coverage gate at every limit and the workspace layout (no [B T, N, N] tensor)."""
import ctypes as C
import glob
import os

import numpy as np
import pytest
import torch

from gnn_rul_benchmarking_amd import _lib

from conftest import GOLDEN

import family_kit as K
import logo_oracle as O

FIELDS = O.KEYS
FIXTURES = ["logo_small_3x2x2_h1_bs4", "logo_fd001geom_bs5", "logo_fd002geom_bs4", "logo_ncmapssgeom_bs3"]
FD001 = dict(patch_size=10, num_patch=5, num_nodes=14, hidden_dim=8)
FD002 = dict(patch_size=2, num_patch=25, num_nodes=14, hidden_dim=6)
FD003 = dict(patch_size=10, num_patch=5, num_nodes=14, hidden_dim=32)
FD004 = dict(patch_size=10, num_patch=5, num_nodes=14, hidden_dim=10)
NCMAPSS = dict(patch_size=5, num_patch=10, num_nodes=20, hidden_dim=10)
RULGNN_EUNSUPPORTED = -2                # include/rulgnn.h


def shape_of(batch, cfg):
    return _lib.LogoShape(batch, *[cfg[k] for k in FIELDS])


def test_registry_serves_the_algorithm_and_refuses_the_model():
    from gnn_rul_benchmarking_amd import algorithms as A
    K.registry_check("LOGO")
    with pytest.raises(NotImplementedError, match="Algorithm not found: LOGO_bearing"):
        A.get_algorithm_class("LOGO_bearing")


def test_algorithm_construction_theta_and_data_parallel_refusal():
    from gnn_rul_benchmarking_amd import algorithms as A
    from gnn_rul_benchmarking_amd.logo import LOGO_model
    from gnn_rul_benchmarking_amd.hparams import get_hparams_class
    from gnn_rul_benchmarking_amd.optim import FusedAdam
    h = get_hparams_class("CMAPSS")("FD002")
    algo = A.get_algorithm_class("LOGO")(h.alg_hparams["LOGO"], h.train_params["LOGO"], "cpu")
    assert isinstance(algo.model, LOGO_model) and isinstance(algo.optimizer, FusedAdam)
    assert algo.hparams == h.train_params["LOGO"] and algo.theta == 0.01 and algo.model.c_family == "logo" and algo.model.dropout_p == 0.2
    assert not hasattr(algo, "lr_schedular")                         # the reference never steps it: none is built
    assert algo.model.eval_sample_independent is False
    assert sum(p.numel() for p in algo.model.parameters()) == _lib.load().rulgnn_logo_param_count(C.byref(shape_of(100, FD002)))
    with pytest.raises(RuntimeError, match="LOGO is not sample-shardable"):
        algo.attach_data_parallel(object())
    algo.eval()
    with pytest.raises(RuntimeError, match="needs algorithm.train"):
        algo.update(torch.zeros(2, 14, 50), torch.zeros(2, 1))


@pytest.mark.parametrize("name", FIXTURES + ["logo_train_curve_3x2x2_h1_bs8"])
def test_a_seed_gives_the_reference_keys_and_initial_values(name):
    """The 46 keys, their order, strict load and -- under the fixture's seed, minus the maker's recorded perturbation -- the reference's
    initial values bit for bit."""
    from gnn_rul_benchmarking_amd.logo import LOGO_model
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    pre = "sd0:" if "curve" in name else "sd:"
    cfg = {k[4:]: int(z[k]) for k in z.files if k.startswith("cfg:")}
    seed = int(z["seed"])
    torch.manual_seed(seed)
    m = LOGO_model(**cfg)
    sd = m.state_dict()
    assert list(sd.keys()) == [k[len(pre):] for k in z.files if k.startswith(pre)] == O.state_keys() and len(sd) == 46
    assert [n for n, _ in m.named_parameters()] == O.param_names() and len(O.param_names()) == 46
    assert np.array_equal(m.flat_params.numpy(), np.concatenate([sd[k].numpy().ravel() for k in O.param_names()]))
    g = torch.Generator().manual_seed(seed + 1000)                  # tests/golden/make_golden_logo.py: p.add_(uniform(-0.1, 0.1))
    for k, v in sd.items():
        want = v.clone().add_(torch.empty_like(v).uniform_(-0.1, 0.1, generator=g))
        assert v.shape == z[pre + k].shape and np.array_equal(want.numpy(), z[pre + k]), k
    other = LOGO_model(**cfg)
    other.load_state_dict({k: torch.from_numpy(z[pre + k]) for k in sd}, strict=True)
    assert np.array_equal(other.state_dict()["cls.weight"].numpy(), z[pre + "cls.weight"])


def test_hparams_rows_equal_the_reference():
    from gnn_rul_benchmarking_amd.hparams import get_hparams_class
    rows = K.hparams_rows_check("LOGO", "logo_hparams_rows.npz", ["CMAPSS/FD001", "CMAPSS/FD002", "CMAPSS/FD003", "CMAPSS/FD004", "NCMAPSS/None"],
                                ["PHM2012/Condition_1"])
    assert [rows[k]["train_params"]["theta"] for k in sorted(rows)] == [0.001, 0.01, 0.01, 0.001, 0.001]
    n = get_hparams_class("NCMAPSS")(None).train_params["LOGO"]
    assert n["batch_size"] == 50 and n["weight_decay"] == 0
    for did, cfg in (("FD001", FD001), ("FD002", FD002), ("FD003", FD003), ("FD004", FD004)):
        assert get_hparams_class("CMAPSS")(did).alg_hparams["LOGO"] == cfg
    assert get_hparams_class("NCMAPSS")(None).alg_hparams["LOGO"] == NCMAPSS


@pytest.mark.parametrize("cfg,count", [(FD001, 82527), (FD002, 130199), (FD003, 876255), (FD004, 116991), (NCMAPSS, 176426)],
                         ids=["FD001", "FD002", "FD003", "FD004", "NCMAPSS"])
def test_param_counts_of_the_five_wirings(cfg, count):
    from gnn_rul_benchmarking_amd.logo import LOGO_model
    m = LOGO_model(**cfg)                                            # FD003 constructs too
    assert sum(p.numel() for p in m.parameters()) == count == O.param_count(cfg) == m.num_live
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == O.param_shapes(cfg)
    got = _lib.load().rulgnn_logo_param_count(C.byref(shape_of(7, cfg)))
    assert got == (count if cfg is not FD003 else -1)


def test_fd003_constructs_and_is_refused_with_the_workspace_query_at_zero():
    """hidden_dim 32: the middle LSTM is 192 wide, beyond the persistent LSTM's 128."""
    from gnn_rul_benchmarking_amd.logo import LOGO_model, LIMITS
    lib = _lib.load()
    s = shape_of(100, FD003)
    assert lib.rulgnn_logo_workspace_bytes(C.byref(s)) == 0 and lib.rulgnn_logo_param_count(C.byref(s)) < 0
    a = _lib.LogoArgs()
    assert lib.rulgnn_logo_forward_f32(C.byref(s), C.byref(a), None) == RULGNN_EUNSUPPORTED
    m = LOGO_model(**FD003)
    assert "do not cover this configuration" in m.not_covered and "6 * hidden_dim <= 128" in m.not_covered
    assert LIMITS == {"max_nodes": 32, "max_patch_size": 16, "max_sequences": 65535, "max_lstm_width": 128}
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "rulgnn.h")).read()
    for name, key in (("NODES", "max_nodes"), ("PATCH_SIZE", "max_patch_size"), ("SEQUENCES", "max_sequences"), ("LSTM_WIDTH", "max_lstm_width")):
        assert f"#define RULGNN_LOGO_MAX_{name} {LIMITS[key]}\n" in header
    for cfg in (FD001, FD002, FD004, NCMAPSS):                       # the rows the limits must admit, at their batch and at 1024
        for B in (1, 50, 100, 1024):
            assert lib.rulgnn_logo_workspace_bytes(C.byref(shape_of(B, cfg))) > 0


def test_cpu_input_raises():
    from gnn_rul_benchmarking_amd.logo import LOGO_model
    m = LOGO_model(2, 2, 3, 1)
    K.cpu_input_raises(m, torch.zeros(2, 3, 4))
    with pytest.raises(RuntimeError, match="HIP path only"):
        m(torch.zeros(2, 3, 4), GL=True)


def test_new_fixtures_hold_no_grad_key():
    """tests/test_grad_gate_cpu.py globs every fixture for ``grad:`` keys: this family's reference gradients are ``refgrad:``."""
    files = sorted(glob.glob(os.path.join(GOLDEN, "logo_*.npz")))
    assert len(files) == 7
    for f in files:
        keys = np.load(f).files
        assert not [k for k in keys if k.startswith("grad:")], f
    for name in FIXTURES:
        keys = np.load(os.path.join(GOLDEN, name + ".npz")).files
        assert sorted(k[8:] for k in keys if k.startswith("refgrad:")) == sorted(O.param_names())
        assert {"x", "y", "pred", "pred_eval", "loss_gl", "loss", "mpnn", "lstm"} <= set(keys)


def test_struct_sizes_are_checked_at_load():
    lib = _lib.load()
    assert _lib.STRUCTS[31] is _lib.LogoShape and _lib.STRUCTS[32] is _lib.LogoArgs
    assert lib.rulgnn_struct_size(31) == C.sizeof(_lib.LogoShape) == 24
    assert lib.rulgnn_struct_size(32) == C.sizeof(_lib.LogoArgs)


def lds_floats(N, L, p, bwd):
    """csrc/logo.hip LgLds, restated."""
    NN, NE = N * (N + 1), N * (2 * p + 1)
    o = N * (L + 1) + 2 * N + 4 * NN + 2 * NE + 5 * NN + 2 * 256
    if bwd:
        CW = 2 * p * p + 2 * p + 6 * p * p + 3 * p + 6 * (N * N + N)
        o += 9 * NN + N * (3 * p + 1) + 2 * NE + CW
    return o


def test_coverage_gate_every_limit_plus_and_minus_one():
    lib = _lib.load()

    def query(cfg, B=3):
        s = shape_of(B, cfg)
        pc, ws = lib.rulgnn_logo_param_count(C.byref(s)), lib.rulgnn_logo_workspace_bytes(C.byref(s))
        assert (pc < 0) == (ws == 0) and (lib.rulgnn_logo_tap_offset(C.byref(s), 1) < 0) == (ws == 0)
        if ws == 0:                    # refused by the entries too, before any launch (no device is needed to be told so)
            a = _lib.LogoArgs()
            rcs = {lib.rulgnn_logo_forward_f32(C.byref(s), C.byref(a), None), lib.rulgnn_logo_backward_f32(C.byref(s), C.byref(a), None),
                   lib.rulgnn_logo_fwdbwd_f32(C.byref(s), C.byref(a), None, None)}
            assert rcs == {RULGNN_EUNSUPPORTED}
        return ws > 0

    def cfg(p=1, T=1, N=2, h=1):
        return dict(patch_size=p, num_patch=T, num_nodes=N, hidden_dim=h)

    assert query(cfg())                                                     # every lower limit at once: N 2, p 1, T 1, h 1
    assert not query(cfg(N=1)) and not query(cfg(p=0)) and not query(cfg(T=0)) and not query(cfg(h=0))
    assert query(cfg(N=32)) and not query(cfg(N=33))
    assert query(cfg(p=16)) and not query(cfg(p=17))
    assert query(cfg(h=21)) and not query(cfg(h=22))                        # 6 h = 126 / 132 against 128
    # the LDS backstop.  A sample's whole window sits in LDS, so the longest window is the one that fills it: at N = 2, p = 1 that is
    # T = 20 161 patches (N T = 40 322), which is why N T <= 65 535 (the persistent LSTM's sequence count) is never the binding limit
    t_max = max(t for t in range(20000, 20400) if 4 * lds_floats(2, t, 1, True) <= 160 * 1024)
    assert 2 * t_max < 65535 and query(cfg(T=t_max)) and not query(cfg(T=t_max + 1))
    assert not query(cfg(N=5, T=13107)) and not query(cfg(N=5, T=13108))    # N T = 65 535 / 65 540: both beyond the LDS
    # N = 32 and p = 16 together leave room for a window of 13 patches (the backward's layout is the larger)
    assert 4 * lds_floats(32, 13 * 16, 16, True) <= 160 * 1024 < 4 * lds_floats(32, 14 * 16, 16, True)
    assert 4 * lds_floats(32, 14 * 16, 16, False) <= 160 * 1024
    assert query(cfg(N=32, p=16, T=13)) and not query(cfg(N=32, p=16, T=14))
    assert query(cfg(N=32, p=16, T=5, h=21))                                # what the GPU test runs just inside
    ws = lambda b: lib.rulgnn_logo_workspace_bytes(C.byref(shape_of(b, FD001)))      # noqa: E731
    assert ws(0) > 0 and ws(1024) > ws(100) > ws(1) >= ws(0) and ws(-1) == 0


def test_workspace_holds_no_per_graph_matrix():
    """Between x and the LSTM's input the workspace holds Hg [T N][B][3p] and, per sample, two loss sums: no [B T, N, N] tensor (A_T,
    A_G, z, r, A^, C) and no [B T, N, 2p] one (E, C E) -- those live in LDS (csrc/logo.hip: LgLds).  The backward's partial rows are
    per workgroup (at most 256), not per graph."""
    lib = _lib.load()
    al = lambda floats: (floats + 63) // 64 * 64      # noqa: E731
    for cfg in (FD001, FD002, FD004, NCMAPSS):
        p, T, N, h = (cfg[k] for k in FIELDS)
        Q = T * N
        for B in (1, 100, 1024):
            s = shape_of(B, cfg)
            hg, td, gl = (lib.rulgnn_logo_tap_offset(C.byref(s), i) for i in range(3))
            assert lib.rulgnn_logo_tap_offset(C.byref(s), 3) == -1
            o1 = hg + al(Q * B * 3 * p)
            assert td - o1 == 2 * al(Q * B * 3 * h) + al(Q * B * 6 * h)      # the three LSTM outputs follow Hg directly
            # everything of the step that is not an LSTM tape, an LSTM-width activation or its gradient
            total = lib.rulgnn_logo_workspace_bytes(C.byref(s)) // 4
            lstm = sum(lib.rulgnn_bilstm_workspace_bytes(C.byref(_lib.BilstmShape(B, Q, I, H))) // 4
                       for I, H in ((3 * p, 3 * h), (3 * h, 6 * h), (6 * h, 3 * h)))
            acts = 2 * (al(Q * B * 3 * p) + 2 * al(Q * B * 3 * h) + al(Q * B * 6 * h) + al(B * Q * 3 * h))
            CW = 2 * p * p + 2 * p + 6 * p * p + 3 * p + 6 * (N * N + N)
            split = max(1024, lib.rulgnn_sgemm_splitk_workspace_bytes(B, 16, Q * 3 * h) // 4)      # bounds fc1's fixed-slice partials
            rest = total - lstm - acts - al(min(B, 256) * CW)
            # what is left: fc1's partials, the head's per-sample rows (16 + 8 + 161 + 16), the loss terms and two loss sums per sample
            assert 0 < rest <= B * 206 + 11 * 64 + al(split), (cfg, B, rest)
            if B >= 100:
                assert rest < B * T * N * N, "a [B T, N, N] tensor would not fit here"
