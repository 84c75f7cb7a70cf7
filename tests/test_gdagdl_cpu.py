"""GDAGDL without a GPU: the registry, the module's surface (36 names in order, a seed gives the reference's initial weights, strict
load, the two gradless tensors first in the flat layout), the hparams rows, the C-ABI's size queries, the coverage gate at every limit
and the workspace's growth per sample."""
import ctypes as C
import glob
import json
import os

import numpy as np
import pytest
import torch

from gnn_rul_benchmarking_amd import _lib

from conftest import GOLDEN

import family_kit as K
import gdagdl_oracle as O
from test_gdagdl_oracle_golden import CURVE, FULL, SMALL, load_case

BASE = dict(gat_layer_dim=[300, 150, 50], lstm_hidden_dim=20, autoencoder_hidden_dim=256, autoencoder_out_dim=50)
PHM_C1 = dict(BASE, num_patch=128, patch_size=20, num_nodes=3, nperseg=4, input_dim=6)
PHM_C3 = dict(BASE, num_patch=80, patch_size=32, num_nodes=5, nperseg=8, input_dim=5)
XJTU = dict(BASE, num_patch=32, patch_size=1024, num_nodes=17, nperseg=32, input_dim=33)
TINY = dict(num_patch=1, patch_size=2, num_nodes=2, nperseg=2, input_dim=2, gat_layer_dim=[1], lstm_hidden_dim=1, autoencoder_hidden_dim=4,
            autoencoder_out_dim=1)
COUNTS = {128: 230347, 80: 280386, 32: 595654}
RULGNN_EUNSUPPORTED = -2                # include/rulgnn.h


def shape_of(batch, cfg):
    s = _lib.GdagdlShape()
    s.batch, s.num_patch, s.patch_size, s.num_nodes, s.nperseg, s.input_dim = batch, cfg["num_patch"], cfg["patch_size"], cfg["num_nodes"], cfg["nperseg"], cfg["input_dim"]
    s.num_gat = len(cfg["gat_layer_dim"])
    for i, c in enumerate(cfg["gat_layer_dim"][:4]):
        s.gat_layer_dim[i] = c
    s.lstm_hidden_dim, s.autoencoder_hidden_dim, s.autoencoder_out_dim = cfg["lstm_hidden_dim"], cfg["autoencoder_hidden_dim"], cfg["autoencoder_out_dim"]
    return s


def test_registry_serves_the_algorithm_and_refuses_the_model():
    K.registry_check("GDAGDL")


@pytest.mark.parametrize("ds,did,cfg", [("PHM2012", "Condition_1", PHM_C1), ("PHM2012", "Condition_3", PHM_C3), ("XJTU_SY", "Condition_2", XJTU)])
def test_algorithm_construction_from_the_rows(ds, did, cfg):
    from gnn_rul_benchmarking_amd import algorithms as A
    from gnn_rul_benchmarking_amd.gdagdl import GDAGDL_model
    from gnn_rul_benchmarking_amd.hparams import get_hparams_class
    from gnn_rul_benchmarking_amd.optim import FusedAdam
    h = get_hparams_class(ds)(did)
    assert h.alg_hparams["GDAGDL"] == cfg
    algo = A.get_algorithm_class("GDAGDL")(h.alg_hparams["GDAGDL"], h.train_params["GDAGDL"], "cpu")
    assert isinstance(algo.model, GDAGDL_model) and isinstance(algo.optimizer, FusedAdam)
    assert algo.hparams == h.train_params["GDAGDL"] and algo.model.c_family == "gdagdl" and algo.model.dropout_p == 0.5
    algo.model.dropout_p = 0.25
    assert algo.model.dropout_p == 0.25                                        # a settable attribute
    assert algo.model.dropout_by_sample_offset is True and algo.model.eval_sample_independent is True and algo.model.bucket_tail == 2
    count = COUNTS[cfg["num_patch"]]
    assert sum(p.numel() for p in algo.model.parameters()) == _lib.load().rulgnn_gdagdl_param_count(C.byref(shape_of(100, cfg))) == count
    assert O.param_count(cfg) == count and algo.model.num_live == count
    algo.eval()
    with pytest.raises(RuntimeError, match="needs algorithm.train"):
        algo.update(torch.zeros(2, cfg["num_patch"] * cfg["patch_size"]), torch.zeros(2, 1))


@pytest.mark.parametrize("name", SMALL + FULL)
def test_a_seed_gives_the_reference_keys_and_initial_values(name):
    """The names, their order, strict load and -- under the fixture's seed plus the maker's recorded perturbation -- the reference's
    values: bit for bit where the fixture stores them, by the fp64 checksum of all of them where it stores the seed alone."""
    from gnn_rul_benchmarking_amd.gdagdl import GDAGDL_model
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    cfg = json.loads(str(z["cfg_json"]))
    seed = int(z["seed"])
    torch.manual_seed(seed)
    m = GDAGDL_model(**cfg)
    sd = m.state_dict()
    names = O.param_names(cfg)
    assert list(sd.keys()) == [n for n, _ in m.named_parameters()] == names and len(names) == 36
    assert names[12:14] == list(O.GRADLESS)                   # in the middle: behind the 12 gat_layers.*, in front of encoder.*
    assert {k: tuple(v.shape) for k, v in sd.items()} == O.param_shapes(cfg) and not list(m.named_buffers())
    g = torch.Generator().manual_seed(seed + 1000)
    moved = {k: v.clone().add_(torch.empty_like(v).uniform_(-0.1, 0.1, generator=g)) for k, v in sd.items()}
    flat = np.concatenate([moved[k].numpy().astype(np.float64).ravel() for k in names])
    assert np.allclose([flat.sum(), (flat * flat).sum()], z["checksum"], rtol=1e-12, atol=0)
    if name in SMALL:
        for k in names:
            assert np.array_equal(moved[k].numpy(), z["sd:" + k]), k
        other = GDAGDL_model(**cfg)
        other.load_state_dict({k: torch.from_numpy(z["sd:" + k]) for k in names}, strict=True)
        assert np.array_equal(other.state_dict()["linear.weight"].numpy(), z["sd:linear.weight"])
        with pytest.raises(RuntimeError):
            other.load_state_dict({k: torch.from_numpy(z["sd:" + k]) for k in names[1:]}, strict=True)
    else:
        assert m.num_live == COUNTS[cfg["num_patch"]]


@pytest.mark.parametrize("cfg", [TINY, PHM_C1, XJTU])
def test_flat_order_puts_the_gradless_tensors_first(cfg):
    from gnn_rul_benchmarking_amd.gdagdl import GDAGDL_model
    torch.manual_seed(3)
    m = GDAGDL_model(**cfg)
    f = cfg["input_dim"]
    assert list(m._layout) == O.flat_names(cfg) and list(m._layout)[:2] == list(O.GRADLESS)
    assert m.gradless_params == 2 and m.optimized_range == (f + 1, m.num_live)
    assert m._layout["node_importance_linear.weight"] == (0, (1, f)) and m._layout["node_importance_linear.bias"] == (f, (1,))
    assert m._layout["gat_layers.0.linear.weight"][0] == f + 1            # the range excludes exactly the two
    sd = m.state_dict()
    assert np.array_equal(m.flat_params.numpy(), np.concatenate([sd[k].numpy().ravel() for k in O.flat_names(cfg)]))
    assert m.bucket.numel() == m.num_live + 1 and m._grad_flat.numel() == m.num_live + 2


def test_hparams_rows_equal_the_reference():
    from gnn_rul_benchmarking_amd.hparams import get_hparams_class
    absent = ["CMAPSS/FD001", "CMAPSS/FD002", "CMAPSS/FD003", "CMAPSS/FD004", "NCMAPSS/None"]
    K.hparams_rows_check("GDAGDL", "gdagdl_hparams_rows.npz", [f"{ds}/Condition_{i}" for ds in ("PHM2012", "XJTU_SY") for i in (1, 2, 3)], absent,
                         absent_is_all=True)
    assert get_hparams_class("PHM2012")("Condition_2").alg_hparams["GDAGDL"] == PHM_C1
    assert get_hparams_class("XJTU_SY")("Condition_3").train_params["GDAGDL"] == {'num_epochs': 81, 'batch_size': 100, 'weight_decay': 1e-4,
                                                                                 'learning_rate': 1e-3}


LIMIT_NAMES = (("NPERSEG", "max_nperseg"), ("FRAMES", "max_frames"), ("LAYERS", "max_layers"), ("WIDTH", "max_width"),
               ("LSTM_HIDDEN", "max_lstm_hidden"), ("AE_WIDTH", "max_ae_width"))


def test_limits_are_stated_once_and_admit_the_six_rows():
    from gnn_rul_benchmarking_amd.gdagdl import LIMITS
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "rulgnn.h")).read()
    assert len(LIMITS) == len(LIMIT_NAMES)
    for name, key in LIMIT_NAMES:
        assert f"#define RULGNN_GDAGDL_MAX_{name} {LIMITS[key]}\n" in header
    assert header.count("#define RULGNN_GDAGDL_MAX_") == len(LIMIT_NAMES)
    for cfg in (PHM_C1, PHM_C3, XJTU):
        for B in (1, 100, 1024):
            assert lib.rulgnn_gdagdl_workspace_bytes(C.byref(shape_of(B, cfg))) > 0
            assert lib.rulgnn_gdagdl_param_count(C.byref(shape_of(B, cfg))) == O.param_count(cfg)


def att_lds_floats(N, Cw, bwd):
    """csrc/gdagdl.hip gd_att_lds_floats, restated."""
    zs, nn = N * (Cw | 1), N * N
    return 2 * zs + 5 * N + 4 * nn if bwd else zs + 3 * N + nn


def test_coverage_gate_every_limit_plus_one():
    from gnn_rul_benchmarking_amd.gdagdl import LIMITS, within_limits
    lib = _lib.load()

    def query(cfg, B=3):
        s = shape_of(B, cfg)
        pc, ws = lib.rulgnn_gdagdl_param_count(C.byref(s)), lib.rulgnn_gdagdl_workspace_bytes(C.byref(s))
        assert (pc < 0) == (ws == 0) and (lib.rulgnn_gdagdl_tap_offset(C.byref(s), 1) < 0) == (ws == 0)
        inside = (within_limits(cfg["patch_size"], cfg["nperseg"], cfg["gat_layer_dim"], cfg["lstm_hidden_dim"], cfg["autoencoder_hidden_dim"],
                                cfg["autoencoder_out_dim"])
                  and cfg["num_nodes"] == cfg["nperseg"] // 2 + 1 and cfg["input_dim"] == 1 + cfg["patch_size"] // cfg["nperseg"])
        assert inside == (ws > 0)                      # the Python statement of the limits and the library's agree
        if ws == 0:                                    # refused by the entries too, before any launch (no device is needed to be told so)
            a = _lib.GdagdlArgs()
            rcs = {lib.rulgnn_gdagdl_forward_f32(C.byref(s), C.byref(a), None), lib.rulgnn_gdagdl_backward_f32(C.byref(s), C.byref(a), None),
                   lib.rulgnn_gdagdl_fwdbwd_f32(C.byref(s), C.byref(a), None, None)}
            assert rcs == {RULGNN_EUNSUPPORTED}
        return ws > 0

    def geom(nperseg, frames, **kw):
        return dict(TINY, nperseg=nperseg, num_nodes=nperseg // 2 + 1, patch_size=(frames - 1) * nperseg, input_dim=frames, **kw)

    assert query(TINY)                                                      # every lower limit at once
    assert not query(dict(TINY, gat_layer_dim=[])) and not query(dict(TINY, lstm_hidden_dim=0)) and not query(dict(TINY, autoencoder_out_dim=0))
    assert not query(dict(TINY, autoencoder_hidden_dim=3)) and not query(dict(TINY, gat_layer_dim=[0]))
    assert not query(geom(3, 3)) and not query(dict(TINY, num_nodes=3)) and not query(dict(TINY, input_dim=3))
    W, S, F = LIMITS["max_width"], LIMITS["max_nperseg"], LIMITS["max_frames"]
    top = geom(S, F, gat_layer_dim=[W] * LIMITS["max_layers"], lstm_hidden_dim=LIMITS["max_lstm_hidden"],
               autoencoder_hidden_dim=LIMITS["max_ae_width"], autoencoder_out_dim=LIMITS["max_ae_width"])
    assert query(top)                                                       # every upper limit at once: still within one CU's LDS
    assert 4 * att_lds_floats(S // 2 + 1, W, True) <= 160 * 1024 < 4 * att_lds_floats(S // 2 + 1, W + 64, True)
    assert att_lds_floats(S // 2 + 1, W, False) < att_lds_floats(S // 2 + 1, W, True)
    assert not query(geom(S + 2, 3)) and not query(geom(4, F + 1))
    for base in (top, TINY):
        assert not query(dict(base, gat_layer_dim=[1] * (LIMITS["max_layers"] + 1)))
        assert not query(dict(base, gat_layer_dim=[W + 1])) and not query(dict(base, gat_layer_dim=[1, W + 1]))
        assert not query(dict(base, lstm_hidden_dim=LIMITS["max_lstm_hidden"] + 1))
        assert not query(dict(base, autoencoder_hidden_dim=LIMITS["max_ae_width"] + 1))
        assert not query(dict(base, autoencoder_out_dim=LIMITS["max_ae_width"] + 1))
    assert query(PHM_C1) and query(PHM_C3) and query(XJTU)
    ws = lambda b: lib.rulgnn_gdagdl_workspace_bytes(C.byref(shape_of(b, XJTU)))      # noqa: E731
    assert ws(0) > 0 and ws(1024) > ws(100) > ws(1) >= ws(0) and ws(-1) == 0


def test_dropout_counters_that_do_not_fit_are_refused():
    """(sample_offset + batch) T N^2 and global_batch T N^2 must fit 32 bits: refused by all three entries before any launch."""
    lib = _lib.load()
    s = shape_of(2, XJTU)
    a = _lib.GdagdlArgs()
    a.global_batch, a.sample_offset = 2, (1 << 32) // (32 * 17 * 17)
    rcs = {lib.rulgnn_gdagdl_forward_f32(C.byref(s), C.byref(a), None), lib.rulgnn_gdagdl_backward_f32(C.byref(s), C.byref(a), None),
           lib.rulgnn_gdagdl_fwdbwd_f32(C.byref(s), C.byref(a), None, None)}
    assert rcs == {RULGNN_EUNSUPPORTED}
    a.sample_offset, a.global_batch = 0, (1 << 32) // (32 * 17 * 17) + 1
    assert lib.rulgnn_gdagdl_forward_f32(C.byref(s), C.byref(a), None) == RULGNN_EUNSUPPORTED


@pytest.mark.parametrize("cfg", [PHM_C1, PHM_C3, XJTU])
def test_workspace_grows_by_the_stated_tensors_and_nothing_pair_shaped(cfg):
    """Per sample: mag + ni + m + sum_l (Z_l + h_l) on the graph side, d Z and one d h buffer of the widest layer, the back end's
    activations and gradients -- and nothing N^2-shaped: the upper bound below is computed from the shapes and has no N^2 term, while
    the reference's pair tensor alone would be T N^2 2 C_1 floats per sample."""
    lib = _lib.load()
    T, N, f, Cs = cfg["num_patch"], cfg["num_nodes"], cfg["input_dim"], cfg["gat_layer_dim"]
    A, Oo, E = cfg["autoencoder_hidden_dim"], cfg["autoencoder_out_dim"], cfg["lstm_hidden_dim"]
    D = N * Cs[-1]
    per = (lib.rulgnn_gdagdl_workspace_bytes(C.byref(shape_of(2048, cfg))) - lib.rulgnn_gdagdl_workspace_bytes(C.byref(shape_of(1024, cfg)))) / 4 / 1024
    graph = T * N * (f + 2 + 2 * sum(Cs))
    grads = T * N * 2 * max(Cs)
    back = T * ((A + A // 2 + A // 4 + Oo) + (A // 4 + A // 2 + A + D) + 2 * D + 2 * max(A, Oo) + Oo + 2 * E) + 2
    lstm = (lib.rulgnn_gdagdl_workspace_bytes(C.byref(shape_of(2048, dict(cfg, gat_layer_dim=[1])))) / 4 / 2048)       # an upper bound of the LSTM's share
    assert graph + grads + back <= per <= graph + grads + back + lstm + 1
    assert per < T * N * N * 2 * Cs[0] or N < 4                # far below the reference's first pair tensor wherever N^2 matters
    s = shape_of(7, cfg)
    offs = [lib.rulgnn_gdagdl_tap_offset(C.byref(s), i) for i in range(6)]
    assert offs[0] == 0 and offs[5] == -1 and all(o >= 0 for o in offs[:5]) and len(set(offs[:5])) == 5
    assert offs[1] - offs[0] >= 7 * T * N * f and offs[2] - offs[1] >= 7 * T * N


def test_out_of_limit_model_constructs_and_is_refused_before_the_library_is_touched(monkeypatch):
    from gnn_rul_benchmarking_amd.gdagdl import GDAGDL_model
    m = GDAGDL_model(**dict(TINY, gat_layer_dim=[513]))
    monkeypatch.setattr(GDAGDL_model, "_require_device", lambda self, x: None)       # the limits answer before any device call
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("library touched")))
    with pytest.raises(RuntimeError, match="do not cover this configuration"):
        m(torch.zeros(2, 2))
    with pytest.raises(RuntimeError, match="do not cover this configuration"):
        m.fused_mse_step(torch.zeros(2, 2), torch.zeros(2))
    assert not m._bufs
    five = GDAGDL_model(**dict(TINY, gat_layer_dim=[1] * 5))
    with pytest.raises(RuntimeError, match="do not cover this configuration"):
        five(torch.zeros(2, 2))


def test_cpu_input_raises():
    from gnn_rul_benchmarking_amd.gdagdl import GDAGDL_model
    K.cpu_input_raises(GDAGDL_model(**TINY), torch.zeros(2, 2))


def test_fixtures_hold_no_grad_key_and_stay_small():
    """tests/test_grad_gate_cpu.py globs every fixture for ``grad:`` keys: this family's reference gradients are ``refgrad:``."""
    files = sorted(glob.glob(os.path.join(GOLDEN, "gdagdl_*.npz")))
    assert len(files) == 8
    for f in files:
        assert not [k for k in np.load(f).files if k.startswith("grad:")], f
        assert os.path.getsize(f) < 1 << 20
    for name in SMALL:
        z, cfg, _ = load_case(name)
        assert sorted(k[8:] for k in z.files if k.startswith("refgrad:")) == sorted(n for n in O.param_names(cfg) if n not in O.GRADLESS)
    for name in SMALL + FULL:
        assert {"x", "y", "pred", "pred_eval", "mse", "recon", "loss", "seed", "checksum", "margin", "tap:ni", "tap:mask"} <= set(load_case(name)[0].files)
    assert {"xs", "ys", "losses", "eval_pred_end", "lr", "wd"} <= set(np.load(os.path.join(GOLDEN, CURVE + ".npz")).files)


def test_struct_sizes_are_checked_at_load():
    lib = _lib.load()
    assert _lib.STRUCTS[35] is _lib.GdagdlShape and _lib.STRUCTS[36] is _lib.GdagdlArgs
    assert lib.rulgnn_struct_size(35) == C.sizeof(_lib.GdagdlShape) == 64
    assert lib.rulgnn_struct_size(36) == C.sizeof(_lib.GdagdlArgs) == 136
