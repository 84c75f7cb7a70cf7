"""DVGTformer without a GPU: the registry, the module's surface (214 names in order, a seed gives the reference's initial weights,
strict load), the hparams rows, the C-ABI's size queries and the coverage gate at every limit."""
import ctypes as C
import glob
import json
import os

import numpy as np
import pytest
import torch

from gnn_rul_benchmarking_amd import _lib

from conftest import GOLDEN

import dvgtformer_oracle as O
import family_kit as K
from test_dvgtformer_oracle_golden import FULL, SMALL, load_case

FD = dict(num_nodes=14, time_length=50, d_model=[144, 248], num_heads=4, lambda_param=0.5, d_ff=[72, 124], dropout=0.1, num_blocks=3)
NCMAPSS = dict(FD, num_nodes=20)
TINY = dict(num_nodes=2, time_length=1, d_model=[1, 1], num_heads=1, lambda_param=0.5, d_ff=[1, 1], dropout=0.1, num_blocks=1)
RULGNN_EUNSUPPORTED = -2                # include/rulgnn.h


def shape_of(batch, cfg):
    return _lib.DvgtformerShape(batch, cfg["num_nodes"], cfg["time_length"], cfg["num_heads"], cfg["num_blocks"],
                                (C.c_int32 * 2)(*cfg["d_model"]), (C.c_int32 * 2)(*cfg["d_ff"]), cfg["lambda_param"])


def test_registry_serves_the_algorithm_and_refuses_the_model():
    K.registry_check("DVGTformer")


def test_algorithm_construction():
    from gnn_rul_benchmarking_amd import algorithms as A
    from gnn_rul_benchmarking_amd.dvgtformer import DVGTformer_model
    from gnn_rul_benchmarking_amd.hparams import get_hparams_class
    from gnn_rul_benchmarking_amd.optim import FusedAdam
    h = get_hparams_class("CMAPSS")("FD002")
    algo = A.get_algorithm_class("DVGTformer")(h.alg_hparams["DVGTformer"], h.train_params["DVGTformer"], "cpu")
    assert isinstance(algo.model, DVGTformer_model) and isinstance(algo.optimizer, FusedAdam)
    assert algo.hparams == h.train_params["DVGTformer"] and algo.model.c_family == "dvgtformer" and algo.model.dropout_p == 0.1
    assert algo.model.dropout_by_sample_offset is True and algo.model.eval_sample_independent is True
    assert sum(p.numel() for p in algo.model.parameters()) == _lib.load().rulgnn_dvgtformer_param_count(C.byref(shape_of(100, FD))) == 850622
    algo.eval()
    with pytest.raises(RuntimeError, match="needs algorithm.train"):
        algo.update(torch.zeros(2, 14, 50), torch.zeros(2, 1))


@pytest.mark.parametrize("name", SMALL + FULL)
def test_a_seed_gives_the_reference_keys_and_initial_values(name):
    """The names, their order, strict load and -- under the fixture's seed plus the maker's recorded perturbation -- the reference's
    values: bit for bit where the fixture stores them, by the fp64 checksum of all 850 622 (N = 14) where it stores the seed alone."""
    from gnn_rul_benchmarking_amd.dvgtformer import DVGTformer_model
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    cfg = json.loads(str(z["cfg_json"]))
    seed = int(z["seed"])
    torch.manual_seed(seed)
    m = DVGTformer_model(**cfg)
    sd = m.state_dict()
    names = O.param_names(cfg)
    assert list(sd.keys()) == [n for n, _ in m.named_parameters()] == names
    assert len(names) == 6 + cfg["num_blocks"] * (12 * cfg["num_heads"] + 20) + 4
    assert {k: tuple(v.shape) for k, v in sd.items()} == O.param_shapes(cfg)
    assert "positional_encoding" not in sd and not list(m.named_buffers())
    assert np.array_equal(m.flat_params.numpy(), np.concatenate([sd[k].numpy().ravel() for k in names]))
    g = torch.Generator().manual_seed(seed + 1000)
    moved = {k: v.clone().add_(torch.empty_like(v).uniform_(-0.1, 0.1, generator=g)) for k, v in sd.items()}
    flat = np.concatenate([moved[k].numpy().astype(np.float64).ravel() for k in names])
    assert np.allclose([flat.sum(), (flat * flat).sum()], z["checksum"], rtol=1e-12, atol=0)
    if name in SMALL:
        for k in names:
            assert np.array_equal(moved[k].numpy(), z["sd:" + k]), k
        other = DVGTformer_model(**cfg)
        other.load_state_dict({k: torch.from_numpy(z["sd:" + k]) for k in names}, strict=True)
        assert np.array_equal(other.state_dict()["x_v"].numpy(), z["sd:x_v"])
    else:
        assert len(names) == 214 and m.num_live == {14: 850622}.get(cfg["num_nodes"], m.num_live)
        assert load_case(name)[2].keys() == sd.keys()


def test_hparams_rows_equal_the_reference():
    from gnn_rul_benchmarking_amd.hparams import get_hparams_class
    K.hparams_rows_check("DVGTformer", "dvgtformer_hparams_rows.npz", ["CMAPSS/FD001", "CMAPSS/FD002", "CMAPSS/FD003", "CMAPSS/FD004", "NCMAPSS/None"],
                         ["PHM2012/Condition_1"])
    assert get_hparams_class("CMAPSS")("FD003").alg_hparams["DVGTformer"] == FD
    assert get_hparams_class("NCMAPSS")(None).alg_hparams["DVGTformer"] == NCMAPSS


def test_limits_are_stated_once_and_admit_the_five_rows():
    from gnn_rul_benchmarking_amd.dvgtformer import LIMITS
    from gnn_rul_benchmarking_amd.hparams import get_hparams_class
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "rulgnn.h")).read()
    for name, key in (("NODES", "max_nodes"), ("TIME", "max_time"), ("HEADS", "max_heads"), ("BLOCKS", "max_blocks"),
                      ("D_MODEL", "max_d_model"), ("D_FF", "max_d_ff")):
        assert f"#define RULGNN_DVGT_MAX_{name} {LIMITS[key]}\n" in header
    rows = [get_hparams_class("CMAPSS")(d).alg_hparams["DVGTformer"] for d in ("FD001", "FD002", "FD003", "FD004")]
    rows.append(get_hparams_class("NCMAPSS")(None).alg_hparams["DVGTformer"])
    for cfg in rows:
        for B in (1, 100, 1024):
            assert lib.rulgnn_dvgtformer_workspace_bytes(C.byref(shape_of(B, cfg))) > 0
            assert lib.rulgnn_dvgtformer_param_count(C.byref(shape_of(B, cfg))) == O_count(cfg)


def O_count(cfg):
    return sum(int(np.prod(s)) for s in O.param_shapes(cfg).values())


def lds_floats(cfg, bwd):
    """csrc/dvgtformer_device.hpp dv_lds, restated."""
    Lp, Np = cfg["time_length"] + 1, cfg["num_nodes"] + 1
    E, Tm = Lp * Np, max(Lp, Np)
    YN, TT, HN = max(Lp * (Np + 1), Np * (Lp + 1)), Tm * Tm, max(Lp * cfg["d_ff"][0], Np * cfg["d_ff"][1])
    hn = max(HN, TT) if bwd else HN
    o = 4 * E + YN + TT + Lp * Lp + Np * Np + hn + 6 * Tm
    return o + (hn + 2 * E + YN + Lp * Lp + Np * Np if bwd else 0)


def test_coverage_gate_every_limit_plus_one():
    from gnn_rul_benchmarking_amd.dvgtformer import LIMITS, within_limits
    lib = _lib.load()

    def query(cfg, B=3):
        s = shape_of(B, cfg)
        pc, ws = lib.rulgnn_dvgtformer_param_count(C.byref(s)), lib.rulgnn_dvgtformer_workspace_bytes(C.byref(s))
        assert (pc < 0) == (ws == 0) and (lib.rulgnn_dvgtformer_tap_offset(C.byref(s), 1) < 0) == (ws == 0)
        inside = within_limits(cfg["num_nodes"], cfg["time_length"], cfg["d_model"], cfg["num_heads"], cfg["d_ff"], cfg["num_blocks"])
        assert inside == (ws > 0)                      # the Python statement of the limits and the library's agree
        if ws == 0:                                    # refused by the entries too, before any launch (no device is needed to be told so)
            a = _lib.DvgtformerArgs()
            rcs = {lib.rulgnn_dvgtformer_forward_f32(C.byref(s), C.byref(a), None), lib.rulgnn_dvgtformer_backward_f32(C.byref(s), C.byref(a), None),
                   lib.rulgnn_dvgtformer_fwdbwd_f32(C.byref(s), C.byref(a), None, None)}
            assert len(rcs) == 1 and rcs <= {RULGNN_EUNSUPPORTED, -1}
        return ws > 0

    assert query(TINY)                                                      # every lower limit at once
    assert not query(dict(TINY, num_nodes=1)) and not query(dict(TINY, time_length=0)) and not query(dict(TINY, num_heads=0))
    assert not query(dict(TINY, num_blocks=0))
    top = dict(TINY, num_nodes=LIMITS["max_nodes"], time_length=LIMITS["max_time"], num_heads=LIMITS["max_heads"],
               num_blocks=LIMITS["max_blocks"], d_model=[LIMITS["max_d_model"]] * 2, d_ff=[LIMITS["max_d_ff"]] * 2)
    assert query(top)                                                       # every upper limit at once: still within one CU's LDS
    assert 4 * lds_floats(top, True) <= 160 * 1024 and lds_floats(top, False) < lds_floats(top, True)
    for key in ("num_nodes", "time_length", "num_heads", "num_blocks"):
        assert not query(dict(top, **{key: top[key] + 1})), key
        assert not query(dict(TINY, **{key: top[key] + 1})), key
    for key in ("d_model", "d_ff"):
        assert not query(dict(top, **{key: [top[key][0] + 1, 1]})) and not query(dict(top, **{key: [1, top[key][1] + 1]}))
    assert query(FD) and query(NCMAPSS)
    ws = lambda b: lib.rulgnn_dvgtformer_workspace_bytes(C.byref(shape_of(b, FD)))      # noqa: E731
    assert ws(0) > 0 and ws(1024) > ws(100) > ws(1) >= ws(0) and ws(-1) == 0


def test_workspace_keeps_half_block_inputs_only():
    """Per sample the workspace holds the 2 nb half-block inputs and the encoder output ((2 nb + 1) (L+1)(N+1) floats), the head's two
    100-wide rows and d enc: no score matrix, no Q / K / V, nothing d_model wide."""
    lib = _lib.load()
    for cfg in (FD, NCMAPSS):
        E = (cfg["time_length"] + 1) * (cfg["num_nodes"] + 1)
        per = (lib.rulgnn_dvgtformer_workspace_bytes(C.byref(shape_of(2048, cfg))) - lib.rulgnn_dvgtformer_workspace_bytes(C.byref(shape_of(1024, cfg)))) / 4 / 1024
        assert (2 * cfg["num_blocks"] + 2) * E + 202 <= per <= (2 * cfg["num_blocks"] + 2) * E + 202 + 1
        s = shape_of(7, cfg)
        x0, enc = lib.rulgnn_dvgtformer_tap_offset(C.byref(s), 0), lib.rulgnn_dvgtformer_tap_offset(C.byref(s), 1)
        assert enc - x0 == 2 * cfg["num_blocks"] * 7 * E and lib.rulgnn_dvgtformer_tap_offset(C.byref(s), 2) == -1


def test_out_of_limit_model_constructs_and_is_refused_before_the_library_is_touched(monkeypatch):
    from gnn_rul_benchmarking_amd.dvgtformer import DVGTformer_model
    m = DVGTformer_model(**dict(TINY, num_nodes=25))
    monkeypatch.setattr(DVGTformer_model, "_require_device", lambda self, x: None)       # the limits answer before any device call
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("library touched")))
    with pytest.raises(RuntimeError, match="do not cover this configuration"):
        m(torch.zeros(2, 25, 1))
    with pytest.raises(RuntimeError, match="do not cover this configuration"):
        m.fused_mse_step(torch.zeros(2, 25, 1), torch.zeros(2))
    assert not m._bufs


def test_cpu_input_raises():
    from gnn_rul_benchmarking_amd.dvgtformer import DVGTformer_model
    m = DVGTformer_model(**TINY)
    K.cpu_input_raises(m, torch.zeros(2, 2, 1))
    with pytest.raises(RuntimeError, match="expects"):
        m(torch.zeros(2, 3, 1))


def test_fixtures_hold_no_grad_key_and_stay_small():
    """tests/test_grad_gate_cpu.py globs every fixture for ``grad:`` keys: this family's reference gradients are ``refgrad:``."""
    files = sorted(glob.glob(os.path.join(GOLDEN, "dvgtformer_*.npz")))
    assert len(files) == 7
    for f in files:
        assert not [k for k in np.load(f).files if k.startswith("grad:")], f
        assert os.path.getsize(f) < 1 << 20
    for name in SMALL:
        z, cfg, _ = load_case(name)
        assert sorted(k[8:] for k in z.files if k.startswith("refgrad:")) == sorted(O.param_names(cfg))
    for name in SMALL + FULL:
        assert {"x", "y", "pred", "pred_eval", "loss", "seed", "checksum", "pe", "tap:x0", "tap:enc", "tap:a_temp", "tap:a_spat"} <= set(load_case(name)[0].files)


def test_struct_sizes_are_checked_at_load():
    lib = _lib.load()
    assert _lib.STRUCTS[33] is _lib.DvgtformerShape and _lib.STRUCTS[34] is _lib.DvgtformerArgs
    assert lib.rulgnn_struct_size(33) == C.sizeof(_lib.DvgtformerShape) == 48
    assert lib.rulgnn_struct_size(34) == C.sizeof(_lib.DvgtformerArgs)
