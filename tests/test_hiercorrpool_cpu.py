"""HierCorrPool without a GPU: the registry, the module's surface, the hparams rows, the C-ABI's size queries, the coverage gate and the
workspace layout (no N x N or N x d graph intermediate per sample beyond X itself)."""
import ctypes as C
import glob
import os

import numpy as np
import pytest
import torch

from gnn_rul_benchmarking_amd import _lib

from conftest import GOLDEN

import family_kit as K
import hiercorrpool_oracle as O

FIELDS = "patch_size num_patch hidden_dim embedding_dim num_nodes encoder_conv_kernel num_nodes_out".split()
FIXTURES = ["hiercorrpool_small_7x3_n5_bs6", "hiercorrpool_fd001geom_bs4", "hiercorrpool_fd004geom_bs4", "hiercorrpool_ncmapssgeom_bs3"]
FD001 = dict(patch_size=25, num_patch=2, hidden_dim=10, embedding_dim=10, num_nodes=14, encoder_conv_kernel=8, num_nodes_out=6)
FD004 = dict(FD001, patch_size=10, num_patch=5, encoder_conv_kernel=12)
NCMAPSS = dict(FD001, patch_size=1, num_patch=50, num_nodes=20, encoder_conv_kernel=32)


def shape_of(batch, cfg):
    return _lib.HiercorrpoolShape(batch, *[cfg[k] for k in FIELDS])


def test_registry_serves_the_algorithm_and_refuses_the_model():
    from gnn_rul_benchmarking_amd import algorithms as A
    K.registry_check("HierCorrPool", needs_train_mode="BatchNorm batch statistics, dropout")
    with pytest.raises(NotImplementedError, match="Algorithm not found: HierCorrPool_bearing"):
        A.get_algorithm_class("HierCorrPool_bearing")


def test_algorithm_construction_and_data_parallel_refusal():
    from gnn_rul_benchmarking_amd import algorithms as A
    from gnn_rul_benchmarking_amd.hiercorrpool import HierCorrPool_model
    from gnn_rul_benchmarking_amd.hparams import get_hparams_class
    from gnn_rul_benchmarking_amd.optim import FusedAdam
    h = get_hparams_class("CMAPSS")("FD001")
    algo = A.get_algorithm_class("HierCorrPool")(h.alg_hparams["HierCorrPool"], h.train_params["HierCorrPool"], "cpu")
    assert isinstance(algo.model, HierCorrPool_model) and isinstance(algo.optimizer, FusedAdam)
    assert algo.hparams == h.train_params["HierCorrPool"] and algo.model.c_family == "hiercorrpool" and algo.model.dropout_p == 0.35
    assert sum(p.numel() for p in algo.model.parameters()) == _lib.load().rulgnn_hiercorrpool_param_count(C.byref(shape_of(100, FD001)))
    with pytest.raises(RuntimeError, match="data parallelism for HierCorrPool is not built yet"):
        algo.attach_data_parallel(object())
    algo.eval()
    with pytest.raises(RuntimeError, match="needs algorithm.train"):
        algo.update(torch.zeros(2, 14, 50), torch.zeros(2, 1))


@pytest.mark.parametrize("name", FIXTURES)
def test_a_seed_gives_the_reference_state_dict(name):
    """The 28 keys, their order, strict load and -- under the fixture's seed -- the initial values bit for bit."""
    from gnn_rul_benchmarking_amd.hiercorrpool import HierCorrPool_model
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    cfg = {k[4:]: int(z[k]) for k in z.files if k.startswith("cfg:")}
    torch.manual_seed(int(z["seed"]))
    m = HierCorrPool_model(**cfg)
    sd = m.state_dict()
    assert list(sd.keys()) == [k[3:] for k in z.files if k.startswith("sd:")] == O.state_keys() and len(sd) == 28
    assert [n for n, _ in m.named_parameters()] == O.param_names() and len(O.param_names()) == 19
    for k, v in sd.items():
        assert v.shape == z["sd:" + k].shape and np.array_equal(v.numpy(), z["sd:" + k]), k
    assert np.array_equal(m.flat_params.numpy(), np.concatenate([z["sd:" + k].ravel() for k in O.param_names()]))
    other = HierCorrPool_model(**cfg)
    other.load_state_dict({k: torch.from_numpy(z["bn_after:" + k] if "bn_after:" + k in z.files else z["sd:" + k]) for k in sd}, strict=True)
    for l in (1, 2, 3):
        key = O.ENC.format(l) + "1."
        assert int(other.state_dict()[key + "num_batches_tracked"]) == 1
        assert np.array_equal(other.state_dict()[key + "running_var"].numpy(), z["bn_after:" + key + "running_var"])
    assert m.input_dim == 10                                # accepted and unused, as in the reference


def test_hparams_rows_equal_the_reference():
    from gnn_rul_benchmarking_amd.hparams import get_hparams_class
    K.hparams_rows_check("HierCorrPool", "hiercorrpool_hparams_rows.npz", ["CMAPSS/FD001", "CMAPSS/FD002", "CMAPSS/FD003", "CMAPSS/FD004", "NCMAPSS/None"],
                         ["PHM2012/Condition_1"])
    assert get_hparams_class("CMAPSS")("FD001").alg_hparams["HierCorrPool"] == dict(FD001, input_dim=10)
    assert get_hparams_class("CMAPSS")("FD004").alg_hparams["HierCorrPool"] == dict(FD004, input_dim=10)
    assert get_hparams_class("NCMAPSS")(None).alg_hparams["HierCorrPool"] == dict(NCMAPSS, input_dim=10)


def test_construction_names_both_numbers_when_the_reshape_cannot_exist():
    from gnn_rul_benchmarking_amd.hiercorrpool import HierCorrPool_model, encoder_lengths
    assert [encoder_lengths(P)[-1] for P in (2, 5, 10, 50)] == [2, 3, 3, 8] == [O.lengths(P)[-1] for P in (2, 5, 10, 50)]
    with pytest.raises(ValueError, match=r"80 in all.*encoder_conv_kernel \* embedding_dim = 120"):
        HierCorrPool_model(**dict(FD001, input_dim=10, encoder_conv_kernel=12))     # FD001's length with FD004's kernel
    # the C side refuses the same configuration before anything else
    lib = _lib.load()
    bad = shape_of(4, dict(FD001, encoder_conv_kernel=12))
    assert lib.rulgnn_hiercorrpool_param_count(C.byref(bad)) < 0 and lib.rulgnn_hiercorrpool_workspace_bytes(C.byref(bad)) == 0


def test_cpu_input_raises():
    from gnn_rul_benchmarking_amd.hiercorrpool import HierCorrPool_model
    K.cpu_input_raises(HierCorrPool_model(3, 7, 10, 2, 2, 5, 12, 3), torch.zeros(2, 5, 21))


def test_new_fixtures_hold_no_grad_key():
    """tests/test_grad_gate_cpu.py globs every fixture for ``grad:`` keys: this family's reference gradients are ``refgrad:``."""
    files = sorted(glob.glob(os.path.join(GOLDEN, "hiercorrpool_*.npz")))
    assert len(files) == 7
    for f in files:
        keys = np.load(f).files
        assert not [k for k in keys if k.startswith("grad:")], f
    for name in FIXTURES:
        keys = np.load(os.path.join(GOLDEN, name + ".npz")).files
        assert sorted(k[8:] for k in keys if k.startswith("refgrad:")) == sorted(O.param_names())


def test_struct_sizes_are_checked_at_load():
    lib = _lib.load()
    assert _lib.STRUCTS[29] is _lib.HiercorrpoolShape and _lib.STRUCTS[30] is _lib.HiercorrpoolArgs
    assert lib.rulgnn_struct_size(29) == C.sizeof(_lib.HiercorrpoolShape) == 40
    assert lib.rulgnn_struct_size(30) == C.sizeof(_lib.HiercorrpoolArgs)


@pytest.mark.parametrize("cfg,millions", [(FD001, 2.0), (FD004, 1.8), (NCMAPSS, 3.7)])
def test_param_and_bn_counts(cfg, millions):
    lib = _lib.load()
    N, h, e, K, M, p = (cfg[k] for k in ("num_nodes", "hidden_dim", "embedding_dim", "encoder_conv_kernel", "num_nodes_out", "patch_size"))
    d, C0, C1 = K * e, N * p, h * N
    want = 8 * (C1 * C0 + 2 * C1 * C1 + 8 * C1 * C1) + 2 * 7 * C1 + 3 * d * d + 3 * d + M * d + M + M * (N + M) + M + 3 * e * 3 * d * M + 3 * e + 3 * e + 1
    got = lib.rulgnn_hiercorrpool_param_count(C.byref(shape_of(7, cfg)))
    assert got == want and round(got / 1e6, 1) == millions
    assert lib.rulgnn_hiercorrpool_bn_state_count(C.byref(shape_of(7, cfg))) == 2 * 7 * C1


def test_coverage_gate_every_limit_plus_and_minus_one():
    lib = _lib.load()
    RULGNN_EUNSUPPORTED = -2                # include/rulgnn.h

    def query(cfg):
        s = shape_of(3, cfg)
        pc, ws = lib.rulgnn_hiercorrpool_param_count(C.byref(s)), lib.rulgnn_hiercorrpool_workspace_bytes(C.byref(s))
        assert (pc < 0) == (ws == 0) and (lib.rulgnn_hiercorrpool_tap_offset(C.byref(s), 1) < 0) == (ws == 0)
        if ws == 0:                    # refused by the entries too, before any launch (no device is needed to be told so)
            a = _lib.HiercorrpoolArgs()
            rcs = {lib.rulgnn_hiercorrpool_forward_f32(C.byref(s), C.byref(a), None), lib.rulgnn_hiercorrpool_backward_f32(C.byref(s), C.byref(a), None),
                   lib.rulgnn_hiercorrpool_fwdbwd_f32(C.byref(s), C.byref(a), None, None)}
            assert rcs == {RULGNN_EUNSUPPORTED}
        return ws > 0

    def cfg(p=1, P=2, h=1, e=1, N=2, K=8, M=1):
        return dict(patch_size=p, num_patch=P, hidden_dim=h, embedding_dim=e, num_nodes=N, encoder_conv_kernel=K, num_nodes_out=M)

    assert query(cfg())                                                     # every lower limit at once: N 2, M 1, P 2, p 1
    assert not query(cfg(N=1, K=8)) and not query(cfg(M=0)) and not query(cfg(P=1)) and not query(cfg(p=0))
    assert query(cfg(N=32)) and not query(cfg(N=33))
    assert query(cfg(M=16)) and not query(cfg(M=17))
    assert query(cfg(P=64, K=40)) and not query(cfg(P=65, K=40))            # L'(64) = L'(65) = 10
    assert query(cfg(p=64)) and not query(cfg(p=65))
    assert query(cfg(h=64, e=64, K=8)) and not query(cfg(h=65, e=65, K=8))  # d = 512 / 520
    assert query(cfg(h=8, e=8, N=32)) and not query(cfg(h=9, e=9, N=32))    # C3 = 1024 / 1152
    assert not query(cfg(K=9))                                              # L' 4h = 8 != K e = 9
    # the widest d beside M = 16 (C3 <= 1024 leaves N = 4 there) and the widest d that N = 32 allows (L' <= 10, h <= 8: 320): the LDS fits
    assert query(cfg(h=64, e=64, K=8, N=4, M=16)) and query(cfg(h=8, e=8, K=40, P=64, N=32, M=16))


def test_workspace_holds_no_graph_intermediate_per_sample():
    """Between the encoder output (X itself, read through the flat reinterpretation) and H the workspace holds X', A' and A' X' and
    nothing else: no N x N matrix (G, A) and no second N x d matrix (A X), S or Z -- those live in LDS (csrc/hiercorrpool.hip:
    HcGraphLds).  Regions are carved in order on 256-byte boundaries, and the taps are their float offsets."""
    lib = _lib.load()
    al = lambda floats: (floats + 63) // 64 * 64      # noqa: E731
    for cfg in (FD001, FD004, NCMAPSS):
        N, e, K, M = (cfg[k] for k in ("num_nodes", "embedding_dim", "encoder_conv_kernel", "num_nodes_out"))
        d = K * e
        for B in (1, 100, 1024):
            s = shape_of(B, cfg)
            enc, xp, ap, H = (lib.rulgnn_hiercorrpool_tap_offset(C.byref(s), i) for i in range(4))
            assert lib.rulgnn_hiercorrpool_tap_offset(C.byref(s), 4) == -1
            assert xp - enc == al(B * N * d)                              # X: the encoder output
            assert ap - xp == al(B * M * d)                               # X'
            assert H - ap == al(B * M * M) + al(B * M * d)                # A', A' X'
            assert (H - enc) / B < N * d + 2 * M * d + M * M + 3 * 64 / B + N * N, "an N x N or N x d intermediate would not fit here"
            assert (H + B * M * 3 * d) * 4 <= lib.rulgnn_hiercorrpool_workspace_bytes(C.byref(s))
    ws = lambda b: lib.rulgnn_hiercorrpool_workspace_bytes(C.byref(shape_of(b, FD001)))      # noqa: E731
    assert ws(0) > 0 and ws(1024) > ws(100) > ws(1) >= ws(0) and ws(-1) == 0
