"""Host-only checks of the grouped Bi-LSTM entries (csrc/bilstm.hip: rulgnn_bilstm_*_group_f32) and of runs.py: every answer here is
given before any kernel launch, so no device is needed."""
import ctypes as C

import pytest
import torch

from gnn_rul_benchmarking_amd import _lib

BASE = 1 << 20              # placeholder device pointers: aligned, non-null, never dereferenced


def _groups(n, shape, short=None):
    """n argument structs with placeholder pointers and a workspace of exactly the queried size (group ``short``: one byte less)."""
    lib = _lib.load()
    need = lib.rulgnn_bilstm_workspace_bytes(C.byref(shape))
    arr = (_lib.BilstmArgs * max(n, 1))()
    for g, a in enumerate(arr):
        k = 0
        for name, ctype in a._fields_:
            if name in ("workspace_bytes", "aux_stream"):
                continue
            if ctype is C.c_void_p:
                k += 1
                setattr(a, name, BASE * (g + 1) + 256 * k)
            else:                                                     # the per-direction pointer pairs
                pair = getattr(a, name)
                for d in range(2):
                    k += 1
                    pair[d] = BASE * (g + 1) + 256 * k
        a.workspace_bytes = need - (1 if g == short else 0)
    return arr


def _entries():
    lib = _lib.load()
    return lib.rulgnn_bilstm_forward_group_f32, lib.rulgnn_bilstm_backward_group_f32


def test_max_groups_is_eight():
    assert _lib.load().rulgnn_bilstm_max_groups() == 8


@pytest.mark.parametrize("n,code", [(0, _lib.EINVAL), (-1, _lib.EINVAL), (9, _lib.EUNSUPPORTED)])
def test_group_count_outside_the_range_is_refused(n, code):
    shape = _lib.BilstmShape(12, 2, 5, 16)
    arr = _groups(9, shape)
    for entry in _entries():
        assert entry(C.byref(shape), arr, n, None) == code


def test_a_shape_the_single_entry_refuses_gets_the_same_code():
    lib = _lib.load()
    shape = _lib.BilstmShape(12, 2, 5, 129)                            # hidden_dim > 128
    assert lib.rulgnn_bilstm_workspace_bytes(C.byref(shape)) == 0
    arr = _groups(2, _lib.BilstmShape(12, 2, 5, 16))
    single = lib.rulgnn_bilstm_forward_f32(C.byref(shape), C.byref(arr[0]), None)
    assert single == _lib.EUNSUPPORTED
    assert lib.rulgnn_bilstm_backward_f32(C.byref(shape), C.byref(arr[0]), None) == single
    for entry in _entries():
        assert entry(C.byref(shape), arr, 2, None) == single


@pytest.mark.parametrize("short", [0, 2])
def test_a_group_whose_workspace_is_one_byte_short_is_refused_before_any_launch(short):
    shape = _lib.BilstmShape(12, 2, 5, 16)
    arr = _groups(3, shape, short=short)
    for entry in _entries():
        assert entry(C.byref(shape), arr, 3, None) == _lib.EWORKSPACE


def test_null_arguments_are_invalid():
    shape = _lib.BilstmShape(12, 2, 5, 16)
    arr = _groups(2, shape)
    for entry in _entries():
        assert entry(None, arr, 2, None) == _lib.EINVAL
        assert entry(C.byref(shape), None, 2, None) == _lib.EINVAL
    arr[1].x = None                                                    # a null pointer in the LAST group
    for entry in _entries():
        assert entry(C.byref(shape), arr, 2, None) == _lib.EINVAL


def _hagcn_tables():
    from gnn_rul_benchmarking_amd.hparams import get_hparams_class
    h = get_hparams_class("CMAPSS")("FD004")
    return h.alg_hparams["HAGCN"], h.train_params["HAGCN"]


def test_more_runs_than_groups_raises_at_construction():
    from gnn_rul_benchmarking_amd.runs import HAGCN_runs
    cfg, tc = _hagcn_tables()
    with pytest.raises(ValueError, match="at most 8"):
        HAGCN_runs(cfg, tc, "cpu", range(9))
    with pytest.raises(ValueError):
        HAGCN_runs(cfg, tc, "cpu", [])


def test_runs_class_is_not_a_registry_entry():
    from gnn_rul_benchmarking_amd.algorithms import get_algorithm_class
    from gnn_rul_benchmarking_amd.runs import HAGCN_runs, get_runs_class
    with pytest.raises(NotImplementedError):
        get_algorithm_class("HAGCN_runs")
    assert get_runs_class("HAGCN") is HAGCN_runs
    with pytest.raises(NotImplementedError):
        get_runs_class("ST_GCN")


def test_runs_are_built_with_the_sequential_protocols_initial_weights_and_refuse_data_parallel():
    from gnn_rul_benchmarking_amd.algorithms import HAGCN
    from gnn_rul_benchmarking_amd.runs import HAGCN_runs
    from gnn_rul_benchmarking_amd.utils import fix_randomness
    cfg, tc = _hagcn_tables()
    group = HAGCN_runs(cfg, tc, "cpu", [3, 1])
    assert len(group) == 2 and all(type(a) is HAGCN for a in group.runs)
    for run_id, algo in zip((3, 1), group.runs):
        fix_randomness(run_id)
        alone = HAGCN(cfg, tc, "cpu")
        for (k, v), (k2, v2) in zip(algo.state_dict().items(), alone.state_dict().items()):
            assert k == k2 and torch.equal(v, v2), k
    with pytest.raises(RuntimeError, match="independent replicas"):
        group.attach_data_parallel(object())


def test_generator_context_restores_the_global_generator_and_separates_the_runs():
    from gnn_rul_benchmarking_amd.runs import RunGenerators
    torch.manual_seed(1234)
    before = torch.get_rng_state().clone()
    a, b = RunGenerators(0, "cpu"), RunGenerators(1, "cpu")
    assert torch.equal(torch.get_rng_state(), before)                  # building them leaves the global generator alone
    with a.active():
        a1 = torch.rand(4)
    with b.active():
        b1 = torch.rand(4)
    with a.active():
        a2 = torch.rand(4)
    assert torch.equal(torch.get_rng_state(), before)                  # ... and so does drawing inside them
    assert not torch.equal(a1, b1)                                     # two runs, two streams
    torch.manual_seed(0)                                               # run 0 alone: the same draws, in the same order
    assert torch.equal(torch.rand(4), a1) and torch.equal(torch.rand(4), a2)
    torch.manual_seed(1)
    assert torch.equal(torch.rand(4), b1)


def test_concurrent_runs_is_refused_for_a_method_without_a_runs_class_before_data_is_loaded(tmp_path):
    import argparse
    from gnn_rul_benchmarking_amd.main import build_parser
    from gnn_rul_benchmarking_amd.trainer import GNN_RUL_trainer
    assert build_parser().parse_args([]).concurrent_runs == 1
    base = dict(save_dir=str(tmp_path / "logs"), experiment_description="e", run_description="r", data_path=str(tmp_path / "no_data"),
                dataset="CMAPSS", dataset_id="FD004", bearing_id="b", num_runs=2, device="cpu")
    with pytest.raises(NotImplementedError, match="runs class"):
        GNN_RUL_trainer(argparse.Namespace(GNN_method="ST_GCN", concurrent_runs=2, **base))
    assert GNN_RUL_trainer(argparse.Namespace(GNN_method="HAGCN", concurrent_runs=2, **base)).concurrent_runs == 2
    assert GNN_RUL_trainer(argparse.Namespace(GNN_method="ST_GCN", **base)).concurrent_runs == 1
