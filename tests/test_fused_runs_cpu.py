"""Host-only checks of the grouped fused-step entries (rulgnn_{dvgtformer,logo}_fwdbwd_group_f32, csrc/rulgnn_api.hip:
step_fwdbwd_group) and of runs.DVGTformer_runs / runs.LOGO_runs: every answer here is given before any kernel launch, so no device is
needed."""
import argparse
import ctypes as C

import pytest
import torch

from gnn_rul_benchmarking_amd import _lib

BASE = 1 << 24              # placeholder device pointers: aligned, non-null, never dereferenced
POINTERS = ("x", "y", "params", "grads", "pred", "loss", "workspace")


def _dvgt_shape(batch=4, N=14):
    return _lib.DvgtformerShape(batch, N, 50, 4, 3, (C.c_int32 * 2)(144, 248), (C.c_int32 * 2)(72, 124), 0.5)


def _logo_shape(batch=4, hidden=8):
    return _lib.LogoShape(batch, 10, 5, 14, hidden)


FAMILIES = {
    "dvgtformer": (_lib.DvgtformerArgs, _dvgt_shape),
    "logo": (_lib.LogoArgs, _logo_shape),
}


def _entries(family):
    lib = _lib.load()
    return getattr(lib, f"rulgnn_{family}_fwdbwd_group_f32"), getattr(lib, f"rulgnn_{family}_fwdbwd_f32")


def _groups(family, n, shape=None, short=None, need=None):
    """n argument structs and Adam blocks with placeholder pointers, a group's own in every field, and a workspace of exactly the queried
    size (group ``short``: one byte less)."""
    Args, make_shape = FAMILIES[family]
    if need is None:
        need = getattr(_lib.load(), f"rulgnn_{family}_workspace_bytes")(C.byref(shape if shape is not None else make_shape()))
        assert need > 0
    args, opts = (Args * max(n, 1))(), (_lib.AdamArgs * max(n, 1))()
    for g, (a, o) in enumerate(zip(args, opts)):
        for k, name in enumerate(POINTERS):
            setattr(a, name, BASE * (g + 1) + 4096 * k)
        a.workspace_bytes = need - (1 if g == short else 0)
        a.global_batch, a.dropout_p, a.seed, a.step, a.training = 4, 0.1, 7 + g, 1, 1
        o.params, o.exp_avg, o.exp_avg_sq = a.params, BASE * (g + 1) + 4096 * 16, BASE * (g + 1) + 4096 * 17
        o.step, o.lr, o.beta1, o.beta2, o.eps = 1, 1e-3, 0.9, 0.999, 1e-8
    return args, opts


def test_step_max_groups_is_eight_and_within_the_grouped_lstms():
    lib = _lib.load()
    assert lib.rulgnn_step_max_groups() == 8 <= lib.rulgnn_bilstm_max_groups()


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n,code", [(0, _lib.EINVAL), (-1, _lib.EINVAL), (9, _lib.EUNSUPPORTED)])
def test_group_count_outside_the_range_is_refused(family, n, code):
    shape = FAMILIES[family][1]()
    args, opts = _groups(family, 9)
    group, _ = _entries(family)
    assert group(C.byref(shape), args, opts, n, None) == code
    assert group(C.byref(shape), args, None, n, None) == code


@pytest.mark.parametrize("family", FAMILIES)
def test_null_structs_and_a_null_pointer_in_the_last_group_are_invalid(family):
    shape = FAMILIES[family][1]()
    args, opts = _groups(family, 3)
    group, _ = _entries(family)
    assert group(None, args, opts, 3, None) == _lib.EINVAL
    assert group(C.byref(shape), None, opts, 3, None) == _lib.EINVAL
    for field in ("x", "grads", "y"):
        args, opts = _groups(family, 3)
        setattr(args[2], field, None)
        assert group(C.byref(shape), args, opts, 3, None) == _lib.EINVAL, field


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("short", [0, 2])
def test_a_group_whose_workspace_is_one_byte_short_is_refused_before_any_launch(family, short):
    shape = FAMILIES[family][1]()
    args, opts = _groups(family, 3, short=short)
    group, single = _entries(family)
    assert group(C.byref(shape), args, opts, 3, None) == _lib.EWORKSPACE
    assert single(C.byref(shape), C.byref(args[short]), None, None) == _lib.EWORKSPACE           # the single entry's answer for that group


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("field", ["workspace", "grads", "params"])
def test_two_groups_sharing_a_buffer_are_invalid(family, field):
    shape = FAMILIES[family][1]()
    args, opts = _groups(family, 3)
    setattr(args[2], field, getattr(args[0], field))
    opts[2].params = args[2].params
    group, _ = _entries(family)
    assert group(C.byref(shape), args, opts, 3, None) == _lib.EINVAL
    assert group(C.byref(shape), args, None, 3, None) == _lib.EINVAL


@pytest.mark.parametrize("family,shape", [("dvgtformer", _dvgt_shape(N=25)), ("logo", _logo_shape(hidden=32))], ids=["dvgtformer-N25", "logo-FD003"])
def test_a_shape_the_single_entry_refuses_gets_the_same_code(family, shape):
    lib = _lib.load()
    assert getattr(lib, f"rulgnn_{family}_workspace_bytes")(C.byref(shape)) == 0
    args, opts = _groups(family, 2, need=1 << 30)
    group, single = _entries(family)
    code = single(C.byref(shape), C.byref(args[0]), None, None)
    assert code == _lib.EUNSUPPORTED
    assert group(C.byref(shape), args, opts, 2, None) == code
    assert group(C.byref(shape), args, None, 2, None) == code


@pytest.mark.parametrize("family", FAMILIES)
def test_an_adam_block_over_another_groups_parameters_is_invalid(family):
    shape = FAMILIES[family][1]()
    args, opts = _groups(family, 2)
    group, single = _entries(family)
    opts[1].params = args[0].params
    assert group(C.byref(shape), args, opts, 2, None) == _lib.EINVAL
    assert single(C.byref(shape), C.byref(args[1]), C.byref(opts[1]), None) == _lib.EINVAL


@pytest.mark.parametrize("family", FAMILIES)
def test_what_the_single_entry_refuses_in_a_group_is_refused_with_its_code(family):
    """A dropout rate of 1 and a ``dpred`` in the last group: the single entry's RULGNN_EINVAL; a misaligned loss pointer: RULGNN_EALIGN."""
    shape = FAMILIES[family][1]()
    group, single = _entries(family)
    for field, value, code in (("dropout_p", 1.0, _lib.EINVAL), ("dpred", BASE * 9, _lib.EINVAL), ("loss", BASE * 9 + 2, _lib.EALIGN)):
        args, opts = _groups(family, 2)
        setattr(args[1], field, value)
        assert single(C.byref(shape), C.byref(args[1]), None, None) == code, field
        assert group(C.byref(shape), args, opts, 2, None) == code, field


# ---- the runs classes -------------------------------------------------------------------------------------------------------------------
def _tables(method, subset="FD001"):
    from gnn_rul_benchmarking_amd.hparams import get_hparams_class
    h = get_hparams_class("CMAPSS")(subset)
    return dict(h.alg_hparams[method]), dict(h.train_params[method])


def _runs_class(method):
    from gnn_rul_benchmarking_amd import runs
    return getattr(runs, method + "_runs")


@pytest.mark.parametrize("method", ["DVGTformer", "LOGO"])
def test_runs_are_built_with_the_sequential_protocols_initial_weights(method):
    from gnn_rul_benchmarking_amd.algorithms import get_algorithm_class
    from gnn_rul_benchmarking_amd.utils import fix_randomness
    cfg, tc = _tables(method)
    plain = get_algorithm_class(method)
    group = _runs_class(method)(cfg, tc, "cpu", [3, 1])
    assert len(group) == 2 and all(type(a) is plain for a in group.runs)
    for run_id, algo in zip((3, 1), group.runs):
        fix_randomness(run_id)
        alone = plain(cfg, tc, "cpu")
        assert algo.model._seed == alone.model._seed
        mine, theirs = algo.state_dict(), alone.state_dict()
        assert list(mine) == list(theirs) and len(mine) > 10
        for k in mine:
            assert torch.equal(mine[k], theirs[k]), k
    assert not torch.equal(group.runs[0].model.flat_params, group.runs[1].model.flat_params)
    assert group.train() is group and all(a.model.training for a in group.runs)
    assert group.eval() is group and not any(a.model.training for a in group.runs)
    with pytest.raises(RuntimeError, match="independent replicas"):
        group.attach_data_parallel(object())


@pytest.mark.parametrize("method", ["DVGTformer", "LOGO"])
def test_more_runs_than_groups_or_none_raise_at_construction(method):
    cfg, tc = _tables(method)
    with pytest.raises(ValueError, match="at most 8"):
        _runs_class(method)(cfg, tc, "cpu", range(9))
    with pytest.raises(ValueError, match="at least one"):
        _runs_class(method)(cfg, tc, "cpu", [])


@pytest.mark.parametrize("method", ["DVGTformer", "LOGO"])
def test_update_refuses_before_any_call_what_it_cannot_step(method):
    """One batch per run, the train mode, a CUDA input (the families' usual error) and one batch size: all before the library is asked."""
    cfg, tc = _tables(method)
    group = _runs_class(method)(cfg, tc, "cpu", [0, 1])
    x = torch.rand(4, 14, 50)
    y = torch.rand(4, 1)
    with pytest.raises(ValueError, match="one batch per run"):
        group.update([x], [y], 1)
    group.eval()
    with pytest.raises(RuntimeError, match="needs algorithm.train"):
        group.update([x, x], [y, y], 1)
    group.train()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        group.update([x, x], [y, y], 1)
    assert all(a.model._step == 0 and a.optimizer._steps == 0 for a in group.runs)          # nothing advanced


def test_the_registry_serves_both_families_and_still_refuses_st_gcn():
    from gnn_rul_benchmarking_amd.algorithms import get_algorithm_class
    from gnn_rul_benchmarking_amd.runs import DVGTformer_runs, LOGO_runs, get_runs_class
    assert get_runs_class("DVGTformer") is DVGTformer_runs and get_runs_class("LOGO") is LOGO_runs
    for name in ("ST_GCN", "LOGO_bearing"):
        with pytest.raises(NotImplementedError):
            get_runs_class(name)
    for name in ("DVGTformer_runs", "LOGO_runs"):
        with pytest.raises(NotImplementedError):
            get_algorithm_class(name)


@pytest.mark.parametrize("method", ["DVGTformer", "LOGO"])
def test_the_trainer_constructs_with_concurrent_runs(method, tmp_path):
    from gnn_rul_benchmarking_amd.main import build_parser
    from gnn_rul_benchmarking_amd.trainer import GNN_RUL_trainer
    base = dict(save_dir=str(tmp_path / "logs"), experiment_description="e", run_description="r", data_path=str(tmp_path / "no_data"),
                dataset="CMAPSS", dataset_id="FD001", bearing_id="b", num_runs=2, device="cpu")
    assert GNN_RUL_trainer(argparse.Namespace(GNN_method=method, concurrent_runs=2, **base)).concurrent_runs == 2
    assert method in build_parser().format_help()
