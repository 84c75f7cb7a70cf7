"""-m gpu: every family's calls on a stale workspace (tests/family_kit.py, section 9).  A workspace need not be initialised and need not
be preserved between calls (include/rulgnn.h): a fused step twice in a row, an eval forward and an autograd forward + backward must give,
with NaN, with the leading bytes of a batch-37 workspace, or with what a step on other data under other weights left in the workspace,
what they give on a zeroed one.  The bar is equal bit patterns; the three families whose steps add fp64 BatchNorm cells with atomicAdd
are held to the bar their own files use between two schedules of one step.

TABLE has one row per FlatModule family but ST_GCN (tests/test_train_mx_hrec_gpu.py and its neighbours hold its matrix-core step to
this); NOT_YET names the families that have none yet.  State dict and sample shape are those of the family's smallest fixture; the
batches of 1, 3 and 5 (every 4-, 8- and 16-sample tile ragged, every clamped grid under-filled) and of 37 are drawn uniformly over the
fixture's own range of values, a new draw per seed: the comparison is between two runs of the kernels, no oracle reads the samples.

Behind the table: an epoch walk per _FusedAlgorithm of the registry (workspaces evicted and allocated again, ``workspace_slots`` and
``_pin_bufs`` untouched) against a fresh algorithm given the same state, and HAGCN, which owns no cached workspace, through its Bi-LSTM
and graph entries on a workspace this file owns.

No slot of the table's families' workspaces holds an index or a count (profiles/r37_stale_workspace.md lists the carves): a fill can
make a result wrong, not an address.  HAGCN's one integer slot, the top-k selection, is written by the forward its backward follows."""
import functools
import importlib
import inspect
import pkgutil

import numpy as np
import pytest
import torch

import family_kit as K

BATCHES = (1, 3, 5)
BITS = None
# the bar between two schedules of one step in the family's own file (autograd against fused: allclose's rtol)
ASTGCNN_BAR = 1e-5          # tests/test_astgcnn_gpu.py:72
ST_CONV_BAR = 1e-5          # tests/test_stconv_gpu.py:77
FC_STGNN_BAR = 1e-4         # tests/test_fcstgnn_gpu.py:116


# ---- the rows --------------------------------------------------------------------------------------------------------------------------------
def _other_state(m):
    """Every floating tensor of the model's state dict but the running statistics, moved by uniform(-0.1, 0.1) under a fixed generator."""
    g = torch.Generator().manual_seed(4711)
    out = {}
    for k, v in m.state_dict().items():
        move = v.dtype.is_floating_point and "running_" not in k
        out[k] = v + torch.empty(v.shape, dtype=v.dtype).uniform_(-0.1, 0.1, generator=g).to(v.device) if move else v.clone()
    return out


def _make_opt(m):
    from gnn_rul_benchmarking_amd.optim import FusedAdam
    return FusedAdam(m, lr=1e-3, weight_decay=1e-4)


def _draw_like(x0):
    lo, hi, shape = float(np.min(x0)), float(np.max(x0)), tuple(np.shape(x0)[1:])

    @functools.lru_cache(maxsize=None)
    def draw(B, seed):
        rng = np.random.default_rng(seed)
        x = rng.uniform(lo, hi, (B,) + shape).astype(np.float32)
        return torch.from_numpy(x).to(K.DEV), torch.from_numpy(rng.uniform(0, 1, B).astype(np.float32)).to(K.DEV)
    return draw


def _adam_file_row(case, bar=BITS):
    """A family of tests/test_fused_adam_families_gpu.py: its builder (the family's smallest configuration, dropout at its own rate)
    and its ``_ready`` (train mode, the file's seed)."""
    def row():
        import test_fused_adam_families_gpu as A
        make, x, _ = A._families()[case][0]()
        return K.StaleCase(lambda: A._ready(make), _make_opt, _draw_like(x.numpy()), _other_state, {}, bar)
    return row


def _kit_row(gpu_file, golden_file, cases, dropout, theta=False, bar=BITS):
    """A family of tests/family_kit.py: ``build_model`` of its GPU file on the first fixture of its list, dropout at the family's rate."""
    def row():
        G, F = importlib.import_module(gpu_file), importlib.import_module(golden_file)
        z, cfg, sd = F.load_case(getattr(F, cases)[0])

        def ready():
            m = G.build_model(cfg, sd, dropout=dropout).train()
            m._seed = 20250131
            return m
        return K.StaleCase(ready, _make_opt, _draw_like(z["x"]), _other_state, {"theta": float(z["theta"])} if theta else {}, bar)
    return row


# family -> (row, batch sizes, calls)
TABLE = {
    "STMSGCN": (_adam_file_row("STMSGCN"), BATCHES, K.STALE_CALLS),
    "ASTGCNN": (_adam_file_row("ASTGCNN-generic-5x12", ASTGCNN_BAR), BATCHES, K.STALE_CALLS),
    "ST_Conv": (_adam_file_row("ST_Conv", ST_CONV_BAR), BATCHES, K.STALE_CALLS),
    "FC_STGNN": (_adam_file_row("FC_STGNN-fd004", FC_STGNN_BAR), BATCHES, K.STALE_CALLS),
    "STGNN": (_adam_file_row("STGNN"), BATCHES, K.STALE_CALLS),
    "RGCNU": (_adam_file_row("RGCNU"), BATCHES, K.STALE_CALLS),
    "STNet": (_adam_file_row("STNet"), BATCHES, K.STALE_CALLS),
    "SAGCN": (_adam_file_row("SAGCN"), BATCHES, K.STALE_CALLS),
    "STAGNN": (_adam_file_row("STAGNN"), BATCHES, K.STALE_CALLS),
    "AGCN_TF": (_adam_file_row("AGCN_TF"), BATCHES, K.STALE_CALLS),
    "GRU_CM": (_adam_file_row("GRU_CM"), BATCHES, K.STALE_CALLS),
    "HierCorrPool": (_kit_row("test_hiercorrpool_gpu", "test_hiercorrpool_oracle_golden", "CASES", 0.35), BATCHES, K.STALE_CALLS),
    "HierCorrPool_bearing": (_kit_row("test_hiercorrpool_bearing_gpu", "test_hiercorrpool_bearing_oracle_golden", "SMALL", 0.35),
                             BATCHES, K.STALE_CALLS),
    "LOGO": (_kit_row("test_logo_gpu", "test_logo_oracle_golden", "CASES", 0.2, theta=True), BATCHES, K.STALE_CALLS),
    "LOGO_bearing": (_kit_row("test_logo_bearing_gpu", "test_logo_bearing_oracle_golden", "SMALL", 0.2, theta=True), BATCHES, K.STALE_CALLS),
    "DVGTformer": (_kit_row("test_dvgtformer_gpu", "test_dvgtformer_oracle_golden", "SMALL", 0.1), BATCHES, K.STALE_CALLS),
    "GDAGDL": (_kit_row("test_gdagdl_gpu", "test_gdagdl_oracle_golden", "SMALL", 0.5), BATCHES, K.STALE_CALLS),
    "GAT_LSTM": (_kit_row("test_gatlstm_gpu", "test_gatlstm_oracle_golden", "SMALL", 0.2), BATCHES, K.STALE_CALLS),
    "STFA": (_kit_row("test_stfa_gpu", "test_stfa_oracle_golden", "SMALL", 0.2), BATCHES, K.STALE_CALLS),
}
# families that have no row yet, each with what failed (batch, fill, call and the observed difference)
NOT_YET = ()


def package_families():
    """The package's FlatModule / DropoutStepModule subclasses but ST_GCN's, under the registry's names (the class name without its
    ``_model`` / ``_RUL`` suffix), found by walking the package's modules."""
    import gnn_rul_benchmarking_amd as P
    from gnn_rul_benchmarking_amd.flat import DropoutStepModule, FlatModule
    names = set()
    for info in pkgutil.iter_modules(P.__path__):
        spec = info.module_finder.find_spec(f"{P.__name__}.{info.name}")
        if info.name in ("main", "build") or not str(spec.origin).endswith(".py"):     # a command line, the compiler driver, the library
            continue
        mod = importlib.import_module(f"{P.__name__}.{info.name}")
        for _, cls in inspect.getmembers(mod, inspect.isclass):
            if issubclass(cls, FlatModule) and cls not in (FlatModule, DropoutStepModule) and cls.__module__ == mod.__name__:
                names.add(cls.__name__.removesuffix("_model").removesuffix("_RUL"))
    return names - {"ST_GCN"}


def check_table_is_complete():
    assert not set(TABLE) & set(NOT_YET)
    assert set(TABLE) | set(NOT_YET) == package_families(), sorted((set(TABLE) | set(NOT_YET)) ^ package_families())
    for _, batches, calls in TABLE.values():
        assert batches and set(calls) <= set(K.STALE_CALLS) and "step" in calls


# ---- the tests ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_table_names_every_family_of_the_package():
    check_table_is_complete()


@functools.lru_cache(maxsize=None)
def _case(family):
    return TABLE[family][0]()


@functools.lru_cache(maxsize=None)
def _baseline(family, B, call):
    base = K.stale_run(_case(family), B, "zero", call)
    K.stale_baseline_ok(base, call)
    for v in base.values():
        v.setflags(write=False)
    return base


CASES = [pytest.param(f, B, fill, call, id=f"{f}-B{B}-{fill}-{call}")
         for f, (_, batches, calls) in TABLE.items() for B in batches for fill in K.STALE_FILLS[1:] for call in calls]


@pytest.mark.gpu
@pytest.mark.parametrize("family,B,fill,call", CASES)
def test_a_stale_workspace_does_not_reach_the_call(family, B, fill, call):
    case = _case(family)
    base = _baseline(family, B, call)
    K.stale_compare(base, K.stale_run(case, B, fill, call), fill, case.bar)


# ---- the epoch walk: workspaces evicted and allocated again, as a training epoch with ragged tails does ---------------------------------------
HPARAMS_ROWS = [("CMAPSS", "FD001"), ("CMAPSS", "FD002"), ("CMAPSS", "FD003"), ("CMAPSS", "FD004"), ("NCMAPSS", None),
                ("PHM2012", "Condition_1"), ("PHM2012", "Condition_2"), ("PHM2012", "Condition_3"),
                ("XJTU_SY", "Condition_1"), ("XJTU_SY", "Condition_2"), ("XJTU_SY", "Condition_3")]
WALK_BARS = {"ASTGCNN": ASTGCNN_BAR, "ST_Conv": ST_CONV_BAR, "FC_STGNN": FC_STGNN_BAR}
WALK_METHODS = ["ST_GCN", "STMSGCN", "ASTGCNN", "ST_Conv", "FC_STGNN", "STGNN", "RGCNU", "STNet", "SAGCN", "AGCN_TF", "HierCorrPool",
                "HierCorrPool_bearing", "LOGO", "LOGO_bearing", "STAGNN", "GRU_CM", "DVGTformer", "GDAGDL", "GAT_LSTM", "STFA"]
WALK_EXTRA_EVAL = (7, 6, 9, 10)          # one more evaluation batch size per workspace slot beyond three: the walk must evict


def fused_algorithms():
    """The registry's _FusedAlgorithm classes by name."""
    from gnn_rul_benchmarking_amd import algorithms as A
    return sorted(n for n, c in vars(A).items() if inspect.isclass(c) and issubclass(c, A._FusedAlgorithm) and not n.startswith("_"))


def first_hparams_row(method):
    """(model configs, training hparams, sample shape) of the first row of hparams.py that names ``method``."""
    from gnn_rul_benchmarking_amd.data_model_configs import get_dataset_class
    from gnn_rul_benchmarking_amd.hparams import get_hparams_class
    for dataset, did in HPARAMS_ROWS:
        h = get_hparams_class(dataset)(did)
        if method in h.alg_hparams:
            d = get_dataset_class(dataset)()
            return h.alg_hparams[method], h.train_params[method], (d.input_channels, d.sequence_len)
    raise AssertionError(f"no hparams row names {method}")


def _algo(method, seed):
    from gnn_rul_benchmarking_amd import algorithms as A
    cfg, hp, shape = first_hparams_row(method)
    torch.manual_seed(seed)
    a = getattr(A, method)(cfg, hp, K.DEV)                  # (the class itself: the registry refuses the two bearing names)
    a.to(K.DEV)
    a.train()
    return a, shape


def _walk_state(a):
    m, o = a.model, a.optimizer.state_dict()
    out = {"walk:bucket": m.bucket[:m.num_live + 1], "walk:flat_params": m.flat_params, "walk:exp_avg": o["exp_avg"],
           "walk:exp_avg_sq": o["exp_avg_sq"]}
    out.update({"walk:sd:" + k: v for k, v in m.state_dict().items()})
    return {k: v.detach().cpu().numpy().copy() for k, v in out.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("method", WALK_METHODS)
def test_a_step_after_an_epoch_walk_equals_the_step_of_a_fresh_algorithm(method):
    """update at 5, 5, 3, eval forwards at 4 and 2 (and one more size per workspace slot beyond three; further updates where the eval
    forward keeps no workspace), update at 5 again: the last update runs on a workspace the allocator handed back after an eviction.  A fresh algorithm given the first one's parameters,
    buffers, optimizer state, seed and step (tests/test_param_changes_between_steps_gpu.py::_fresh_like) takes only that update."""
    a, shape = _algo(method, 31)
    slots = a.model.workspace_slots
    g = torch.Generator(device=K.DEV).manual_seed(5)
    batch = lambda n: (torch.rand(n, *shape, device=K.DEV, generator=g), torch.rand(n, 1, device=K.DEV, generator=g))    # noqa: E731
    held = []
    for n in (5, 5, 3):
        assert np.isfinite(a.update(*batch(n), 1)["loss"])
        held.append(len(a.model._bufs))
    a.eval()
    with torch.no_grad():
        for n in (4, 2) + WALK_EXTRA_EVAL[:max(0, slots - 3)]:
            a.model(batch(n)[0])
            held.append(len(a.model._bufs))
    a.train()
    for n in WALK_EXTRA_EVAL:                                # (ST_GCN's eval forward keeps no training workspace: further updates evict)
        if 5 not in a.model._bufs:
            break
        assert np.isfinite(a.update(*batch(n), 1)["loss"])
        held.append(len(a.model._bufs))
    assert max(held) <= slots and 5 not in a.model._bufs, "the walk evicted nothing: it tested nothing"
    c, _ = _algo(method, 99)
    c.model.load_state_dict({k: v.clone() for k, v in a.model.state_dict().items()})
    c.optimizer.load_state_dict(a.optimizer.state_dict())
    for k in ("_seed", "_step"):
        if hasattr(a.model, k):
            setattr(c.model, k, getattr(a.model, k))
    X, y = batch(5)
    la, lc = a.update(X, y, 1)["loss"], c.update(X, y, 1)["loss"]
    want, got = _walk_state(c), _walk_state(a)
    want["walk:loss"], got["walk:loss"] = np.asarray(lc, np.float32), np.asarray(la, np.float32)
    K.stale_baseline_ok(want, "step")
    want["filled:walk"], got["filled:walk"] = np.asarray(0), np.asarray(1)          # (the eviction asserted above stands for the fill)
    K.stale_compare(want, got, "walk", WALK_BARS.get(method))


@pytest.mark.gpu
def test_the_walk_names_every_fused_algorithm_of_the_registry():
    assert sorted(WALK_METHODS) == fused_algorithms()


# ---- HAGCN: no cached workspace, so through the C entries on a workspace this file owns (ws_step of tests/test_train_mx_hrec_gpu.py) ------------
HAGCN_CASES = {"bilstm-Bq1-T1-H64": (1, 1, 4, 64), "bilstm-Bq2-T9-H60": (2, 9, 7, 60),        # tests/test_bilstm_group_gpu.py::GROUP_CASES
               "graph-N10-enc7-hid8-G5": (10, 7, 8, 5)}                                          # the smallest of tests/test_hagcn_gpu.py


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=K.DEV)


def _randn(rng, *shape):
    return torch.from_numpy(rng.normal(size=shape).astype(np.float32)).to(K.DEV)


def _bilstm_call(ws, dims, seed):
    """rulgnn_bilstm_forward_f32 + rulgnn_bilstm_backward_f32 of one layer drawn under ``seed``, on ``ws``: every output, NaN before."""
    import ctypes as C
    from gnn_rul_benchmarking_amd import _lib
    Bq, T, I, H = dims
    rng = np.random.default_rng(seed)
    w = [[_randn(rng, 4 * H, I) * 0.3, _randn(rng, 4 * H, H) * 0.3, _randn(rng, 4 * H) * 0.3, _randn(rng, 4 * H) * 0.3] for _ in range(2)]
    x, dout = _randn(rng, Bq, T, I), _randn(rng, Bq, T, H)
    out, dx, g = _nan(Bq, T, H), _nan(Bq, T, I), [[_nan(*t.shape) for t in d] for d in w]
    shp, a, st = _lib.BilstmShape(T, Bq, I, H), _lib.BilstmArgs(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    a.x, a.out, a.dout, a.dx = x.data_ptr(), out.data_ptr(), dout.data_ptr(), dx.data_ptr()
    for d in range(2):
        a.w_ih[d], a.w_hh[d], a.b_ih[d], a.b_hh[d] = (t.data_ptr() for t in w[d])
        a.dw_ih[d], a.dw_hh[d], a.db_ih[d], a.db_hh[d] = (t.data_ptr() for t in g[d])
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    _lib.check(_lib.load().rulgnn_bilstm_forward_f32(C.byref(shp), C.byref(a), st), "rulgnn_bilstm_forward_f32")
    _lib.check(_lib.load().rulgnn_bilstm_backward_f32(C.byref(shp), C.byref(a), st), "rulgnn_bilstm_backward_f32")
    torch.cuda.synchronize()
    res = {"hagcn:out": out, "hagcn:dx": dx, **{f"hagcn:grad{d}{i}": g[d][i] for d in range(2) for i in range(4)}}
    return {k: v.cpu().numpy() for k, v in res.items()}


def _graph_call(ws, dims, seed):
    """rulgnn_hagcn_graph_forward_f32 + ..._backward_f32 of a graph stack drawn under ``seed``, on ``ws``: every output, NaN before."""
    import ctypes as C
    from gnn_rul_benchmarking_amd import _lib
    from gnn_rul_benchmarking_amd.hagcn import HAGCN_model
    from oracle import hagcn_oracle as O
    N, enc, hid, G = dims
    rng = np.random.default_rng(seed)
    m = HAGCN_model(patch_size=5, num_patch=1, encoder_hidden_dim=enc, hidden_dim=hid, output_dim=4)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in O.random_graph_params(enc, hid, seed=seed).items()}, strict=False)
    m = m.to(K.DEV)
    nodes, dfeats, dkl = _randn(rng, G, N, enc), _randn(rng, G, 3 * hid), torch.full((1,), 7.0, device=K.DEV)
    feats, kl, dnodes, grads = _nan(G, 3 * hid), _nan(1), _nan(G, N, enc), _nan(m._count)
    topk = torch.full((G, _lib.HAGCN_TOPK_SLOTS), -1, dtype=torch.int32, device=K.DEV)
    shp, a, st = _lib.HagcnShape(G, N, enc, hid), _lib.HagcnArgs(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    a.nodes, a.params, a.feats, a.kl, a.topk = nodes.data_ptr(), m._flat.data_ptr(), feats.data_ptr(), kl.data_ptr(), topk.data_ptr()
    a.dfeats, a.dkl, a.dnodes, a.grads = dfeats.data_ptr(), dkl.data_ptr(), dnodes.data_ptr(), grads.data_ptr()
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    _lib.check(_lib.load().rulgnn_hagcn_graph_forward_f32(C.byref(shp), C.byref(a), st), "rulgnn_hagcn_graph_forward_f32")
    _lib.check(_lib.load().rulgnn_hagcn_graph_backward_f32(C.byref(shp), C.byref(a), st), "rulgnn_hagcn_graph_backward_f32")
    torch.cuda.synchronize()
    res = {"hagcn:feats": feats, "hagcn:kl": kl, "hagcn:topk": topk, "hagcn:dnodes": dnodes, "hagcn:grad": grads}
    return {k: v.cpu().numpy() for k, v in res.items()}


def _hagcn_run(case, fill):
    import ctypes as C
    from gnn_rul_benchmarking_amd import _lib
    dims = HAGCN_CASES[case]
    if case.startswith("bilstm"):
        Bq, T, I, H = dims
        nbytes, call = _lib.load().rulgnn_bilstm_workspace_bytes(C.byref(_lib.BilstmShape(T, Bq, I, H))), _bilstm_call
    else:
        N, enc, hid, G = dims
        nbytes, call = _lib.load().rulgnn_hagcn_workspace_bytes(C.byref(_lib.HagcnShape(G, N, enc, hid))), _graph_call
    assert nbytes > 0 and nbytes % 4 == 0
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=K.DEV)
    if fill == "nan":
        ws.view(torch.int32).fill_(K.QUIET_NAN)
    elif fill == "same-batch":
        call(ws, dims, 77)                       # forward + backward of another layer / stack on other data: what they left stays
    else:
        assert fill == "zero"
    out = {"filled:1": np.asarray(int(torch.count_nonzero(ws.view(torch.int32))))}
    out.update(call(ws, dims, 5))
    return out


@functools.lru_cache(maxsize=None)
def _hagcn_baseline(case):
    base = _hagcn_run(case, "zero")
    K.stale_baseline_ok(base, "step")
    assert any(v.any() for k, v in base.items() if "grad" in k)          # (T = 1: h_prev = 0, the recurrent weights' gradient is zero)
    return base


@pytest.mark.gpu
@pytest.mark.parametrize("fill", ["nan", "same-batch"])
@pytest.mark.parametrize("case", list(HAGCN_CASES))
def test_hagcn_entries_on_a_stale_workspace(case, fill):
    K.stale_compare(_hagcn_baseline(case), _hagcn_run(case, fill), fill, BITS)
