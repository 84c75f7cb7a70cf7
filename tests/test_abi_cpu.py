"""CPU-side checks of the C-ABI library: it loads, exports every symbol include/rulgnn.h declares,
and its host-only entry points behave (no kernels are launched here)."""
import ctypes as C
import os
import re

import pytest
import torch

from gnn_rul_benchmarking_amd import _lib, build, params as PL

from conftest import ROOT


def test_library_builds_and_loads():
    build.build()
    lib = _lib.load()
    assert lib.rulgnn_version() >= 100


def test_every_declared_symbol_is_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "rulgnn.h")).read()
    declared = set(re.findall(r"\b(rulgnn_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.EXPORTED_SYMBOLS)
    raw = C.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), name


def _struct_defines():
    """{index: define suffix} of the ``#define RULGNN_STRUCT_<X> <n>`` lines of include/rulgnn.h."""
    hdr = open(os.path.join(ROOT, "include", "rulgnn.h")).read()
    found = re.findall(r"^#define RULGNN_STRUCT_(\w+) (\d+)\s*$", hdr, re.M)
    table = {int(n): suffix for suffix, n in found}
    assert len(table) == len(found), "two RULGNN_STRUCT_* constants share an index"
    return table


def test_struct_table_is_the_headers():
    assert set(_struct_defines()) == set(_lib.STRUCTS)


def test_struct_size_answers_the_mirror_and_zero_elsewhere():
    lib = _lib.load()
    for which in range(-2, max(_lib.STRUCTS) + 8):
        mirror = _lib.STRUCTS.get(which)
        assert lib.rulgnn_struct_size(which) == (C.sizeof(mirror) if mirror is not None else 0), which


def _c_compiler():
    """The system C compiler; without one, the host compiler hipcc drives (the library cannot have been built without it)."""
    import shutil
    if shutil.which("cc"):
        return shutil.which("cc")
    clang = os.path.join(os.path.dirname(os.path.realpath(build._hipcc())), "..", "lib", "llvm", "bin", "clang")
    assert os.access(clang, os.X_OK), "no C compiler: neither cc nor hipcc's clang"
    return clang


def test_every_mirror_field_sits_where_the_header_puts_it(tmp_path):
    """sizeof and offsetof of every field of every mirror, as a C99 compiler reads include/rulgnn.h, against ctypes.  The C struct of
    ``RULGNN_STRUCT_<X>`` is ``rulgnn_<x>``."""
    import subprocess
    lines, want = ['#include <stdio.h>', '#include <stddef.h>', '#include "rulgnn.h"', 'int main(void) {'], []
    for which, suffix in sorted(_struct_defines().items()):
        mirror, cname = _lib.STRUCTS[which], "rulgnn_" + suffix.lower()
        lines.append(f'    printf("{which} sizeof %zu\\n", sizeof({cname}));')
        want.append(f"{which} sizeof {C.sizeof(mirror)}")
        for field, _ in mirror._fields_:
            lines.append(f'    printf("{which} {field} %zu\\n", offsetof({cname}, {field}));')
            want.append(f"{which} {field} {getattr(mirror, field).offset}")
    lines += ['    return 0;', '}']
    src, exe = tmp_path / "offsets.c", tmp_path / "offsets"
    src.write_text("\n".join(lines) + "\n")
    cc = subprocess.run([_c_compiler(), "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    got = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert got.returncode == 0, got.stderr
    assert len(want) > 480
    assert got.stdout.splitlines() == want


def test_param_count_and_layout_agree_with_library():
    lib = _lib.load()
    for N, L in [(14, 2), (40, 2), (16, 3), (2, 1)]:
        assert lib.rulgnn_stgcn_param_count(N, L) == PL.param_count(N, L)
        for k in (1, 2, 3):
            assert lib.rulgnn_stgcn_param_count_order(N, L, k) == PL.param_count(N, L, k)
        lay = PL.live_param_layout(N, L)
        last_off, last_shape = list(lay.values())[-1]
        assert last_off + 1 == PL.param_count(N, L)
    assert PL.param_count(14, 2) == 1525       # 1,525 live parameters


def test_error_codes_have_messages():
    for code in (0, -1, -2, -3, -4, -5):
        assert "unknown" not in _lib.strerror(code)
    assert "unknown" in _lib.strerror(-99)


def test_shape_validation_without_gpu():
    lib = _lib.load()
    bad = _lib.StgcnShape(4, 8192, 32, 2, 1)          # beyond every path
    assert lib.rulgnn_stgcn_forward_f32(C.byref(bad), None, None, None, None, None, 0, None) == -2
    big = _lib.StgcnShape(4, 1024, 32, 2, 1)          # XJTU-sized num_patch: tiled path, needs a workspace
    assert lib.rulgnn_stgcn_forward_workspace_bytes(C.byref(big)) > 0
    assert lib.rulgnn_stgcn_forward_workspace_bytes(C.byref(_lib.StgcnShape(4, 14, 30, 2, 1))) == 0
    bad = _lib.StgcnShape(4, 14, 30, 2, 4)            # MPNN order: 1..3 (2, 3 on the row-mapped kernels, num_patch <= 64)
    assert lib.rulgnn_stgcn_forward_f32(C.byref(bad), None, None, None, None, None, 0, None) == -2
    assert lib.rulgnn_stgcn_forward_f32(C.byref(_lib.StgcnShape(4, 160, 16, 2, 2)), None, None, None, None, None, 0, None) == -2
    # k > 1 on a shape the fused kernels cannot hold (a 4096-point window; four layers) must not fall through to the tiled kernels
    for shp in (_lib.StgcnShape(4, 14, 4096, 2, 2), _lib.StgcnShape(4, 14, 30, 4, 2)):
        assert lib.rulgnn_stgcn_train_workspace_bytes(C.byref(shp)) == 0
    assert lib.rulgnn_stgcn_forward_f32(C.byref(_lib.StgcnShape(4, 14, 4096, 2, 2)), None, None, None, None, None, 0, None) == -2
    assert lib.rulgnn_stgcn_train_workspace_bytes(C.byref(_lib.StgcnShape(4, 14, 4096, 2, 1))) > 0
    assert lib.rulgnn_stgcn_forward_f32(C.byref(_lib.StgcnShape(4, 14, 30, 2, 0)), None, None, None, None, None, 0, None) == -1
    assert lib.rulgnn_stgcn_forward_f32(C.byref(_lib.StgcnShape(4, 14, 30, 2, 3)), None, None, None, None, None, 0, None) == -1   # valid shape, null pointers
    ok = _lib.StgcnShape(4, 14, 30, 2, 1)
    assert lib.rulgnn_stgcn_forward_f32(C.byref(ok), None, None, None, None, None, 0, None) == -1   # null pointers
    empty = _lib.StgcnShape(0, 14, 30, 2, 1)
    assert lib.rulgnn_stgcn_forward_f32(C.byref(empty), None, None, None, None, None, 0, None) == 0  # empty batch is a no-op


def test_single_hip_runtime_even_when_library_is_loaded_before_torch():
    """Regression: loading librulgnn.so before torch used to map /opt/rocm's libamdhip64 next to the
    one bundled with torch (two HIP runtimes -> every launch on a torch stream failed)."""
    import subprocess
    import sys
    code = "\n".join([
        "import sys, os; sys.path.insert(0, %r)" % ROOT,
        "from gnn_rul_benchmarking_amd import _lib",
        "_lib.load()",
        "import torch",
        "libs = {l.split()[-1] for l in open('/proc/self/maps') if 'libamdhip64' in l}",
        "print(len({os.path.realpath(p) for p in libs}))"])
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == "1", out.stdout


# (family, dataset, dataset id, C entry prefix, argument struct): the fwdbwd entries whose rulgnn_adam_args validation is pinned below
_FWDBWD_FAMILIES = [("STGNN", "CMAPSS", "FD004", "stgnn", _lib.StmsgcnArgs), ("STNet", "PHM2012", "Condition_1", "stnet", _lib.StnetArgs),
                    ("SAGCN", "PHM2012", "Condition_2", "sagcn", _lib.SagcnArgs), ("RGCNU", "CMAPSS", "FD004", "rgcnu", _lib.RgcnuArgs),
                    ("STAGNN", "CMAPSS", "FD001", "stagnn", _lib.StagnnArgs), ("ST_Conv", "CMAPSS", "FD004", "stconv", _lib.AstgcnnArgs),
                    ("STMSGCN", "XJTU_SY", "Condition_1", "stmsgcn", _lib.StmsgcnArgs),
                    ("FC_STGNN", "CMAPSS", "FD004", "fcstgnn", _lib.FcstgnnArgs), ("ASTGCNN", "NCMAPSS", None, "astgcnn", _lib.AstgcnnArgs)]
_BN_OPT_FAMILIES = ("ST_Conv", "FC_STGNN", "ASTGCNN")          # their entries also check opt->bn_stats


@pytest.mark.skipif(torch.cuda.is_available(),
                    reason="placeholder device pointers: a case that got through would launch kernels on them")
@pytest.mark.parametrize("family,ds,did,prefix,Args", _FWDBWD_FAMILIES)
def test_fwdbwd_rejects_bad_adam_arguments_before_any_launch(family, ds, did, prefix, Args):
    """Every rulgnn_<family>_fwdbwd_f32 validates its rulgnn_adam_args the same way, in the same order, before any launch: the step
    (or a device step state) and ``opt->params == args->params`` first, then null / misaligned optimizer pointers (EINVAL / EALIGN),
    then -- BatchNorm families -- ``opt->bn_stats``.  Every other argument is a valid placeholder, so the codes come from that check."""
    from gnn_rul_benchmarking_amd.algorithms import get_algorithm_class
    from gnn_rul_benchmarking_amd.hparams import get_hparams_class
    h = get_hparams_class(ds)(did)
    model = get_algorithm_class(family)(h.alg_hparams[family], h.train_params[family], "cpu").model
    lib = _lib.load()
    entry = getattr(lib, f"rulgnn_{prefix}_fwdbwd_f32")
    B, base = 4, 1 << 20
    shp = model._shape(B)
    a = Args()
    for i, (name, ctype) in enumerate(a._fields_):
        if ctype is C.c_void_p and name not in ("dpred", "recon_weight", "step_state", "aux_stream"):
            setattr(a, name, base + 256 * i)
    a.workspace_bytes, a.global_batch = 1 << 40, B
    if hasattr(a, "training"):
        a.training = 1

    def code(**opt):
        o = _lib.AdamArgs(a.params, base + 65536, base + 131072, None, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.1, None)
        for k, v in opt.items():
            setattr(o, k, v)
        return entry(C.byref(shp), C.byref(a), C.byref(o), None)

    EINVAL, EALIGN = _lib.EINVAL, _lib.EALIGN
    assert code(step=0) == EINVAL                                        # no step and no device step state
    assert code(params=a.params + 4) == EINVAL                           # an optimizer over other parameters
    assert code(params=None) == EINVAL
    assert code(exp_avg=None) == EINVAL
    assert code(exp_avg_sq=None) == EINVAL
    assert code(exp_avg=base + 65538) == EALIGN
    assert code(exp_avg_sq=base + 131074) == EALIGN
    assert code(step=0, step_state=base + 196608, exp_avg=base + 65538) == EALIGN     # a device step state stands in for the step
    assert code(step=0, exp_avg=base + 65538) == EINVAL                  # the step check fires before the pointer checks
    assert code(params=a.params + 4, exp_avg=None) == EINVAL
    if family in _BN_OPT_FAMILIES:
        assert code(bn_stats=base + 196610) == EINVAL                    # misaligned running statistics
        assert code(bn_stats=base + 196610, exp_avg=base + 65538) == EALIGN


# The gates at the edges of the fused row-mapped kernels' LDS budget (tests/test_stgcn_lds_envelope_gpu.py runs these shapes): each
# pair is the last window one launch form holds and the first it does not.  eval: "fused" (no workspace), "tiled" (a workspace) or
# "refused" (order k > 1: -2 before any launch); training: "chain" (the phase chains), "tiled" or "refused".
_LDS_EDGE = [
    # eval, exact row-mapped kernel, order 1 (an order-1 shape past the edge goes to the tiled path)
    (33, 207, 2, 1, "fused", "tiled"), (33, 208, 2, 1, "tiled", "tiled"),
    (40, 171, 2, 1, "fused", "tiled"), (40, 172, 2, 1, "tiled", "tiled"),
    (47, 146, 2, 1, "fused", "tiled"), (47, 147, 2, 1, "tiled", "tiled"),
    (48, 143, 2, 1, "fused", "tiled"), (48, 144, 2, 1, "tiled", "tiled"),
    (64, 107, 2, 1, "fused", "tiled"), (64, 108, 2, 1, "tiled", "tiled"),
    (17, 219, 8, 1, "fused", "tiled"), (17, 220, 8, 1, "tiled", "tiled"), (32, 115, 8, 1, "fused", "tiled"), (32, 116, 8, 1, "tiled", "tiled"),
    # the wide matrix-core eval shapes past the edge: not the wide kernel (its scan would not fit) but the tiled path
    (40, 200, 2, 1, "tiled", "tiled"), (47, 190, 2, 1, "tiled", "tiled"),
    # training, fp32 phase chain, order 1 (41 x 132 and 40 x 136 qualify for the wide matrix-core chain, but a guard retry would land on
    # the fp32 chain: the tiled path)
    (41, 131, 2, 1, "fused", "chain"), (41, 133, 2, 1, "fused", "tiled"), (41, 132, 2, 1, "fused", "tiled"),
    (40, 135, 2, 1, "fused", "chain"), (40, 136, 2, 1, "fused", "tiled"),
    (48, 111, 2, 1, "fused", "chain"), (48, 112, 2, 1, "fused", "tiled"), (64, 83, 2, 1, "fused", "chain"), (64, 84, 2, 1, "fused", "tiled"),
    # order 2, 3: refused up front
    (17, 255, 2, 2, "fused", "chain"), (17, 256, 2, 2, "refused", "chain"),
    (40, 115, 2, 2, "fused", "chain"), (40, 116, 2, 2, "refused", "chain"), (40, 135, 2, 2, "refused", "chain"), (40, 136, 2, 2, "refused", "refused"),
    (64, 71, 2, 2, "fused", "chain"), (64, 72, 2, 2, "refused", "chain"), (64, 83, 2, 2, "refused", "chain"), (64, 84, 2, 2, "refused", "refused"),
    (17, 198, 2, 3, "fused", "chain"), (17, 199, 2, 3, "fused", "refused"), (17, 239, 2, 3, "fused", "refused"), (17, 240, 2, 3, "refused", "refused"),
    (17, 203, 1, 3, "fused", "chain"), (17, 204, 1, 3, "fused", "refused"),
    (40, 63, 2, 3, "fused", "chain"), (40, 64, 2, 3, "refused", "chain"), (40, 83, 2, 3, "refused", "chain"), (40, 84, 2, 3, "refused", "refused"),
    (64, 39, 2, 3, "fused", "chain"), (64, 40, 2, 3, "refused", "chain"), (64, 51, 2, 3, "refused", "chain"), (64, 52, 2, 3, "refused", "refused"),
    # every benchmarked shape stays where it was
    (14, 30, 2, 1, "fused", "chain"), (14, 50, 2, 1, "fused", "chain"), (40, 64, 2, 1, "fused", "chain"),
    (160, 16, 2, 1, "tiled", "tiled"), (1024, 32, 2, 1, "tiled", "tiled"),
]


@pytest.mark.parametrize("N,P,L,k,ev,tr", _LDS_EDGE)
def test_stgcn_gates_at_the_lds_edge(N, P, L, k, ev, tr):
    """Host-only: the workspace queries, the null-pointer forward call and rulgnn_stgcn_train_step_resolve agree on which path a shape
    takes -- and so which calls must run and which are refused before anything is launched."""
    lib = _lib.load()
    shp = _lib.StgcnShape(7, N, P, L, k)
    x = C.c_void_p(1 << 20)                     # 16-byte aligned placeholder: resolve only looks at its alignment
    fwd_ws = lib.rulgnn_stgcn_forward_workspace_bytes(C.byref(shp))
    fwd_rc = lib.rulgnn_stgcn_forward_f32(C.byref(shp), None, None, None, None, None, 0, None)
    assert (fwd_ws > 0, fwd_rc) == {"fused": (False, _lib.EINVAL), "tiled": (True, _lib.EINVAL), "refused": (False, _lib.EUNSUPPORTED)}[ev]
    train_ws = lib.rulgnn_stgcn_train_workspace_bytes(C.byref(shp))
    guard = lib.rulgnn_stgcn_train_guard_counter_offset(C.byref(shp))
    auto = lib.rulgnn_stgcn_train_step_resolve(C.byref(shp), x, _lib.STEP_AUTO)
    chain = lib.rulgnn_stgcn_train_step_resolve(C.byref(shp), x, _lib.STEP_CHAIN)
    if tr == "chain":
        assert train_ws > 0 and guard >= 0 and chain == _lib.STEP_CHAIN
        # the matrix-core chains where they apply: num_patch <= 47 and num_patch x patch_size a multiple of 4
        assert auto == (_lib.STEP_MX if N <= 47 and k == 1 and (N * P) % 4 == 0 else _lib.STEP_CHAIN)
    else:
        assert (train_ws > 0) == (tr == "tiled")
        assert guard == -1 and auto == chain == _lib.EUNSUPPORTED
