"""The host-only answers of the library -- workspace sizes, parameter counts and the codes the C entries return for bad argument
sets -- against tests/golden/host_plumbing.json, which the library built from the parent commit wrote
(tests/golden/make_host_plumbing_golden.py).  Nothing here launches a kernel."""
import importlib.util
import json
import os

import pytest
import torch

from gnn_rul_benchmarking_amd import _lib

from conftest import ROOT

_GEN = os.path.join(ROOT, "tests", "golden", "make_host_plumbing_golden.py")
_spec = importlib.util.spec_from_file_location("make_host_plumbing_golden", _GEN)
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

_no_gpu = pytest.mark.skipif(torch.cuda.is_available(),
                             reason="placeholder device pointers: an argument set that got through would launch kernels on them")


@pytest.fixture(scope="module")
def golden():
    with open(gen.GOLDEN) as f:
        g = json.load(f)
    return {"parent_commit": g["parent_commit"], "sizes": gen.unpack(g["sizes"]), "codes": gen.unpack(g["codes"])}


@pytest.fixture(scope="module")
def current():
    return gen.collect(_lib.load(), codes=not torch.cuda.is_available())


def _groups(section):
    with open(gen.GOLDEN) as f:
        return sorted({k.split("/")[0] for k in json.load(f)[section]})


def _compare(want, got, group):
    want = {k: v for k, v in want.items() if k.split("/")[0] == group}
    got = {k: v for k, v in got.items() if k.split("/")[0] == group}
    assert want, group
    assert sorted(got) == sorted(want), "the case list changed: regenerate the golden from the parent commit"
    diff = {k: (want[k], got[k]) for k in want if want[k] != got[k]}
    assert not diff, f"{len(diff)} of {len(want)} differ from the parent (parent, now): {dict(list(diff.items())[:8])}"


def test_golden_names_its_parent_commit(golden):
    assert len(golden["parent_commit"]) == 40 and int(golden["parent_commit"], 16) >= 0
    assert len(golden["sizes"]) > 1200 and len(golden["codes"]) > 1650


@pytest.mark.parametrize("group", _groups("sizes"))
def test_workspace_sizes_and_counts_equal_the_parents(golden, current, group):
    # (runs with a GPU too: the golden was written at the library's compute-unit fallback of 256, the MI355X's own count)
    _compare(golden["sizes"], current["sizes"], group)


@_no_gpu
@pytest.mark.parametrize("group", _groups("codes"))
def test_return_codes_equal_the_parents(golden, current, group):
    _compare(golden["codes"], current["codes"], group)
