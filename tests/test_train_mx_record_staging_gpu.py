"""-m gpu: the full-tile records of the matrix-core training chain (csrc/stgcn_train_mx.hip: X_l, Q_l, H_l, d(x0 + H), d X_l) are staged in
LDS where they are produced and stored one tile late.  That path changes no arithmetic, no summation order and no byte that reaches
memory, so at every shape where the staging can go wrong the step must give, bit for bit, what the library of the commit before the
rework gave (tests/golden/train_mx_record_stores.npz, written by tests/golden/make_golden_train_mx_record_stores.py, whose cases and
runner this test imports): the loss, every gradient after one step, every parameter and BatchNorm buffer after three fused-Adam steps.
Each case runs twice in one process and the two runs must be equal as well."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_train_mx_record_stores as M  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ["b1", "b3", "b4", "b5", "multi2", "multi3", "multi2_nodrop", "n15_multi2", "n15_multi3", "n9_multi2", "n9_multi3",
         "layers1_multi2", "layers3_multi2", "single_launch", "single_launch_n9"]
KEYS = ("loss", "grads", "params_after", "bn_after")


@pytest.fixture(scope="module")
def golden():
    with np.load(M.FIXTURE) as z:
        return {k: z[k] for k in z.files}


def test_the_case_list_is_the_fixtures():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert [c[0] for c in M.cases(cus)] == NAMES


@pytest.mark.parametrize("name", NAMES)
def test_record_stores_bitwise_against_the_parent(name, golden):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    # the multi-tile batches are sized from the phase grid: the fixture holds them for the device it was written on
    assert int(golden["cus"]) == cus, f"fixture written on {int(golden['cus'])} CUs, this device has {cus}: regenerate it from the parent commit"
    case = next(c for c in M.cases(cus) if c[0] == name)
    first, second = M.run_case(case), M.run_case(case)
    keys = KEYS + (("pred",) if f"{name}:pred" in golden else ())
    for k in keys:
        a, b, want = first[k], second[k], golden[f"{name}:{k}"]
        assert a.dtype == want.dtype and a.shape == want.shape, (name, k)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (name, k, "two runs differ")
        assert np.array_equal(a.view(np.uint32), want.view(np.uint32)), (name, k, "differs from the parent",
                                                                          int(np.count_nonzero(a.view(np.uint32) != want.view(np.uint32))))
