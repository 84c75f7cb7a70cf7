"""Golden results of the matrix-core ST_GCN training chain at the shapes where the staging of its full-tile records can go wrong
(tests/test_train_mx_record_staging_gpu.py), written by the library of the commit BEFORE the record stores were reworked: the rework
changes no arithmetic, no summation order and no byte that reaches memory, so every result must stay bitwise what it was.

    RULGNN_LIB=<library built from the parent commit> python tests/golden/make_golden_train_mx_record_stores.py <parent commit hash> [output file]

Needs the GPU the test will run on: two of the batches are sized from the phase grid the launcher chooses (two workgroups per CU), so
that every wavefront carries two or three tiles.  Inputs and weights are generated from seeds (`run_case`, which the test imports); the
fixture holds, per case, the loss, every gradient after one step, and the parameters and BatchNorm buffers after three fused-Adam
steps."""
import ctypes as C
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

from gnn_rul_benchmarking_amd import _lib, params as PL  # noqa: E402
from oracle import stgcn_oracle as O  # noqa: E402

FIXTURE = os.path.join(HERE, "train_mx_record_stores.npz")
MXT_WAVES = 4          # wavefronts per workgroup, four samples per wavefront tile (csrc/stgcn_train_mx_ops.hpp)
ADAM_STEPS = 3


def phase_grid(cus):
    """Workgroups of a phase launch at a batch that fills the device: two per CU (mxt_launch, csrc/stgcn_train_mx.hip)."""
    return 2 * cus


def cases(cus):
    """(name, N, P, B, L, dropout, path).  `multi2` / `multi3`: every wavefront of the phase grid carries two / three tiles (the pending
    record, the re-use of the staging tile, the drain behind the loop) and the last tile is partial."""
    g = phase_grid(cus)
    multi2, multi3 = 4 * MXT_WAVES * g * 2 + 5, 4 * MXT_WAVES * g * 3 + 1
    out = [(f"b{b}", 14, 30, b, 2, 0.2, _lib.STEP_MX) for b in (1, 3, 4, 5)]           # partial and full single tiles, nothing pending
    out += [("multi2", 14, 30, multi2, 2, 0.2, _lib.STEP_MX), ("multi3", 14, 30, multi3, 2, 0.2, _lib.STEP_MX),
            ("multi2_nodrop", 14, 30, multi2, 2, 0.0, _lib.STEP_MX)]
    for n, p in ((15, 16), (9, 20)):                                                    # the generic body: 10 N pieces, no multiple of 64
        out += [(f"n{n}_multi2", n, p, multi2, 2, 0.2, _lib.STEP_MX), (f"n{n}_multi3", n, p, multi3, 2, 0.2, _lib.STEP_MX)]
    out += [("layers1_multi2", 14, 30, multi2, 1, 0.2, _lib.STEP_MX),                   # TOP reads H_0
            ("layers3_multi2", 14, 30, multi2, 3, 0.2, _lib.STEP_MX)]                   # F_4 / G_4
    out += [("single_launch", 14, 30, 1027, 2, 0.2, _lib.STEP_MX_PERSIST),              # the opt-in persistent launch
            ("single_launch_n9", 9, 20, 100, 2, 0.2, _lib.STEP_MX_PERSIST)]
    return out


def run_case(case):
    """One forward + backward step, then ADAM_STEPS fused-Adam steps from the same start, through the C-ABI on cuda:0."""
    import gpu_util as G
    name, N, P, B, L, p, path = case
    lib = _lib.load()
    dev = torch.device("cuda:0")
    seed = sum(map(ord, name)) + 1000 * N + L
    rng = np.random.default_rng(seed)
    flat, _ = PL.pack_numpy(O.random_params(N, L, seed=seed % 97), N, L)
    x = torch.from_numpy(rng.uniform(0, 1, (B, N * P)).astype(np.float32)).to(dev)
    y = torch.from_numpy(rng.uniform(0, 1, (B,)).astype(np.float32)).to(dev)
    shp = G.shape_struct(B, N, P, L)
    nbytes = lib.rulgnn_stgcn_train_workspace_bytes(C.byref(shp))
    out = {}

    def step(prm, opt, k):
        grads = torch.full_like(prm, float("nan"))
        pred = torch.full((B,), float("nan"), device=dev)
        loss = torch.full((1,), float("nan"), device=dev)
        bnb = torch.full((L * 2 * 2 * 10,), float("nan"), device=dev)
        ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        a = _lib.StgcnTrainArgs()
        a.x = x.data_ptr(); a.y = y.data_ptr(); a.dpred = None
        a.params = prm.data_ptr(); a.grads = grads.data_ptr(); a.pred = pred.data_ptr(); a.loss = loss.data_ptr()
        a.bn_batch = bnb.data_ptr(); a.workspace = ws.data_ptr(); a.workspace_bytes = nbytes
        a.global_batch = B; a.sample_offset = 0
        a.dropout_p = p; a.seed = 99; a.step = k
        rc = lib.rulgnn_stgcn_train_step_path_f32(C.byref(shp), C.byref(a), opt, path, G.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0, (name, rc)
        return loss.cpu().numpy(), grads.cpu().numpy(), pred.cpu().numpy()

    prm = torch.from_numpy(flat.copy()).to(dev)
    out["loss"], out["grads"], out["pred"] = step(prm, None, 1)
    m, v = torch.zeros_like(prm), torch.zeros_like(prm)
    bn = torch.zeros(L * 2 * 2 * 10, device=dev)
    for k in range(1, ADAM_STEPS + 1):
        opt = _lib.AdamArgs(prm.data_ptr(), m.data_ptr(), v.data_ptr(), bn.data_ptr(), k, 1e-3, 0.9, 0.999, 1e-8, 1e-4, 0.1, None)
        step(prm, C.byref(opt), k)
    out["params_after"], out["bn_after"] = prm.cpu().numpy(), bn.cpu().numpy()
    return out


if __name__ == "__main__":
    if len(sys.argv) not in (2, 3) or not os.environ.get("RULGNN_LIB"):
        raise SystemExit("usage: RULGNN_LIB=<library built from the parent commit> make_golden_train_mx_record_stores.py <parent commit hash> [output file]")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    fx = {"parent_commit": np.array(sys.argv[1]), "cus": np.int64(cus)}
    for case in cases(cus):
        r = run_case(case)
        assert np.isfinite(r["loss"]).all() and np.isfinite(r["grads"]).all() and np.isfinite(r["params_after"]).all(), case[0]
        for k, val in r.items():
            if k != "pred" or case[3] <= 8:         # predictions only of the single-tile cases: the fixture stays small
                fx[f"{case[0]}:{k}"] = val
        print("case", case[0], "batch", case[3], "loss", float(r["loss"][0]))
    dst = sys.argv[2] if len(sys.argv) == 3 else FIXTURE
    np.savez_compressed(dst, **fx)
    print("wrote", dst, os.path.getsize(dst), "bytes")
