"""-m gpu: every family's gradients of one fused training step, element by element against the fp64 oracles, on every golden fixture
that holds the reference's gradients (tests/grad_cases.py).

The other GPU tests hold gradients to max|got - ref| / max|ref| < 5e-4..1e-3 per tensor, which lets any element below that share of
its tensor's largest be 100 % wrong; in most of these tensors that is most of the elements (tests/golden/grad_noise.json).  Here every
element of every live tensor is held to

    |got_e - g64_e| <= rtol |g64_e| + 16 max(noise of the reference's fp32 gradient on this tensor, 2^-23 max|g64|)

(tests/grad_gate.py: rtol is the family's existing gate; the floor is measured on the reference's own fp32 autograd from the fixture,
never on the kernels).  Tensors that are zero in exact arithmetic stay under the families' existing rules (tests/test_grad_gate_cpu.py
pins which).  One line per tensor is printed, so the run's log is the record of the kernels' own ratios.

Each step is the family's existing entry point at dropout 0 on the fixture's parameters and batch: ``fused_mse_step`` for the module
families, the C-ABI for ST_GCN (once per training path that accepts the shape) and GRU_CM (both recurrences), the graph stack under
the reference's imposed selection and the LSTM stack for HAGCN, whose data gradient d loss / d nodes is gated too.  FC_STGNN runs
its fp32 path; the bf16 variant does not claim fp32 accuracy.

The ``*_wrap_*`` fixtures (tests/golden/make_golden_wrap.py) run the same comparison at batches of thousands, where the clamped grids
give every workgroup several items and a ragged last trip: partial-gradient rows that sum many items, persistent loops on their
second trip, the paths a large batch switches to.  Their input is rebuilt from a seed (tests/golden/synth.py::Fixture).  On them the
prediction is held per element and the loss at the family's forward gate as well, against the oracle's own (_check_forward), ST_GCN
asserts the resolved form and two trips per workgroup under every grid the launch code bounds from outside, and GRU_CM holds
both recurrences.  The derivation, from the launch code (all of csrc/; "oracle s" is the fp64 oracle's CPU seconds where the fixtures
were made, the limit being 10):

fixture, oracle s                      kernel / launch                                         items                          clamp   items at B
stgcn_wrap_14x30_bs32803      7.6      matrix-core chain: min(loads, CUs x 2, max_grid 2048)   workgroup-loads: 4 wavefront   512     2051
                                       (mxt_launch caps the occupancy at MX_WAVES_PER_SIMD 2)  tiles of 4 samples = B / 16
                                       fp32 chain: min(loads, resident grid, max_grid 2048);   the same workgroup-loads       1024    2051
                                       F_0 (38464 B of LDS: 4 per CU), G_0 (44224 B: 3), and
                                       by their registers F_2, TOP, G_1 .. G_3 (104 to 168)
                                       fp32 chain, F_1 and F_3 (11584 B, 76 registers: 6 per CU)   the same workgroup-loads   1536    2051  (*)
fcstgnn_wrap_fd004like_4p_bs257  0.9   partial-gradient rows, w->rows 512 (fcstgnn.hip)        M = B NP N = 56 B rows         512     14392  (**)
astgcnn_wrap_14x50_bs4099     3.9      ast_graph_bwd_kernel, resident_rows(B, AST_BWD_ROWS)    B samples                      2048    4099
                                       tcn_conv_bwd_kernel<2>, resident_rows(B, w->rows 1024)  B samples                      1024    4099
                                       tcn_conv_kernel<1>, ast_front_kernel, resident_rows(B)  B samples                      2048    4099
stmsgcn_wrap_6x113_bs4099  8.5-12 (5*) msg_features_mx / msg_gcn_backward_mx (22 nodes >= 12), ceil(G / MXW 4), G = 6 B       1024    6149
                                       resident_rows(.., rows_gcn_max 1024)
                                       msg_gi_backward_kernel<24>, parts = min(R / 256, 1024)  R / 256, R = G n = 132 B rows  1024    2114
                                       head: parts loop runs while B parts < 1024              B samples                      1024    4099
stconv_wrap_6x11_bs4099       0.3      sc_cnn_bwd_kernel, resident_rows(B, w->rows 1024)       B samples                      1024    4099
rgcnu_wrap_5x12_bs4099        0.5      sample kernels, blocks = min(B, 512)                    B samples                      512     4099
                                       graph kernels, gblocks = min(G, 2048), halved on mx     G >= B graphs                  2048    >= 4099
stagnn_wrap_5x12_bs4099       0.3      every kernel of the step, nblk = min(B, 256)            B samples                      256     4099
stgnn_wrap_3x7_bs9721         0.5      gn_blocks: min(ceil(n / 256), 4096) workgroups          n = B Q = 216 B elements       2^20    2099736
stnet_wrap_4x24_bs2051        0.4      sn_head_kernel, min(B, 1024)                            B samples                      1024    2051  (***)
                                       sn_stft / sn_terms / sn_terms_bwd, ggrid = min(G, 4096) G = 4 B graphs                 4096    8204
                                       sn_grid: min(ceil(n / 256), 4096): bias, ReLU, head     n <= B T D = 60 B elements     2^20    123060  (6*)
                                       backward, add, scale; sn_recon_kernel, rblocks 1024     B T D elements                 2^18    123060  (6*)
sagcn_wrap_16x7_bs8209        2.2      sg_graph_mx_kernel (16 patches: the form the wirings    B samples                      4096    8209
                                       dispatch), sg_features_kernel, min(B, 4096)
                                       sg_patch_features_kernel<64> (n <= 64), min(R, 65536)   R = P B patch rows             65536   131344
                                       sg_grid: min(ceil(n / 256), 8192): bias, ReLU, tanh     n = R H = 512 B or Ah B H      2^21    4203008
                                       sg_attn_head_kernel, min(B ceil(H / 64), 65536)         B x 1 wavefronts (H = 32)      65536   8209  (7*)
agcntf_wrap_5x7_bs16411       7.4      at_graph_kernel<false / true>, at_grid(B, 8192)         B samples                      8192    16411
                                       sagcn_features: sg_features_kernel, min(B, 4096)        B samples                      4096    16411
                                       sagcn_features: sg_patch_features_kernel<64>, min(R, 65536)   R = P B patch rows       65536   82055  (****)
                                       attention forward / backward, at_grid(B heads nqt, 65536)   B x 4 heads x 1 tile       65536   65644  (****)
grucm_wrap_9x21_bs4099        7.5      graph forward / backward, min(rounds, GC_MAX_BLOCKS)    rounds = G / 16, G = 21 B      1024    5380
                                       head gradient: hslices = ceil(B / 128); 1 writes directly, more go through hpart   B   128     4099 (33 slices)

Short of the rule (items < 2 clamp + 3), and why:
(*)    ST_GCN.  A workgroup is 4 wavefronts and a wavefront tile 4 samples, so a grid of g workgroups takes B / 16 loads.  The matrix-core
       chain never launches more than 2 workgroups per CU, and the fp32 phases F_0 and G_0 are held to 4 and 3 per CU by the LDS they
       ask for (pinned in csrc/stgcn_train.hip; 160 KB a CU): with at most 256 CUs every workgroup of those makes two trips or more
       (2051 >= 2 x 1024 + 3), which the GPU test asserts from the device's CU count.  The other fp32 phases are held by their
       registers alone, which no entry reports and the test cannot see: as compiled for gfx950 today (vgpr_count in the code object's
       notes, 512 registers a SIMD lane) F_2 has 104, TOP 153 and G_1 .. G_3 151 to 168, at most 4 workgroups per CU, but F_1 and F_3
       have 76 and may launch 6 per CU, 1536: there 515 workgroups make a second trip.  The rule for them needs 3075 loads (4099 if
       one goes by max_grid alone), B >= 49185, where the fp64 oracle takes more than 10 s (7.6 s at 32803, 20 s at 65569).  The
       14 x 30 shape is what the kernels are specialised on, so the geometry is not shrunk.
(**)   FC_STGNN has no clamp on samples; the rule needs M >= 1027.  At B = 4099 the reference's own fp32 autograd is 2.5e-3 of the
       largest element away from fp64 on nonlin_map2.1.bias and above the family's 5e-4 gate on 12 tensors (4.6e-4 at B = 1031), so
       neither the family's rule nor a floor of 16 x that noise would say anything; at 257 it is 5e-5 and every partial row sums 28 rows.
       The FD004 wiring with 4 patches instead of 25 (as fcstgnn_fd003like_6p shrinks FD003): that noise grows with the rows M.
(***)  STNet decides node by node against a threshold; the family's rule (no node weight within 5e-5 of 0.7, tests/test_stnet_gpu.py)
       passed no draw of 50 at B = 4099 (49188 node weights), so it gets the next batch that passes its smallest clamp twice.  The
       graph kernels' 4096 then needs 4 patches; with stnet_small's 4 nodes (32816 node weights) no draw passed either, so the fixture
       has nperseg 4: 3 nodes x 7 frames, 24612 node weights as at 3 patches of 4 nodes.
(****) AGCN_TF.  4 heads is the most the kernels take and 5 patches make one query tile: wrapping the attention grids and the patch-feature
       grid twice needs B >= 32769, where the oracle takes 22 s, or 8 patches, for which its 7.4 to 9.5 s at 5 patches leave no room.  At 16411 both caps are active (108
       attention workgroups and 16519 patch-feature wavefronts take a second item); the graph and feature kernels wrap twice.
(5*)   STMSGCN's oracle took 8.5, 9.1, 11.6 and 11.8 s in four runs on the machine the fixture was made on: it straddles the limit.  22 nodes
       are the fewest at which msg_gi_backward's parts pass 2 x 1024 + 3 with the 6 patches of the small wiring shape, so nothing is left to shrink.
(6*)   STNet's element-wise kernels run one element per thread and would need B T D >= 2^21 + 3 (2^19 + 3 for sn_recon) for a second trip:
       a layer 256 wide at this batch, while the widest of the small geometry is D = 15.  They never wrap here.
(7*)   sg_attn_head_kernel runs one wavefront per (sample, 64 hidden units): two trips need B >= 131075, sixteen times the batch and the
       oracle's 2.2 s.  It never wraps here.  at_head_finish_kernel (ceil(B / 256) against 4096) and SAGCN's kernels on sg_grid(B H),
       sg_grid(B) and sg_grid(P H) stay below their caps as well (one element per thread).
"""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import grad_cases as GC
import grad_gate as GG
from gnn_rul_benchmarking_amd import _lib, params as PL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (family, tensor) -> (margin, where the source states arithmetic coarser than fp32 for it, measured ratio at margin 16).
# Conditions: no margin above 64; at most one tensor in ten of a family; the elements over the base gate spread over the tensor
# (not a row, a column or a trailing range).  Empty: every tensor is held at the base margin.
MARGINS = {}

ST_GCN_PATHS = {"chain": _lib.STEP_CHAIN, "mx": _lib.STEP_MX}


def _cases():
    out = []
    for fam, name in GC.all_cases():
        if fam != "ST_GCN":
            out.append(pytest.param(fam, name, None, id=name))
            continue
        # the fp32 phase chain and the matrix-core chain (narrow: num_patch <= 15; wide: 40 x 64, 16 x 16) through the step entry with an
        # explicit path.  A path that does not take a shape says so by its return code, before anything is compared.  num_patch = 160
        # is the tiled path, which ignores the path argument (include/rulgnn.h): one case, through the forward-backward entry.
        for path in ["tiled"] if "160x16" in name else list(ST_GCN_PATHS):
            out.append(pytest.param(fam, name, path, id=f"{name}-{path}"))
    return out


def test_rtol_is_each_familys_existing_gate():
    import test_agcntf_gpu, test_astgcnn_gpu, test_fcstgnn_gpu, test_grucm_gpu, test_hagcn_gpu, test_mpnn_order_gpu, test_rgcnu_gpu      # noqa: E401
    import test_stconv_gpu, test_stmsgcn_gpu, test_stnet_gpu, test_train_gpu                                                             # noqa: E401
    want = {"ST_GCN": test_train_gpu.GTOL, "FC_STGNN": test_fcstgnn_gpu.GTOL, "ASTGCNN": test_astgcnn_gpu.GTOL, "HAGCN": test_hagcn_gpu.GTOL,
            "STMSGCN": test_stmsgcn_gpu.GTOL, "ST_Conv": test_stconv_gpu.GTOL, "RGCNU": test_rgcnu_gpu.GTOL, "STNet": test_stnet_gpu.GTOL,
            "AGCN_TF": test_agcntf_gpu.GTOL, "GRU_CM": test_grucm_gpu.GTOL_ORACLE}
    assert test_mpnn_order_gpu.GTOL == test_train_gpu.GTOL
    import test_sagcn_gpu, test_stagnn_gpu                                                                                                # noqa: E401
    for mod in (test_agcntf_gpu, test_astgcnn_gpu, test_fcstgnn_gpu, test_grucm_gpu, test_rgcnu_gpu, test_sagcn_gpu, test_stagnn_gpu,
                test_stconv_gpu, test_stmsgcn_gpu, test_stnet_gpu, test_train_gpu):
        assert mod.TOL == FORWARD_TOL, mod.__name__
    for fam, tol in want.items():
        assert GC.rtol_of(fam) == tol, fam
    assert all(m <= 64 for m, _, _ in MARGINS.values())
    for fam in GC.FAMILIES:
        n = len(GC.case(fam, GC.fixtures(fam)[0]).live)
        assert 10 * sum(1 for f, _ in MARGINS if f == fam) <= n, fam


# ---- one training step per family ----------------------------------------------------------------------------------------------------

LAST = {}          # the prediction [B] and the loss of the step a runner made last (held on the wrap cases)


def _keep(pred, loss):
    LAST["pred"] = (pred.detach().cpu().numpy() if torch.is_tensor(pred) else np.asarray(pred)).reshape(-1)
    LAST["loss"] = float(loss)


def _xy(c):
    return torch.tensor(c.x, device=DEV), torch.from_numpy(c.z["y"]).to(DEV)


def _module_step(m, c, grads_of):
    m.train()
    x, y = _xy(c)
    pred, loss = m.fused_mse_step(x, y)
    torch.cuda.synchronize()
    _keep(pred, loss)
    return grads_of(m)


def _sd(z):
    return {k[3:]: z[k] for k in z.files if k.startswith("sd:")}


def _stgcn(c, path):
    import gpu_util as G
    z, sd = c.z, c.extra["sd"]
    N, P, L, K = c.extra["dims"]
    flat, _ = PL.pack_numpy(sd, N, L, k=K)
    if path == "tiled":
        shp = G.shape_struct(c.x.shape[0], N, P, L, K)
        assert _lib.load().rulgnn_stgcn_train_step_resolve(C.byref(shp), None, _lib.STEP_AUTO) == _lib.EUNSUPPORTED    # not a phase chain
        r = G.abi_train(c.x, z["y"], flat, N, P, L=L, k=K, mode="fwdbwd")
        got = r["grads"]
    else:
        from test_stgcn_lds_envelope_gpu import run_train
        B = c.x.shape[0]
        rc, r = run_train(np.array(c.x.reshape(B, -1), np.float32), np.ascontiguousarray(z["y"].reshape(B), np.float32),
                          flat, N, P, L, K, "step", ST_GCN_PATHS[path], False, 0.0, 0, 1)
        if rc == _lib.EUNSUPPORTED and not c.wrap:                            # (the wrap case is 14 x 30, which both chains must take)
            assert r["untouched"]
            pytest.skip(f"the {path} path does not take {N} x {P}, {L} layers, order {K} (EUNSUPPORTED before any launch)")
        assert rc == 0, rc
        form = _lib.load().rulgnn_stgcn_train_step_resolve(C.byref(G.shape_struct(B, N, P, L, K)), None, ST_GCN_PATHS[path])
        print(f"ST_GCN {c.name} [{path}]: the step resolves to form {form} (CHAIN {_lib.STEP_CHAIN}, COOP {_lib.STEP_COOP}, MX {_lib.STEP_MX})")
        if c.wrap:
            # No entry reports the grid a phase launched.  What the launch code fixes from outside: a phase's grid is
            # min(workgroup-loads, CUs x workgroups per CU, max_grid 2048); the matrix-core chain caps the workgroups per CU at
            # MX_WAVES_PER_SIMD = 2 (mxt_launch, train_f0_mx_launch), and the fp32 phases F_0 and G_0 ask for 38464 and 44224 B of the
            # CU's 160 KB of LDS (pinned in csrc/stgcn_train.hip), 4 per CU at the most.  Under those every workgroup makes two trips
            # or more with a ragged last one; under the 8 per CU that 256 threads allow, none of the other phases covers the batch in
            # one trip (note (*) above says how far those fall short of the rule).
            assert form == ST_GCN_PATHS[path], (form, path)
            assert (N, P, L) == (14, 30, 2), (N, P, L)
            tiles = -(-B // 4)                                                # 4 samples per wavefront tile at num_patch <= 16 (train_geometry)
            loads = -(-tiles // 4)                                            # 4 wavefronts per workgroup
            cus = torch.cuda.get_device_properties(0).multi_processor_count
            held = min(2048, cus * (2 if path == "mx" else (160 * 1024) // 38464))
            cap = min(2048, 8 * cus)
            print(f"ST_GCN {c.name} [{path}]: {tiles} sample tiles, {loads} workgroup-loads; grid at most {held} where the launch code "
                  f"bounds the occupancy, at most {cap} elsewhere")
            assert loads >= 2 * held + 3 and loads % held, (loads, held)
            assert cap < loads < tiles, (cap, loads, tiles)
        got = r["grads"]
    _keep(r["pred"], r["loss"])
    return {k: got[off:off + int(np.prod(shape))] for k, (off, shape) in PL.live_param_layout(N, L, K).items()}


def _fcstgnn(c, _):
    from test_fcstgnn_gpu import build_model, grads_of
    return _module_step(build_model(c.extra["cfg"], _sd(c.z)), c, grads_of)


def _astgcnn(c, _):
    from test_astgcnn_gpu import build_model, cfg_of, grads_of
    return _module_step(build_model(cfg_of(c.z), _sd(c.z)), c, grads_of)


def _stconv(c, _):
    from test_stconv_gpu import build_model, cfg_of, grads_of
    return _module_step(build_model(cfg_of(c.z), _sd(c.z)), c, grads_of)


def _with_cfg(module):
    def run(c, _):
        mod = __import__(module)
        return _module_step(mod.build_model(c.extra["cfg"], c.extra["p"]), c, mod.grads_of)
    return run


def _stgnn(c, _):
    from test_stgnn_gpu import model_from
    m = model_from(c.z, c.extra["cfg"]).train()
    x, y = _xy(c)
    pred, loss = m.fused_mse_step(x, y)
    torch.cuda.synchronize()
    _keep(pred, loss)
    flat = m.bucket[:m.num_live].detach().cpu().numpy()
    out, off = {}, 0
    for k, p in m._named_live():
        out[k] = flat[off:off + p.numel()]
        off += p.numel()
    assert off == m.num_live
    return out


def _grucm(c, _):
    import grucm_oracle as O
    from test_grucm_gpu import abi
    z, cfg = c.z, c.extra["cfg"]
    p32 = {k: v for k, v in _sd(z).items()}
    kw = dict(mode="fwdbwd", y_np=z["y"], training=True)
    got = {}
    # the persistent recurrence (the default at these shapes) and the step loop: the second set of tensors carries the path's name
    for tag, path in (("", _lib.GRUCM_GRU_AUTO), ("@step_loop", _lib.GRUCM_GRU_STEP_LOOP)):
        r = abi(c.x, p32, cfg, gru_path=path, **kw)
        g = O.unflatten(r["grads"], p32)
        got.update({k + tag: v for k, v in g.items()})
        if c.wrap:
            _check_forward(c, r["pred"], r["loss"], f"GRU_CM {c.name} [{tag[1:] or 'auto'}]")
    return got


def _hagcn(c, _):
    from test_hagcn_gpu import build, cfg_of, forced_of
    z = c.z
    m = build(cfg_of(z), _sd(z)).train()
    m.forced_topk = forced_of(z)
    nodes = torch.from_numpy(z["nodes"]).to(DEV).requires_grad_(True)
    y = torch.from_numpy(z["y"]).to(DEV)
    feats, kl = m.graph_stack(nodes)
    pred = m.fc(feats.reshape(y.size(0), -1))
    (torch.nn.functional.mse_loss(pred, y) + float(z["alpha"]) * kl).backward()
    table = dict(m.named_parameters())
    got = {k: table[k].grad.cpu().numpy() for k in c.g64 if not k.startswith("TD.") and k != "grad_nodes"}
    got["grad_nodes"] = nodes.grad.cpu().numpy()
    td = [k for k in c.g64 if k.startswith("TD.")]
    if td:
        # the LSTM stack with the reference's d loss / d nodes fed in (tests/test_hagcn_gpu.py::test_lstm_stack_gradients_match_reference_golden)
        m.zero_grad()
        x = torch.from_numpy(z["x"]).to(DEV)
        bs, N = x.size(0), x.size(1)
        ps, npatch = int(z["cfg:patch_size"]), int(z["cfg:num_patch"])
        v = x.reshape(bs, N, npatch, ps).transpose(1, 2).transpose(1, 2).reshape(bs * N, npatch, ps).transpose(1, 0)
        out = m.TD(v).transpose(1, 0).reshape(bs, N, npatch, -1).transpose(1, 2).reshape(bs * npatch, N, -1)
        out.backward(torch.from_numpy(z["grad_nodes"]).to(DEV))
        table = dict(m.named_parameters())
        got.update({k: table[k].grad.cpu().numpy() for k in td})
    torch.cuda.synchronize()
    return got


FORWARD_TOL = 1e-4          # every family's forward / loss gate (TOL of its GPU test file; test_rtol_is_each_familys_existing_gate)


def _check_forward(c, pred, loss, tag):
    """The wrap cases' prediction per element (gpu_util.elem_gate at the family's forward gate) and loss against the fp64 oracle's.
    The absolute floor is elem_gate's own 1e-6 of the largest prediction wherever the reference's own fp32 prediction (the fixture's)
    passes that gate against the oracle: eleven of the twelve fixtures, at ratios of 0.001 to 0.40.  AGCN_TF's does not, at 13.8 (its
    predictions, at most 0.03, are differences of far larger terms); only there the floor is 16 x the distance of the reference's fp32
    prediction from the oracle, 5.4e-4 of the largest -- the construction of tests/grad_gate.py::floor_for.  Which floor applies is
    decided by the fixture and the oracle alone, never by what the kernels give."""
    import gpu_util as G
    ref32 = np.asarray(c.z["pred"], np.float32).reshape(-1)
    floor = 1e-6
    if G.elem_gate(ref32, c.pred64, rtol=FORWARD_TOL, floor=floor) > 1.0:
        floor = GG.MARGIN * GG.noise(ref32, c.pred64) / np.abs(c.pred64).max()
    e = G.elem_gate(pred, c.pred64, rtol=FORWARD_TOL, floor=floor)
    le = abs(loss - c.loss64) / abs(c.loss64)
    print(f"{tag}: prediction elem_gate {e:.3f} (floor {floor:.1e} of max), loss rel err {le:.2e}")
    assert np.asarray(pred).size == c.pred64.size and e <= 1.0, (tag, e)
    assert le < FORWARD_TOL, (tag, le)


RUN = {"ST_GCN": _stgcn, "FC_STGNN": _fcstgnn, "ASTGCNN": _astgcnn, "HAGCN": _hagcn, "STMSGCN": _with_cfg("test_stmsgcn_gpu"),
       "ST_Conv": _stconv, "RGCNU": _with_cfg("test_rgcnu_gpu"), "STAGNN": _with_cfg("test_stagnn_gpu"), "STGNN": _stgnn,
       "STNet": _with_cfg("test_stnet_gpu"), "SAGCN": _with_cfg("test_sagcn_gpu"), "AGCN_TF": _with_cfg("test_agcntf_gpu"), "GRU_CM": _grucm}


@pytest.mark.parametrize("family,name,path", _cases())
def test_gradients_element_by_element_against_fp64(family, name, path):
    with np.errstate(over="ignore"):
        c = GC.case(family, name)
    t0 = time.perf_counter()
    LAST.clear()
    got = RUN[family](c, path)
    tag = f"{family} {name}" + (f" [{path}]" if path else "")
    lines, bad = GC.check(c, got, tag, MARGINS)
    print("\n".join(lines))
    if c.wrap:
        print(f"{tag}: oracle {c.oracle_seconds:.2f} s (once per process), step and comparison {time.perf_counter() - t0:.2f} s")
        if family != "GRU_CM":                       # (both of GRU_CM's recurrences were held inside its runner)
            _check_forward(c, LAST["pred"], LAST["loss"], tag)
    assert not bad, "\n".join(bad)
