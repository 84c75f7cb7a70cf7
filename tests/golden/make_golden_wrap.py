"""The "wrap" fixtures: one per older family, at a batch at which every clamped launch of the family's training step gives each
workgroup at least two items and a ragged last trip, produced by RUNNING THE REFERENCE on the CPU.

    python tests/golden/make_golden_wrap.py [FAMILY ...]     # needs the reference checkout (read-only import)

Models, weights and switches are those of each family's own maker (its ``build`` / ``perturbed_model``, dropout off).  The input is not
stored: it comes from tests/golden/synth.py::seeded_input (numpy default_rng; the value range and kind each maker uses today), and the
fixture holds ``x_seed``, ``x_kind``, ``x_shape``, ``x_lo``, ``x_hi`` and the fp64 sum ``x_checksum``; tests/golden/synth.py::Fixture
rebuilds ``x`` and checks the sum.  Stored besides: ``y``, the configuration, ``sd:`` weights, ``pred``, ``loss``, ``grad:*``,
``hasgrad:*``.  No per-sample taps (GRU_CM and STGNN, whose tests enumerate their fixtures by glob, hold ``eval_pred`` as well).

Batch rule.  For every kernel of the training step whose grid is clamped, ``items >= 2 clamp + 3``, where clamp is the explicit cap
(grid = min(items, cap)), min(cap, 2048) where the grid comes from an occupancy query (csrc/host_util.hpp::resident_rows and the like:
at most 256 CUs x 8 workgroups of 256 threads), or the batch at which a path switches.  B is odd and no multiple of a per-workgroup
tile.  Geometry: the family's smallest fixture geometry, or its wiring shape where kernels are specialised on it.  "oracle s" is the
family's fp64 oracle through tests/grad_cases.py::case on the machine the fixtures were made on (CPU, numpy's own threading); the
limit is 10 s.  All of csrc/:

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
SAGCN and AGCN_TF redraw the input until tests/test_sagcn_gpu.py::rank_margin > 1e-5, STAGNN until no covariance lies within 3e-8 of
its threshold (tests/test_stagnn_gpu.py); STGNN's GPU test has no such rule for its top-k and the first draw is kept.  The seed that
passed is the one stored.  SAGCN's kernels on sg_grid(B H), sg_grid(B) and sg_grid(P H) stay below their cap (one element per thread).
"""
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
import make_golden as mg                                   # noqa: E402  (installs the shims, sets sys.path)
import synth                                               # noqa: E402

MAX_DRAWS = 50


def rank_margin(x, n):
    """tests/test_sagcn_gpu.py::rank_margin: how far the median-rank power and the top amplitude of every patch sit from a tie."""
    F = np.fft.fft(x.reshape(-1, n), axis=1)
    pw = np.sort(np.abs(F) ** 2, axis=1)
    m = pw[:, n // 2:n // 2 + 1]
    below = np.where(pw < m * (1 - 1e-9), pw, -np.inf).max(1)
    above = np.where(pw > m * (1 + 1e-9), pw, np.inf).min(1)
    edge = np.minimum((m[:, 0] - below) / m[:, 0], (above - m[:, 0]) / m[:, 0])
    top = np.sort(np.abs(np.fft.rfft(x.reshape(-1, n), axis=1)), axis=1)
    return min(edge.min(), ((top[:, -1] - top[:, -2]) / top[:, -1]).min())


def draw(kind, seed, shape, lo=0.0, hi=1.0, accept=None):
    """The first of at most MAX_DRAWS inputs (seed, seed + 1000, ...) that ``accept`` takes; (x, the seed that passed)."""
    for attempt in range(MAX_DRAWS):
        s = seed + 1000 * attempt
        x = synth.seeded_input(kind, s, shape, lo, hi)
        if accept is None or accept(x.astype(np.float64)):
            return x, s
    raise SystemExit(f"no draw of {kind} {shape} passes the family's margin rule in {MAX_DRAWS} attempts")


def record(name, m, kind, seed, shape, cfg, lo=0.0, hi=1.0, accept=None, forward=None, dead=lambda n: False, state=mg.state_np,
           cfg_prefix="cfg:", cfg_type=np.int64, extra=None, before=None, eval_pred=False):
    bs = shape[0]
    x_np, x_seed = draw(kind, seed + 7, shape, lo, hi, accept)
    x = torch.from_numpy(x_np)
    y = torch.rand(bs, 1, generator=torch.Generator().manual_seed(seed + 8))
    out = {"x_seed": np.int64(x_seed), "x_kind": np.array(kind), "x_shape": np.asarray(shape, np.int64), "x_lo": np.float64(lo),
           "x_hi": np.float64(hi), "x_checksum": np.float64(x_np.astype(np.float64).sum()), "y": y.numpy().copy()}
    for k, v in cfg.items():
        out[cfg_prefix + k] = np.asarray(v, cfg_type)
    for k, v in state(m, "sd:").items():
        if not dead(k):
            out[k] = v
    out.update(extra or {})
    if eval_pred:                      # the families whose tests enumerate their fixtures by glob compare this one too
        m.eval()
        with torch.no_grad():
            out["eval_pred"] = m(x).numpy().copy()
    m.train()
    if before:
        before(m)
    t0 = time.time()
    res = forward(m, x) if forward else m(x)
    pred, add = res if isinstance(res, tuple) else (res, None)
    loss = torch.nn.functional.mse_loss(pred, y)
    if add is not None:
        loss = loss + add
    m.zero_grad()
    loss.backward()
    out["pred"], out["loss"] = pred.detach().numpy().copy(), np.float64(loss.item())
    for n_, p in m.named_parameters():
        if dead(n_):
            assert p.grad is None, n_
            continue
        out["grad:" + n_] = p.grad.numpy().copy() if p.grad is not None else np.zeros(tuple(p.shape), np.float32)
        out["hasgrad:" + n_] = np.bool_(p.grad is not None)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"wrote {name}: loss {out['loss']:.6f}, x seed {x_seed}, reference {time.time() - t0:.1f} s, {os.path.getsize(path)} bytes", flush=True)


def net01(n):
    return ".net0." in n or ".net1." in n


def stgcn():
    record("stgcn_wrap_14x30_bs32803", mg.perturbed_model(14, 30, 101), "uniform", 101, (32803, 14, 30),
           dict(num_patch=14, patch_size=30), cfg_prefix="", dead=lambda n: net01(n) and not n.startswith("sd:"))


def stconv():
    import make_golden_stconv as M
    cfg = dict(num_nodes=6, time_length=11, kernel_size=6)
    record("stconv_wrap_6x11_bs4099", M.build(cfg, 102), "uniform", 102, (4099, 6, 11), cfg, dead=lambda n: M.dead(n))


def astgcnn():
    import make_golden_astgcnn as M
    cfg = dict(num_nodes=14, time_length=50, encoder_out_dim=50, output_dim=64, K=3)
    record("astgcnn_wrap_14x50_bs4099", M.build(cfg, 103), "uniform", 103, (4099, 14, 50), cfg,
           dead=lambda n: net01(n) and not n.startswith("sd:"))


def rgcnu():
    import make_golden_rgcnu as M
    cfg = dict(num_nodes=5, time_length=12, hidden_dim=6, encoder_hidden_dim=8, kernel_size=3, alpha=0.7)
    record("rgcnu_wrap_5x12_bs4099", M.build(cfg, 104), "uniform", 104, (4099, 5, 12), cfg, cfg_type=np.float64,
           forward=lambda m, x: m(x, train=True)[0])


def fcstgnn():
    import make_golden_fcstgnn as M
    cfg = dict(M.WIRINGS["fd004"], num_patch=4, num_windows=5)          # the FD004 wiring with 4 patches of 2 instead of 25
    record("fcstgnn_wrap_fd004like_4p_bs257", M.build(cfg, 105), "uniform", 105, (257, cfg["num_node"], cfg["num_patch"] * cfg["patch_size"]), cfg,
           state=M.state_np)


def grucm():
    import make_golden_grucm as M
    cfg = dict(time_length=21, num_nodes=9, gru_hidden_dim=64)
    torch.manual_seed(106)
    m = M.ref_model.GRU_CM_model(**cfg)
    record("grucm_wrap_9x21_bs4099", m, "uniform", 106, (4099, 9, 21), cfg, before=M.no_dropout, eval_pred=True)


def stmsgcn():
    import make_golden_stmsgcn as M
    cfg = dict(num_patch=6, patch_size=113, interval=3, band_width=5, gcn_dims=[16, 64, 16, 1], gru_hidden_dim=8)       # 22 nodes
    record("stmsgcn_wrap_6x113_bs4099", M.build(cfg, 107), "uniform", 107, (4099, 1, 678), cfg)


def stagnn():
    import make_golden_stagnn as M
    from oracle import stagnn_oracle as O
    cfg = dict(num_nodes=5, time_length=12, hidden_dim=9, output_dim=4, num_heads=2, threshold=0.001)
    record("stagnn_wrap_5x12_bs4099", M.build(cfg, 108), "drifting", 108, (4099, 5, 12), cfg, cfg_type=np.float64,
           accept=lambda x: np.abs(O.adjacency(x, cfg["threshold"])[1] - cfg["threshold"]).min() > 3e-8)


def stgnn():
    import make_golden_stgnn as M
    cfg = dict(patch_size=7, num_patch=3, num_nodes=6, hidden_dim=12, K=2, top_k=4)
    record("stgnn_wrap_3x7_bs9721", M.build(cfg, 109), "uniform", 109, (9721, 6, 21), cfg, eval_pred=True)


def stnet(bs=2051):
    import make_golden_stnet as M
    from oracle import stnet_oracle as O
    cfg = dict(num_patch=4, patch_size=24, num_nodes=3, nperseg=4, input_dim=7, Cheb_layers=[7, 5], lstm_hidden_dim=3, autoencoder_hidden_dim=6)

    def accept(x):
        mag = O.stft_magnitude(x.reshape(bs * cfg["num_patch"], cfg["patch_size"]), cfg["nperseg"])
        nw = 0.3 * mag.mean(-1) + 0.1 * mag.max(-1) + 0.1
        return np.abs(nw - O.NODE_THRESHOLD).min() > 5e-5
    record(f"stnet_wrap_4x24_bs{bs}", M.build(cfg, 110), "modulated", 110, (bs, 96), cfg, accept=accept,
           forward=lambda m, x: m(x, train=True))


def sagcn():
    import make_golden_sagcn as M
    cfg = dict(num_patch=16, patch_size=7, gcn_hidden_dim=32, attention_hidden_dim=17)
    record("sagcn_wrap_16x7_bs8209", M.build(cfg, 111), "vibration", 111, (8209, 112), cfg, accept=lambda x: rank_margin(x, 7) > 1e-5,
           extra={"argsort_pinned_stable": np.bool_(False)})


def agcntf():
    import make_golden_agcntf as M
    cfg = dict(num_patch=5, patch_size=7, hidden_adj_dim=6, hidden_gnn_dim=7, num_heads=4)
    torch.manual_seed(112)
    m = M.ref_model.AGCN_TF_model(**cfg)
    record("agcntf_wrap_5x7_bs16411", m, "vibration", 112, (16411, 35), cfg, accept=lambda x: rank_margin(x, 7) > 1e-5,
           extra={"argsort_pinned_stable": np.bool_(False), "seed": np.int64(112)})


FAMILIES = {"ST_GCN": stgcn, "ST_Conv": stconv, "ASTGCNN": astgcnn, "RGCNU": rgcnu, "FC_STGNN": fcstgnn, "GRU_CM": grucm, "STMSGCN": stmsgcn,
            "STAGNN": stagnn, "STGNN": stgnn, "STNet": stnet, "SAGCN": sagcn, "AGCN_TF": agcntf}

if __name__ == "__main__":
    for fam in sys.argv[1:] or list(FAMILIES):
        FAMILIES[fam]()
