"""Time one LOGO_bearing training step on the GPU at the reference's two geometries (PHM2012: patch 64, 40 patches, nperseg 8 -- 5 nodes
of 9 features; XJTU_SY: 1024, 32, 32 -- 17 nodes of 33), in the two forms of tools/time_logo.py, whose driver this is:

  (a) ``LOGO_bearing.update``: the graph kernels of csrc/logo.hip with the STFT fused in front (the spectrogram never leaves LDS) + the
      persistent Bi-LSTM of csrc/bilstm.hip + the shared SGEMM + fused Adam, one C call, and the MultiStepLR step on the host;
  (c) the torch restatement of tests/logo_bearing_oracle.py on the GPU (``torch.stft``, ATen bmm / softmax, the vendor LSTM,
      torch.optim.Adam): what a user of the reference's model gets on this card.

    python tools/time_logo_bearing.py [--shapes phm2012 xjtu_sy] [--batches own 1024] [--steps 100] [--warmup 10] [--out FILE]
    python tools/time_logo_bearing.py --trace xjtu_sy 100 [--form a|c]      # launches per step and the per-kernel split
    python tools/time_logo_bearing.py --bytes                                 # the graph kernels' HBM traffic per sample, from the shapes

``--bytes`` prints, per geometry, what the two graph kernels move per sample beside the parameters (which stay in cache): the raw window
in, Hg out (forward); the raw window and d Hg in (backward) -- against the raw window's own size and against the spectrogram a
separate magnitude pass would write and both kernels would read back."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import time_logo as TL          # noqa: E402  (sets sys.path for the package and tests/)

SHAPES = {"phm2012": ("PHM2012", "Condition_1"), "xjtu_sy": ("XJTU_SY", "Condition_1")}


def config(shape):
    from gnn_rul_benchmarking_amd.hparams import get_hparams_class
    h = get_hparams_class(SHAPES[shape][0])(SHAPES[shape][1])
    return dict(h.alg_hparams["LOGO_bearing"]), dict(h.train_params["LOGO_bearing"])


def fused_step_fn(dev, cfg, hp):
    from gnn_rul_benchmarking_amd.algorithms import LOGO_bearing
    torch.manual_seed(0)
    algo = LOGO_bearing(cfg, hp, dev)
    algo.to(dev)
    algo.train()
    algo.sync_loss = False
    return lambda x, y: algo.update(x, y, 1)


def torch_step_fn(dev, cfg, hp):
    import logo_bearing_oracle as O
    from gnn_rul_benchmarking_amd.logo_bearing import LOGO_bearing_model
    torch.manual_seed(0)
    sd = {k: v.detach().clone().to(dev) for k, v in LOGO_bearing_model(**cfg).state_dict().items()}
    for k in O.param_names():
        sd[k].requires_grad_(True)
    opt = torch.optim.Adam([sd[k] for k in O.param_names()], lr=hp["learning_rate"], weight_decay=hp["weight_decay"])
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, [5, 10, 20, 25], 0.5)

    def step(x, y):
        loss = O.torch_step(sd, opt, x, y, cfg, hp["theta"])
        sched.step()
        return loss
    return step


def batch(dev, cfg, B):
    return torch.randn(B, cfg["num_patch"] * cfg["patch_size"], device=dev), torch.rand(B, 1, device=dev)


def graph_bytes():
    for shape in SHAPES:
        cfg, _ = config(shape)
        T, P, N, f = cfg["num_patch"], cfg["patch_size"], cfg["num_nodes"], cfg["input_dim"]
        raw, hg, spec = 4 * T * P, 4 * T * N * 3 * f, 4 * T * N * f
        print(json.dumps(dict(shape=shape, raw_window_bytes=raw, fwd_bytes=raw + hg + 8, bwd_bytes=raw + hg, spectrogram_bytes=spec,
                              fwd_over_raw=(raw + hg + 8) / raw, bwd_over_raw=(raw + hg) / raw,
                              separate_pass_extra_bytes=3 * spec)))


if __name__ == "__main__":
    if "--bytes" in sys.argv:
        graph_bytes()
    else:
        TL.main(tuple(SHAPES), config, fused_step_fn, torch_step_fn, batch)
