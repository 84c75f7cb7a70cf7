"""Time one HierCorrPool_bearing training step on the GPU at the reference's five geometries (PHM2012 Condition_1, _2, _3 and XJTU_SY
Condition_1, _2 = _3; hidden 10, embedding 10, six pooled nodes), in the two forms of tools/time_hiercorrpool.py, whose driver this is:

  (a) ``HierCorrPool_bearing.update``: the STFT packing kernel and the chain of csrc/hiercorrpool.hip + the shared SGEMM + fused Adam,
      one C call;
  (c) the torch restatement of tests/hiercorrpool_bearing_oracle.py on the GPU (``torch.stft``, ATen conv1d / batch_norm / max_pool1d /
      bmm, torch.optim.Adam): what a user of the reference's model gets on this card.

    python tools/time_hiercorrpool_bearing.py [--shapes phm1 phm2 phm3 xjtu1 xjtu2] [--batches 100 1024] [--steps 100] [--out FILE]
    python tools/time_hiercorrpool_bearing.py --trace xjtu1 100 [--form a|c]      # launches per step and the per-kernel split
    python tools/time_hiercorrpool_bearing.py --stft [--batches 100 1024]         # the packing kernel alone, against its byte count

``--stft`` runs a few eval forwards per geometry under the HIP activity tracer, takes the packing kernel's own line and prints its
time per launch, the 4 (P p + (P + 8) C0) bytes per sample it must move (the raw window in, the padded block-1 input out) and the
bandwidth that time amounts to.  (Bytes the memory system actually moved need the hardware counters: run the same command under
``rocprofv3 --pmc`` in a run of its own.)"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import time_hiercorrpool as TH          # noqa: E402  (sets sys.path for the package and tests/)

SHAPES = {"phm1": ("PHM2012", "Condition_1"), "phm2": ("PHM2012", "Condition_2"), "phm3": ("PHM2012", "Condition_3"),
          "xjtu1": ("XJTU_SY", "Condition_1"), "xjtu2": ("XJTU_SY", "Condition_2")}
KERNEL = "hcpb_stft_input_kernel"


def config(shape):
    from gnn_rul_benchmarking_amd.hparams import get_hparams_class
    return dict(get_hparams_class(SHAPES[shape][0])(SHAPES[shape][1]).alg_hparams["HierCorrPool_bearing"])


def fused_step_fn(dev, cfg):
    from gnn_rul_benchmarking_amd.algorithms import HierCorrPool_bearing
    torch.manual_seed(0)
    algo = HierCorrPool_bearing(cfg, {"learning_rate": TH.LR, "weight_decay": TH.WD}, dev)
    algo.to(dev)
    algo.train()
    algo.sync_loss = False
    return lambda x, y: algo.update(x, y, 1)


def torch_step_fn(dev, cfg):
    import hiercorrpool_bearing_oracle as O
    from gnn_rul_benchmarking_amd.hiercorrpool_bearing import HierCorrPool_bearing_model
    torch.manual_seed(0)
    sd = {k: v.detach().clone().to(dev) for k, v in HierCorrPool_bearing_model(**cfg).state_dict().items()}
    for k in O.param_names():
        sd[k].requires_grad_(True)
    opt = torch.optim.Adam([sd[k] for k in O.param_names()], lr=TH.LR, weight_decay=TH.WD)
    return lambda x, y: O.torch_step(sd, opt, x, y, cfg)


def batch(dev, cfg, B):
    return torch.randn(B, cfg["num_patch"] * cfg["patch_size"], device=dev), torch.rand(B, 1, device=dev)


def must_move_bytes(cfg):
    """Per sample: the raw window in, the padded channel-last block-1 input out."""
    P, p, C0 = cfg["num_patch"], cfg["patch_size"], cfg["num_nodes"] * cfg["input_dim"]
    return 4 * (P * p + (P + 8) * C0)


def stft_alone(shapes, batches):
    from gnn_rul_benchmarking_amd.hiercorrpool_bearing import HierCorrPool_bearing_model
    dev = torch.device("cuda:0")
    for shape in shapes:
        cfg = config(shape)
        torch.manual_seed(0)
        m = HierCorrPool_bearing_model(**cfg).to(dev).eval()
        for B in batches:
            x, y = batch(dev, cfg, B)

            def fn(x, y):
                with torch.no_grad():
                    return m(x)
            _, _, rows = TH.trace(fn, x, y, 10)
            mine = [r for r in rows if KERNEL in r[0]]
            us = mine[0][2] / mine[0][1]
            need = must_move_bytes(cfg)
            print(json.dumps(dict(kernel=KERNEL, shape=shape, batch=B, launches_per_forward=mine[0][1], us_per_launch=us,
                                  must_move_bytes_per_sample=need, raw_window_bytes_per_sample=4 * cfg["num_patch"] * cfg["patch_size"],
                                  gbytes_per_s_at_that_count=need * B / us / 1e3)), flush=True)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("time_hiercorrpool_bearing.py measures on the GPU: none found")
    if "--stft" in sys.argv:
        i = sys.argv.index("--batches") if "--batches" in sys.argv else None
        stft_alone(tuple(SHAPES), [int(b) for b in sys.argv[i + 1:]] if i else [100, 1024])
    else:
        TH.main(tuple(SHAPES), config, fused_step_fn, torch_step_fn, batch)
