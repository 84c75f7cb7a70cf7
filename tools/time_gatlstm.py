"""Time one GAT_LSTM training step (forward + backward + Adam) on the GPU at three of the reference's geometries (40 nodes of 64 points:
PHM2012 Condition_1 / _3; 80 of 32: PHM2012 Condition_2; 32 of 1024: XJTU_SY Condition_1 / _3), in two forms per batch size:

  (a) ``GAT_LSTM.update``: the patch statistics and the banded attention kernels of csrc/gatlstm.hip + the shared SGEMM + the LSTM
      kernels + fused Adam, one C call;
  (c) the torch restatement of tests/gatlstm_oracle.py on the GPU, computed the reference's way -- the pair tensor cat(Wh_i, Wh_j) and
      the dense adjacency included, the LSTM layers on the vendor kernel behind nn.LSTM (torch._VF.lstm) -- with torch's dropout and
      torch.optim.Adam: what a user of the reference's model gets on this card.

    python tools/time_gatlstm.py [--shapes 40x64 80x32 32x1024] [--batches 100 1024] [--steps 100] [--warmup 10] [--out FILE]
    python tools/time_gatlstm.py --trace 80x32 100 [--form a|c]      # a run of its own: launches per step and the per-kernel split

The two forms alternate in windows inside one process so that they see the same machine state; every window ends in a device
synchronise.  ``--trace`` runs a few steps of one form under the HIP activity tracer (torch.profiler) and prints the kernel launches per
step, the time per kernel name, the attention kernels' share and their bytes per graph against the 2 N C 4 of one read of Z and one
write of h.  One JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROWS = {"40x64": ("PHM2012", "Condition_1"), "80x32": ("PHM2012", "Condition_2"), "32x1024": ("XJTU_SY", "Condition_1")}


def config(shape):
    from gnn_rul_benchmarking_amd.hparams import get_hparams_class
    h = get_hparams_class(ROWS[shape][0])(ROWS[shape][1])
    return dict(h.alg_hparams["GAT_LSTM"]), dict(h.train_params["GAT_LSTM"])


def fused_step_fn(dev, cfg, hp):
    from gnn_rul_benchmarking_amd.algorithms import GAT_LSTM
    torch.manual_seed(0)
    algo = GAT_LSTM(cfg, hp, dev)
    algo.to(dev)
    algo.train()
    algo.sync_loss = False
    return lambda x, y: algo.update(x, y, 1)


def torch_step_fn(dev, cfg, hp):
    import gatlstm_oracle as O
    from gnn_rul_benchmarking_amd.gatlstm import GAT_LSTM_model
    torch.manual_seed(0)
    sd = {k: v.detach().clone().to(dev).requires_grad_(True) for k, v in GAT_LSTM_model(**cfg).state_dict().items()}
    opt = torch.optim.Adam(list(sd.values()), lr=hp["learning_rate"], weight_decay=hp["weight_decay"])
    return lambda x, y: O.torch_step(sd, opt, x, y, cfg, cfg["dropout"])


def window(fn, x, y, steps, sync):
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn(x, y)
    sync()
    return (time.perf_counter() - t0) / steps * 1e6


def trace(fn, x, y, steps):
    from torch.profiler import ProfilerActivity, profile
    for _ in range(5):
        fn(x, y)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(steps):
            fn(x, y)
        torch.cuda.synchronize()
    rows = [(e.key, e.count, e.device_time_total if hasattr(e, "device_time_total") else e.cuda_time_total) for e in prof.key_averages()]
    rows = [r for r in rows if r[2] > 0]
    rows.sort(key=lambda r: -r[2])
    return sum(r[1] for r in rows) / steps, sum(r[2] for r in rows) / steps, [(k, c / steps, t / steps) for k, c, t in rows]


def attention_bytes(cfg, B, bwd):
    """(what the attention kernels of one step are built to move, the one-read-one-write minimum 2 N C 4 per graph and layer).  Forward:
    Z once for the scores, three rows per node again (cache-resident) and h written -- counted as 2 reads + 1 write; backward: Z and the
    pair (d h, h) for the band's dot products and again for d Z, d Z written -- counted as 2 x 3 reads + 1 write."""
    rows = B * cfg["num_patch"]
    built = sum(4 * rows * c * (7 if bwd else 3) for c in cfg["hidden_dim"])
    return built, sum(4 * rows * c * 2 for c in cfg["hidden_dim"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(ROWS))
    ap.add_argument("--batches", nargs="+", type=int, default=[100, 1024])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", nargs=2, metavar=("SHAPE", "BATCH"), default=None)
    ap.add_argument("--form", choices=["a", "c"], default="a")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_gatlstm.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    def batch(cfg, B):
        return torch.randn(B, cfg["num_patch"] * cfg["patch_size"], device=dev), torch.rand(B, 1, device=dev)

    if args.trace:
        shape, B = args.trace[0], int(args.trace[1])
        cfg, hp = config(shape)
        fn = fused_step_fn(dev, cfg, hp) if args.form == "a" else torch_step_fn(dev, cfg, hp)
        launches, dev_us, rows = trace(fn, *batch(cfg, B), 10)
        emit(form=args.form, shape=shape, batch=B, launches_per_step=launches, kernel_us_per_step=dev_us)
        if args.form == "a":
            for tag, bwd in (("gl_att_fwd", False), ("gl_att_bwd", True)):
                us = sum(t for k, _, t in rows if tag in k)
                built, least = attention_bytes(cfg, B, bwd)
                emit(kernel_group=tag, us_per_step=us, share_of_kernel_time=us / dev_us if dev_us else None, built_bytes_per_graph=built / B,
                     minimum_bytes_per_graph=least / B, gbytes_per_s_at_minimum=least / us / 1e3 if us else None)
        for k, c, t in rows[:20]:
            emit(kernel=k[:96], per_step=c, us_per_step=t)
    else:
        for shape in args.shapes:
            cfg, hp = config(shape)
            fns = {"a_fused": fused_step_fn(dev, cfg, hp), "c_torch_gpu": torch_step_fn(dev, cfg, hp)}
            for B in args.batches:
                x, y = batch(cfg, B)
                steps = max(5, min(args.steps, 4000 // B))
                times = {k: [] for k in fns}
                for k, fn in fns.items():
                    window(fn, x, y, min(args.warmup, steps), sync)
                for _ in range(args.windows):                   # alternate the forms: same machine state for both
                    for k, fn in fns.items():
                        times[k].append(window(fn, x, y, steps, sync))
                for k, v in times.items():
                    v = sorted(v)
                    emit(form=k, device=torch.cuda.get_device_name(0), shape=shape, batch=B, step_us=v[len(v) // 2], min_us=v[0], max_us=v[-1],
                         steps=steps, windows=args.windows)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
