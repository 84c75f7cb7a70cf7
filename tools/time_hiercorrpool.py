"""Time one HierCorrPool training step on the GPU at the reference's FD001, FD004 and N-CMAPSS wirings (hidden 10, embedding 10, six
pooled nodes), in two forms per batch size:

  (a) ``HierCorrPool.update``: the kernels of csrc/hiercorrpool.hip + the shared SGEMM + fused Adam, one C call;
  (c) the torch restatement of tests/hiercorrpool_oracle.py on the GPU (ATen conv1d / batch_norm / max_pool1d / bmm, torch.optim.Adam):
      what a user of the reference's model gets on this card.

    python tools/time_hiercorrpool.py [--shapes fd001 fd004 ncmapss] [--batches 100 1024] [--steps 100] [--warmup 10] [--out FILE]
    python tools/time_hiercorrpool.py --trace fd001 100 [--form a|c]      # a run of its own: launches per step and the per-kernel split

The two forms alternate in windows inside one process so that they see the same machine state; every window ends in a device
synchronise.  ``--trace`` runs a few steps of one form under the HIP activity tracer (torch.profiler) and prints the kernel launches
per step and the time per kernel name.  One JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LR, WD = 1e-3, 1e-4


def config(shape):
    from gnn_rul_benchmarking_amd.hparams import get_hparams_class
    h = get_hparams_class("NCMAPSS")(None) if shape == "ncmapss" else get_hparams_class("CMAPSS")(shape.upper())
    return dict(h.alg_hparams["HierCorrPool"])


def fused_step_fn(dev, cfg):
    from gnn_rul_benchmarking_amd.algorithms import HierCorrPool
    torch.manual_seed(0)
    algo = HierCorrPool(cfg, {"learning_rate": LR, "weight_decay": WD}, dev)
    algo.to(dev)
    algo.train()
    algo.sync_loss = False
    return lambda x, y: algo.update(x, y, 1)


def torch_step_fn(dev, cfg):
    import hiercorrpool_oracle as O
    from gnn_rul_benchmarking_amd.hiercorrpool import HierCorrPool_model
    torch.manual_seed(0)
    sd = {k: v.detach().clone().to(dev) for k, v in HierCorrPool_model(**cfg).state_dict().items()}
    for k in O.param_names():
        sd[k].requires_grad_(True)
    opt = torch.optim.Adam([sd[k] for k in O.param_names()], lr=LR, weight_decay=WD)
    return lambda x, y: O.torch_step(sd, opt, x, y, cfg)


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


def batch(dev, cfg, B):
    return torch.rand(B, cfg["num_nodes"], cfg["num_patch"] * cfg["patch_size"], device=dev), torch.rand(B, 1, device=dev)


def main(shapes=("fd001", "fd004", "ncmapss"), config=config, fused_step_fn=fused_step_fn, torch_step_fn=torch_step_fn, make_batch=batch):
    """``tools/time_hiercorrpool_bearing.py`` runs this with its own wirings, step functions and inputs."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(shapes))
    ap.add_argument("--batches", type=int, nargs="+", default=[100, 1024])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", nargs=2, metavar=("SHAPE", "BATCH"), default=None)
    ap.add_argument("--form", choices=["a", "c"], default="a")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_hiercorrpool.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    def batch(cfg, B):
        return make_batch(dev, cfg, B)

    if args.trace:
        cfg, B = config(args.trace[0]), int(args.trace[1])
        fn = fused_step_fn(dev, cfg) if args.form == "a" else torch_step_fn(dev, cfg)
        launches, dev_us, rows = trace(fn, *batch(cfg, B), 10)
        emit(form=args.form, shape=args.trace[0], batch=B, launches_per_step=launches, kernel_us_per_step=dev_us)
        for k, c, t in rows[:24]:
            emit(kernel=k[:96], per_step=c, us_per_step=t)
    else:
        for shape in args.shapes:
            cfg = config(shape)
            fns = {"a_fused": fused_step_fn(dev, cfg), "c_torch_gpu": torch_step_fn(dev, cfg)}
            for B in args.batches:
                x, y = batch(cfg, B)
                steps = max(10, min(args.steps, 20000 // B))
                times = {k: [] for k in fns}
                for k, fn in fns.items():
                    window(fn, x, y, args.warmup, sync)
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
