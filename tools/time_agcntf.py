"""Time one AGCN_TF training step on the GPU at the reference's three wirings (40 x 64, 128 x 256, 256 x 128 with hidden 100 / 100, one
head), in two forms per batch size:

  (a) ``AGCN_TF.update``: SAGCN's front end + the kernels of csrc/agcntf.hip + fused Adam, one C call;
  (c) the vectorised torch restatement of tests/agcntf_oracle.py on the GPU (ATen, torch.optim.Adam): what a user of the reference's
      model gets on this card once its per-patch Python loops are batched.

    python tools/time_agcntf.py [--shapes 40x64 128x256 256x128] [--batches 100 1024] [--steps 100] [--warmup 10] [--out FILE]
    python tools/time_agcntf.py --trace 40x64 100 [--form a|c]      # a run of its own: launches per step and the per-kernel split

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

HA = HG = 100
LR, WD = 1e-4, 1e-4


def fused_step_fn(dev, P, n):
    from gnn_rul_benchmarking_amd.algorithms import AGCN_TF
    torch.manual_seed(0)
    algo = AGCN_TF({"num_patch": P, "patch_size": n, "hidden_adj_dim": HA, "hidden_gnn_dim": HG}, {"learning_rate": LR, "weight_decay": WD}, dev)
    algo.to(dev)
    algo.train()
    algo.sync_loss = False
    return lambda x, y: algo.update(x, y, 1)


def torch_step_fn(dev, P, n):
    import agcntf_oracle as O
    from gnn_rul_benchmarking_amd.agcntf import AGCN_TF_model
    torch.manual_seed(0)
    sd = AGCN_TF_model(P, n, HA, HG).state_dict()
    p = {k: torch.nn.Parameter(v.detach().clone().to(dev)) for k, v in sd.items()}
    opt = torch.optim.Adam(list(p.values()), lr=LR, weight_decay=WD)
    return lambda x, y: O.torch_step(p, opt, x, y, P, n)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["40x64", "128x256", "256x128"])
    ap.add_argument("--batches", type=int, nargs="+", default=[100, 1024])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", nargs=2, metavar=("SHAPE", "BATCH"), default=None)
    ap.add_argument("--form", choices=["a", "c"], default="a")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_agcntf.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    if args.trace:
        P, n = (int(v) for v in args.trace[0].split("x"))
        B = int(args.trace[1])
        fn = fused_step_fn(dev, P, n) if args.form == "a" else torch_step_fn(dev, P, n)
        x, y = torch.rand(B, P * n, device=dev) * 2 - 1, torch.rand(B, 1, device=dev)
        launches, dev_us, rows = trace(fn, x, y, 10)
        emit(form=args.form, shape=args.trace[0], batch=B, launches_per_step=launches, kernel_us_per_step=dev_us)
        for k, c, t in rows[:24]:
            emit(kernel=k[:96], per_step=c, us_per_step=t)
    else:
        for shape in args.shapes:
            P, n = (int(v) for v in shape.split("x"))
            fns = {"a_fused": fused_step_fn(dev, P, n), "c_torch_gpu": torch_step_fn(dev, P, n)}
            for B in args.batches:
                x, y = torch.rand(B, P * n, device=dev) * 2 - 1, torch.rand(B, 1, device=dev)
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
