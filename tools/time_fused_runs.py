"""Time R independent DVGTformer or LOGO training runs on one GPU, stepped one after the other and stepped together:

  (s) R consecutive ``update`` calls of R plain algorithms, one per run: the sequential protocol's cost of one step of every run (the
      single-run path, which ``runs.py`` does not change);
  (g) one ``DVGTformer_runs.update`` / ``LOGO_runs.update`` over the same R runs: ONE ``rulgnn_<family>_fwdbwd_group_f32`` call, the
      dominant kernels launched once for all runs with the run in ``blockIdx.y``, the heads, the sums and Adam per run.

    python tools/time_fused_runs.py [--cases dvgtformer:fd001 dvgtformer:ncmapss logo:fd001 logo:fd002 logo:ncmapss] [--runs 2 5]
                                    [--steps 50] [--warmup 10] [--windows 5] [--out FILE]
    python tools/time_fused_runs.py --trace dvgtformer:fd001 5 [--form s|g]      # a run of its own: launches per step, per-kernel split

A case is ``<family>:<wiring>``; the batch is the wiring's own (``train_params['batch_size']``).  The two forms alternate in windows
inside one process so that they see the same machine state; every window ends in a device synchronise; a measurement is the median
window with its minimum and maximum.  Both forms keep the trainer's ``sync_loss`` (one ``loss.item()`` per run and step).  The single
run's guard is ``tools/time_dvgtformer.py`` / ``tools/time_logo.py``, which need nothing of runs.py and so time an older checkout too.
One JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

METHODS = {"dvgtformer": "DVGTformer", "logo": "LOGO"}
DEFAULT_CASES = ["dvgtformer:fd001", "dvgtformer:ncmapss", "logo:fd001", "logo:fd002", "logo:ncmapss"]


def config(case):
    from gnn_rul_benchmarking_amd.hparams import get_hparams_class
    family, wiring = case.split(":")
    method = METHODS[family]
    h = get_hparams_class("NCMAPSS")(None) if wiring == "ncmapss" else get_hparams_class("CMAPSS")(wiring.upper())
    cfg, hp = dict(h.alg_hparams[method]), dict(h.train_params[method])
    length = cfg["time_length"] if family == "dvgtformer" else cfg["num_patch"] * cfg["patch_size"]
    return method, cfg, hp, int(hp["batch_size"]), (cfg["num_nodes"], length)


def batches(dev, B, window_shape, R):
    g = torch.Generator(device="cpu").manual_seed(7)
    return [(torch.rand(B, *window_shape, generator=g).to(dev), torch.rand(B, 1, generator=g).to(dev)) for _ in range(R)]


def sequential_fn(dev, method, cfg, hp, data):
    from gnn_rul_benchmarking_amd.algorithms import get_algorithm_class
    algos = []
    for r in range(len(data)):
        torch.manual_seed(r)
        algo = get_algorithm_class(method)(cfg, hp, dev)
        algo.to(dev)
        algo.train()
        algos.append(algo)

    def step():
        for algo, (x, y) in zip(algos, data):
            algo.update(x, y, 1)
    return step


def grouped_fn(dev, method, cfg, hp, data):
    from gnn_rul_benchmarking_amd.runs import get_runs_class
    group = get_runs_class(method)(cfg, hp, dev, range(len(data)))
    group.train()
    xs, ys = [d[0] for d in data], [d[1] for d in data]
    return lambda: group.update(xs, ys, 1)


def window(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def trace(fn, steps):
    from torch.profiler import ProfilerActivity, profile
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
    rows = [(e.key, e.count, e.device_time_total if hasattr(e, "device_time_total") else e.cuda_time_total) for e in prof.key_averages()]
    rows = sorted((r for r in rows if r[2] > 0), key=lambda r: -r[2])
    return sum(r[1] for r in rows) / steps, sum(r[2] for r in rows) / steps, [(k, c / steps, t / steps) for k, c, t in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=DEFAULT_CASES)
    ap.add_argument("--runs", nargs="+", type=int, default=[2, 5])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", nargs=2, metavar=("CASE", "RUNS"), default=None)
    ap.add_argument("--form", choices=["s", "g"], default="g")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_fused_runs.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    def stats(v):
        v = sorted(v)
        return dict(ms=round(v[len(v) // 2], 4), min_ms=round(v[0], 4), max_ms=round(v[-1], 4))

    if args.trace:
        method, cfg, hp, B, shape = config(args.trace[0])
        R = int(args.trace[1])
        fn = (grouped_fn if args.form == "g" else sequential_fn)(dev, method, cfg, hp, batches(dev, B, shape, R))
        launches, dev_us, rows = trace(fn, 5)
        emit(form=args.form, case=args.trace[0], batch=B, runs=R, launches_per_step=launches, kernel_us_per_step=round(dev_us, 1))
        for k, c, t in rows[:16]:
            emit(kernel=k[:110], per_step=c, us_per_step=round(t, 1))
    else:
        for case in args.cases:
            method, cfg, hp, B, shape = config(case)
            for R in args.runs:
                data = batches(dev, B, shape, R)
                fns = {"s_sequential": sequential_fn(dev, method, cfg, hp, data), "g_grouped": grouped_fn(dev, method, cfg, hp, data)}
                times = {k: [] for k in fns}
                for fn in fns.values():
                    window(fn, args.warmup)
                for _ in range(args.windows):                   # alternate the forms: same machine state for both
                    for k, fn in fns.items():
                        times[k].append(window(fn, args.steps))
                seq = stats(times["s_sequential"])
                for k, v in times.items():
                    s = stats(v)
                    emit(form=k, device=torch.cuda.get_device_name(0), case=case, batch=B, runs=R, steps=args.steps, windows=args.windows, **s,
                         ratio_to_sequential=round(s["ms"] / seq["ms"], 4))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
