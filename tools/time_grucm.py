"""Time one GRU_CM training step at the FD004 wiring (14 nodes x 50 steps, GRU hidden 64) on the GPU, in three forms per batch size:

  (a) the default path: graph stage + persistent GRU (csrc/gru_seq.hip) + head + fused Adam, one C call;
  (b) the same step with the recurrence on the step-loop GRU (csrc/gru.hip), through the debugging switch ``model.gru_path``;
  (c) the torch restatement of tests/grucm_oracle.py moved to the GPU (ATen + the vendor GRU, torch.optim.Adam): what a user of the
      reference gets on this card.

    python tools/time_grucm.py [--batches 100 256 4096] [--steps 200] [--warmup 20] [--out FILE]
    python tools/time_grucm.py --cpu-baseline          # form (c) on the CPU only (no GPU needed), labelled as such
    python tools/time_grucm.py --once 100              # a few steps of (a) alone, for a kernel trace around this process

(a) and (b) alternate in windows inside one process so that they see the same machine state; every window ends in a device synchronise.
One JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, L, H = 14, 50, 64


def fused_algo(dev, path):
    from gnn_rul_benchmarking_amd.algorithms import GRU_CM
    torch.manual_seed(0)
    algo = GRU_CM({"num_nodes": N, "time_length": L, "gru_hidden_dim": H}, {"learning_rate": 1e-3, "weight_decay": 1e-4}, dev)
    algo.to(dev)
    algo.train()
    algo.sync_loss = False
    algo.model.gru_path = path
    return algo


def torch_step_fn(dev):
    import grucm_oracle as O
    torch.manual_seed(0)
    m = O.torch_model(L, N, H).to(dev)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-4)
    drop = torch.nn.Dropout(0.2)

    def step(x, y):
        bs = x.size(0)
        keep = [drop(torch.ones(bs, L, N, N // 2, device=dev)), drop(torch.ones(bs, L, N, N // 2, device=dev)), drop(torch.ones(bs, L, H, device=dev))]
        loss = torch.nn.functional.mse_loss(m(x, keep), y)
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss
    return step


def window(fn, x, y, steps, sync):
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn(x, y)
    sync()
    return (time.perf_counter() - t0) / steps * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[100, 256, 4096])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--cpu-baseline", action="store_true")
    ap.add_argument("--once", type=int, default=0)
    args = ap.parse_args()
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    if args.cpu_baseline:
        step = torch_step_fn(torch.device("cpu"))
        for B in args.batches:
            x, y = torch.rand(B, N, L), torch.rand(B, 1)
            n = max(3, min(args.steps, 20000 // B))
            window(step, x, y, 2, lambda: None)
            emit(form="c_torch_cpu", device="cpu", batch=B, step_us=window(step, x, y, n, lambda: None), steps=n, threads=torch.get_num_threads())
    else:
        if not torch.cuda.is_available():
            raise SystemExit("time_grucm.py measures on the GPU: none found (use --cpu-baseline for the labelled CPU figure)")
        from gnn_rul_benchmarking_amd import _lib
        dev = torch.device("cuda:0")
        sync = torch.cuda.synchronize
        if args.once:
            algo = fused_algo(dev, _lib.GRUCM_GRU_AUTO)
            x, y = torch.rand(args.once, N, L, device=dev), torch.rand(args.once, 1, device=dev)
            for _ in range(10):
                algo.update(x, y, 1)
            sync()
            return
        forms = {"a_persistent": fused_algo(dev, _lib.GRUCM_GRU_AUTO), "b_step_loop": fused_algo(dev, _lib.GRUCM_GRU_STEP_LOOP)}
        fns = {k: (lambda x, y, a=a: a.update(x, y, 1)) for k, a in forms.items()}
        fns["c_torch_gpu"] = torch_step_fn(dev)
        for B in args.batches:
            x, y = torch.rand(B, N, L, device=dev), torch.rand(B, 1, device=dev)
            steps = max(20, min(args.steps, 400000 // B))
            times = {k: [] for k in fns}
            for k, fn in fns.items():
                window(fn, x, y, args.warmup, sync)
            for _ in range(args.windows):                   # alternate the forms: same machine state for all of them
                for k, fn in fns.items():
                    times[k].append(window(fn, x, y, steps, sync))
            for k, v in times.items():
                v = sorted(v)
                emit(form=k, device=torch.cuda.get_device_name(0), batch=B, step_us=v[len(v) // 2], min_us=v[0], max_us=v[-1], steps=steps,
                     windows=args.windows)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
