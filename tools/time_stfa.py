"""Time one STFA training step (forward + backward + Adam) on the GPU at the reference's one wiring (C-MAPSS FD001-FD004: 25 patches of
2 points, 14 nodes, 10 heads of width 5, LSTM 95 -> 64), in two forms per batch size:

  (a) ``STFA.update``: the fused graph-attention kernels of csrc/stfa.hip + the LSTM kernels + the last-step head + fused Adam, one C call;
  (c) the torch restatement of tests/stfa_oracle.py on the GPU, computed the reference's way -- the pair tensor cat(Wh_i, Wh_j), the
      repeated dense adjacency and the v / tanh / singleton-softmax branch included, the LSTM on the vendor kernel behind nn.LSTM
      (torch._VF.lstm) -- with torch's dropout and torch.optim.Adam: what a user of the reference's model gets on this card.

    python tools/time_stfa.py [--batches 100 1024] [--steps 100] [--warmup 10] [--out FILE]
    python tools/time_stfa.py --trace 100 [--form a|c]      # a run of its own: launches per step and the per-kernel split

The two forms alternate in windows inside one process so that they see the same machine state; every window ends in a device
synchronise.  ``--trace`` runs a few steps of one form under the HIP activity tracer (torch.profiler) and prints the kernel launches per
step, the time per kernel name, the two attention kernels' share and their bytes per graph against what they must move: the x tile in
(14 P floats) and the LSTM's input row out (T + 14 C floats) for the forward; the x tile, the row and its gradient in for the backward.
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


def config():
    from gnn_rul_benchmarking_amd.hparams import get_hparams_class
    h = get_hparams_class("CMAPSS")("FD001")
    return dict(h.alg_hparams["STFA"]), dict(h.train_params["STFA"])


def fused_step_fn(dev, cfg, hp):
    from gnn_rul_benchmarking_amd.algorithms import STFA
    torch.manual_seed(0)
    algo = STFA(cfg, hp, dev)
    algo.to(dev)
    algo.train()
    algo.sync_loss = False
    return lambda x, y: algo.update(x, y, 1)


def torch_step_fn(dev, cfg, hp):
    import stfa_oracle as O
    from gnn_rul_benchmarking_amd.stfa import STFA_model
    torch.manual_seed(0)
    sd = {k: v.detach().clone().to(dev).requires_grad_(True) for k, v in STFA_model(**cfg).state_dict().items()}
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


def attention_bytes(cfg, bwd):
    """(bytes per graph the attention kernel is built to move, bytes per graph it must move).  Must: x in and the row out (forward); x, the
    row's features (the ReLU gate) and their gradient in (backward).  Built: the same, plus in the backward one read and one write of the
    wavefront's partial row of Hd (C P + 3 C + 1) gradients per graph -- traffic that stays in L2 (a row is 1 KB and its wavefront's
    alone) but is issued.  The parameters (read once per graph, cache-resident) are not counted."""
    x = 4 * 14 * cfg["patch_size"]
    feat = 4 * 14 * cfg["output_dim"]
    row = 4 * cfg["num_patch"] + feat
    part = 4 * cfg["num_heads"] * (cfg["output_dim"] * cfg["patch_size"] + 3 * cfg["output_dim"] + 1)
    must = x + 2 * feat if bwd else x + row
    return (must + 2 * part if bwd else must), must


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", nargs="+", type=int, default=[100, 1024])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", type=int, metavar="BATCH", default=None)
    ap.add_argument("--form", choices=["a", "c"], default="a")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_stfa.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    lines = []
    cfg, hp = config()

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    def batch(B):
        return torch.randn(B, cfg["num_nodes"], cfg["num_patch"] * cfg["patch_size"], device=dev), torch.rand(B, 1, device=dev)

    if args.trace is not None:
        B = args.trace
        fn = fused_step_fn(dev, cfg, hp) if args.form == "a" else torch_step_fn(dev, cfg, hp)
        launches, dev_us, rows = trace(fn, *batch(B), 10)
        emit(form=args.form, batch=B, launches_per_step=launches, kernel_us_per_step=dev_us)
        if args.form == "a":
            G = B * cfg["num_patch"]
            for tag, bwd in (("sf_att_fwd", False), ("sf_att_bwd", True)):
                us = sum(t for k, _, t in rows if tag in k)
                built, must = attention_bytes(cfg, bwd)
                emit(kernel_group=tag, us_per_step=us, share_of_kernel_time=us / dev_us if dev_us else None, graphs=G,
                     built_bytes_per_graph=built, must_move_bytes_per_graph=must, gbytes_per_s_at_must=must * G / us / 1e3 if us else None)
        for k, c, t in rows[:20]:
            emit(kernel=k[:96], per_step=c, us_per_step=t)
    else:
        fns = {"a_fused": fused_step_fn(dev, cfg, hp), "c_torch_gpu": torch_step_fn(dev, cfg, hp)}
        for B in args.batches:
            x, y = batch(B)
            steps = max(5, min(args.steps, 40000 // B))
            times = {k: [] for k in fns}
            for k, fn in fns.items():
                window(fn, x, y, min(args.warmup, steps), sync)
            for _ in range(args.windows):                   # alternate the forms: same machine state for both
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
