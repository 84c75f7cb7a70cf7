"""Tiled-path ST_GCN step with and without synchronised BatchNorm in a world of one: ms per forward + backward call.

    python tools/time_tiled_syncbn.py [plain|all] [N:P:B ...]          (default: all 1024:32:100 1024:32:1024 160:16:100)

plain  ``fused_mse_step`` (rulgnn_stgcn_train_step_path_f32 without an optimizer);
keep   the synchronised entry with a Python callback that leaves the cells as they are: the 4 L collapse launches + callbacks alone;
group  ... with ``torch.distributed.all_reduce`` on the process group (RCCL, world size 1) as the cell reduction;
peer   ... with the one-shot all-reduce over peer mailboxes (dp.PeerAllReduce, world size 1): no Python frame between the kernels.
(sync) minus (plain) is the price of synchronised BatchNorm on one device; what two devices add is not measured here."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from benchlib.common import event_time_ms
from gnn_rul_benchmarking_amd.stgcn import ST_GCN_model

dev = torch.device("cuda:0")
args = sys.argv[1:]
mode = args.pop(0) if args and args[0] in ("plain", "all") else "all"
cases = [tuple(int(v) for v in a.split(":")) for a in args] or [(1024, 32, 100), (1024, 32, 1024), (160, 16, 100)]
peer = None
if mode == "all":
    import torch.distributed as dist
    from gnn_rul_benchmarking_amd.dp import PeerAllReduce
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    peer = PeerAllReduce()


def best(fn):
    return min(event_time_ms(fn, 20, warm=5) for _ in range(3))


for N, P, B in cases:
    torch.manual_seed(0)
    m = ST_GCN_model(N, P, num_layers=2, dropout=0.3).to(dev).train()
    x, y = torch.rand(B, N, P, device=dev), torch.rand(B, 1, device=dev)
    row = {"plain": best(lambda: m.fused_mse_step(x, y, update_running_stats=False))}
    if mode == "all":
        row["keep"] = best(lambda: m.fused_mse_step_syncbn(x, y, B, 0, 1.0, lambda v: None))
        row["group"] = best(lambda: m.fused_mse_step_syncbn(x, y, B, 0, 1.0, lambda v: dist.all_reduce(v)))
        row["peer"] = best(lambda: m.fused_mse_step_syncbn(x, y, B, 0, 1.0, peer))
        row["plain_again"] = best(lambda: m.fused_mse_step(x, y, update_running_stats=False))
    print(f"{N}x{P} batch {B}: " + ", ".join(f"{k} {v:.4f} ms" for k, v in row.items()), flush=True)
    del m, x, y
if peer is not None:
    peer.check()
    peer.close()
    dist.destroy_process_group()
