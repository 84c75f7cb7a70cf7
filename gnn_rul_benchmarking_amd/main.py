"""CLI with the reference's flags (main.py:12-34) plus the data-parallel additions.

    python -m gnn_rul_benchmarking_amd.main --GNN_method ST_GCN --dataset CMAPSS --dataset_id FD004 --device cuda:0
    python -m gnn_rul_benchmarking_amd.main --GNN_method STFA --dataset CMAPSS --dataset_id FD001 --device cuda:0
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m gnn_rul_benchmarking_amd.main ...
    python -m gnn_rul_benchmarking_amd.main --GNN_method HAGCN --dataset_id FD004 --num_runs 5 --concurrent_runs 5      # the five seeds stepped together (runs.py)

``--GNN_method`` takes the reference's names (main.py:43-46).  Aero-engine datasets (CMAPSS, NCMAPSS): ASTGCNN, GRU_CM, HAGCN, ST_Conv, STFA
(CMAPSS only), RGCNU, STGNN, STAGNN, FC_STGNN, HierCorrPool, LOGO, DVGTformer; bearing datasets (PHM2012, XJTU_SY): STNet, SAGCN, ST_GCN,
GAT_LSTM, GDAGDL, STMSGCN, AGCN_TF, LOGO_bearing, HierCorrPool_bearing; ST_GCN also runs on the aero-engine datasets (hparams.py).
"""
import argparse
import os


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument('--save_dir', default='experiments_logs', type=str)
    p.add_argument('--experiment_description', default='Test_', type=str)
    p.add_argument('--run_description', default='test', type=str)
    p.add_argument('--GNN_method', default='ST_GCN', type=str)
    p.add_argument('--data_path', default=r'./Data_Process/Processed_dataset', type=str)
    p.add_argument('--dataset', default='CMAPSS', type=str)
    p.add_argument('--dataset_id', default='FD004', type=str)
    p.add_argument('--bearing_id', default='Testing_bearing_1', type=str)
    p.add_argument('--num_runs', default=5, type=int)
    p.add_argument('--device', default='cuda:0', type=str)
    # additions
    p.add_argument('--window', default=None, type=int, help='C-MAPSS window length (= ST_GCN patch_size); data decides')
    p.add_argument('--num_epochs', default=None, type=int, help='override the table value (81)')
    p.add_argument('--concurrent_runs', default=1, type=int,
                   help='step this many of the --num_runs runs together on the device (HAGCN, DVGTformer and LOGO; single process, at most 8); '
                        '1: one after the other')
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    import torch
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        local = int(os.environ.get("LOCAL_RANK", "0"))
        args.device = f"cuda:{local}"
        torch.cuda.set_device(local)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.distributed.init_process_group("nccl", device_id=torch.device(args.device))
    from .trainer import GNN_RUL_trainer
    GNN_RUL_trainer(args).train()
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
