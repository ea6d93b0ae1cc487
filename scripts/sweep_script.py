#!/usr/bin/env python3
"""Hyper-parameter sweep over precomputed SR data: the reference's sweep_script.py and its wandb agent, offline.

The sweep file is the wandb format the reference ships (configs/sweep_configs/sweep.yaml, sweep_all.yaml): JSON always,
YAML when PyYAML is installed.  ``grid`` expands the value / values parameters; ``random`` draws ``--count``
configurations from a seeded numpy Generator; ``bayes`` needs the wandb service and runs as ``random``.  Unswept
hyper-parameters take sweep_script.py's defaults.  Each interchange file is loaded and uploaded once for all
configurations (asr_amd.sweep.sweep_precomputed); every configuration's IoUs equal those of its own SR_single_class-style
run.  Rank 0 writes one CSV row per configuration (index, every hyper-parameter, the six means over the valid images,
n_valid) and prints the best configuration by the sweep's metric and goal (ties: the lowest index)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IMG_SIZE = (512, 512)
FEATURE_SIZE = (128, 128)
NUM_AUG = 100
TH_FACTOR = 0.65


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweep", required=True, help="wandb sweep file (.json, or .yaml with PyYAML installed)")
    ap.add_argument("--count", type=int, default=None, help="configurations to draw (random / bayes; default: the file's)")
    ap.add_argument("--seed", type=int, default=None, help="seed of the random draws (default: the file's, else 1234)")
    ap.add_argument("--data", required=True, help="folder of interchange files written by generate_augmented_copies.py")
    ap.add_argument("--gt", required=True, help="folder of ground-truth label PNGs named <filename>.png")
    ap.add_argument("--standard", default=None, help="folder of standard-output PNGs (optional)")
    ap.add_argument("--num_aug", type=int, default=NUM_AUG)
    ap.add_argument("--num_samples", type=int, default=500)
    ap.add_argument("--class_id", type=int, default=8)
    ap.add_argument("--th_factor", type=float, default=TH_FACTOR)
    ap.add_argument("--feature_size", type=int, default=FEATURE_SIZE[0],
                    help="side of the stored model outputs: 128 for the Xception copies, 64 for MobileNet (OS 8)")
    ap.add_argument("--out", default="sweep.csv", help="CSV written by rank 0")
    args = ap.parse_args()

    from asr_amd import sweep as SW
    spec = SW.load_spec(args.sweep)
    configs = SW.expand(spec, count=args.count, seed=args.seed)
    metric_col, goal = SW.metric_of(spec)

    import numpy as np
    import torch
    from asr_amd import distributed as D
    from asr_amd.evaluation import interchange_files

    np.random.seed(SW.SEED)
    rank, world, local_rank = D.init_from_env()
    torch.cuda.set_device(local_rank)
    paths = interchange_files(args.data)[:args.num_samples]
    table, _thr, valid = SW.sweep_precomputed(configs, paths, args.gt, args.standard, num_aug=args.num_aug,
                                              class_id=args.class_id, th_factor=args.th_factor, img_size=IMG_SIZE,
                                              feature_size=(args.feature_size, args.feature_size), rank=rank, world=world)
    if rank == 0:
        means = SW.means_per_config(table, valid)
        n_valid = int(np.sum(valid))
        SW.write_sweep_csv(args.out, configs, means, n_valid)
        field = D.IOU_FIELDS[metric_col]
        name = next(k for k, v in SW.METRICS.items() if v == field)
        best = SW.best_index([m[field] for m in means], goal)
        print(f"{len(configs)} configurations x {n_valid} valid images -> {args.out}")
        if best is None:
            print(f"Best configuration: none ({name} is NaN for every configuration)")
        else:
            swept = {k: configs[best][k] for k in (spec.get("parameters") or {})}
            print(f"Best configuration: index {best}, {name} = {means[best][field]} ({goal}), {swept}")
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
