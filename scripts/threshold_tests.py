#!/usr/bin/env python3
"""Threshold-factor test over precomputed SR data: the reference's threshold_tests.py, offline.

Each valid image is solved once with threshold_tests.py's hyper-parameters (lambdas normalised with
normalize_coefficients, copy_dropout 0.2, lr 0.1, decay 100 / 0.65) and its aug-SR target is scored single-class at the 17
factors 0.10, 0.15, ..., 0.90 (no th_mask, also for slice_max files), all in one threshold-sweep launch.  Writes
``th_<mode>_<num_samples>.csv`` in DataFrame.to_csv's layout (header ``,Th_Value,IoU``) and prints the best record and
the standard IoU.

Deviations from the reference, on purpose:
- The means are over the VALID images.  The reference averages an np.empty array of NUM_SAMPLES columns, whose columns of
  skipped or missing files hold whatever the allocation held.
- Images are evaluated by asr_amd.sweep.sweep_precomputed, so the optimizer's global step counter advances like
  SR_single_class.py's: two solves for a slice_max file (class map and max map), where the reference's threshold test
  solves the class map only."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IMG_SIZE = (512, 512)
FEATURE_SIZE = (128, 128)
NUM_AUG = 100
NUM_SAMPLES = 500


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", required=True, help="folder of interchange files written by generate_augmented_copies.py")
    ap.add_argument("--gt", required=True, help="folder of ground-truth label PNGs named <filename>.png")
    ap.add_argument("--standard", default=None, help="folder of standard-output PNGs (optional)")
    ap.add_argument("--num_aug", type=int, default=NUM_AUG)
    ap.add_argument("--num_samples", type=int, default=NUM_SAMPLES)
    ap.add_argument("--class_id", type=int, default=8)
    ap.add_argument("--mode", default="slice_var", help="name of the OPM mode, used in the CSV file name")
    ap.add_argument("--feature_size", type=int, default=FEATURE_SIZE[0],
                    help="side of the stored model outputs: 128 for the Xception copies, 64 for MobileNet (OS 8)")
    ap.add_argument("--out", default=os.path.join(ROOT, "data", "threshold_test"), help="folder of the CSV")
    args = ap.parse_args()

    import numpy as np
    import torch
    from asr_amd import distributed as D
    from asr_amd import sweep as SW
    from asr_amd.evaluation import interchange_files
    from asr_amd.superresolution_scripts.superres_utils import normalize_coefficients

    np.random.seed(SW.SEED)
    config = dict(SW.THRESHOLD_DEFAULTS)
    coeff = normalize_coefficients({k: config[k] for k in ("lambda_tv", "lambda_L2", "lambda_L1")})
    config.update(coeff)
    rank, world, local_rank = D.init_from_env()
    torch.cuda.set_device(local_rank)
    if rank == 0:
        print(coeff)
    paths = interchange_files(args.data)[:args.num_samples]
    table, thr, valid = SW.sweep_precomputed([config], paths, args.gt, args.standard, num_aug=args.num_aug,
                                             class_id=args.class_id, th_factors=SW.TH_FACTORS, img_size=IMG_SIZE,
                                             feature_size=(args.feature_size, args.feature_size), rank=rank, world=world)
    if rank == 0:
        ious = [float(np.mean(thr[0][valid, k])) for k in range(len(SW.TH_FACTORS))]
        os.makedirs(args.out, exist_ok=True)
        path = os.path.join(args.out, f"th_{args.mode}_{args.num_samples}.csv")
        SW.write_threshold_csv(path, SW.TH_FACTORS, ious)
        for i, (t, v) in enumerate(zip(SW.TH_FACTORS, ious)):
            print(f"{i:>3} Th_Value {t:<5} IoU {v}")
        best = SW.best_index(ious, "maximize")
        if best is None:
            print("Best record: none (every IoU is NaN)")
        else:
            print(f"Best record: Th_Value {SW.TH_FACTORS[best]}, IoU {ious[best]}")
        print(f"Standard IoU: {float(np.mean(table[0][valid, 0]))}")
        print(f"Done: {int(np.sum(valid))} valid images -> {path}")
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
