#!/usr/bin/env python3
"""Batch consumer: interchange files -> ASR / max-SR / mean-SR -> IoUs per image -> means.  Counterpart of
the reference's SR_single_class.py (same hyper-parameters and IoU record); images sharded over the GPUs of
the node, one all-gather of the per-image IoU records at the end (asr_amd.distributed)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IMG_SIZE = (512, 512)
FEATURE_SIZE = (128, 128)
HYPER = dict(lambda_df=1, lambda_tv=0.3, lambda_L2=0.7, lambda_L1=0.0, num_iter=300, optimizer="adam",
             learning_rate=1e-3, amsgrad=True, lr_scheduler=True, decay_steps=60, decay_rate=0.3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", required=True, help="folder of interchange files written by generate_augmented_copies.py")
    ap.add_argument("--gt", required=True, help="folder of ground-truth label PNGs named <filename>.png")
    ap.add_argument("--standard", default=None, help="folder of standard-output PNGs (optional)")
    ap.add_argument("--num_aug", type=int, default=10)
    ap.add_argument("--num_samples", type=int, default=500)
    ap.add_argument("--class_id", type=int, default=8)
    ap.add_argument("--th_factor", type=float, default=0.65)
    ap.add_argument("--feature_size", type=int, default=FEATURE_SIZE[0],
                    help="side of the stored model outputs: 128 for the Xception copies, 64 for MobileNet (OS 8)")
    ap.add_argument("--out", default=None, help="output folder (default: data/superres_root/superres_output); when given, "
                    "the masks of --extra_sr_types are written there as PNGs")
    ap.add_argument("--extra_sr_types", default="", help="comma-separated one-pass robust fusions to score after the "
                    "reference's six means: median, trimmed_mean, covered_mean, covered_median")
    ap.add_argument("--cover", choices=["frame", "validity"], default="frame", help="what the covered fusions count as "
                    "seen: the output frame only, or also the part of each copy that came from inside the image")
    ap.add_argument("--trim", type=float, default=0.1, help="fraction of the copies the trimmed mean drops at each end")
    ap.add_argument("--df_loss", choices=["l2", "l1", "huber"], default="l2", help="data term of the iterative solve: l2 (the reference's), l1, or huber with threshold --df_delta")
    ap.add_argument("--df_delta", type=float, default=0.1, help="Huber threshold, in units of the stacks (normalised to [0, 1]); finite, > 0")
    ap.add_argument("--sr_stop_tol", type=float, default=None,
                    help="stop each image's iterative solve once its loss has not improved by this relative amount (finite, >= 0; e.g. 1e-4)")
    ap.add_argument("--sr_stop_patience", type=int, default=None, help="evaluations in a row without that improvement before a solve stops (default 3)")
    ap.add_argument("--sr_stop_every", type=int, default=None, help="evaluate the loss every this many iterations (default 1)")
    ap.add_argument("--sr_stop_min_iter", type=int, default=None, help="no solve stops before this iteration (default 0)")
    ap.add_argument("--sr_adjoint", choices=["registered", "exact"], default="registered",
                    help="the data-term gradient of the iterative solve: TensorFlow's registered gradient of the rotate (the reference's) or its exact transpose")
    ap.add_argument("--sr_reweight", choices=["cauchy", "hard"], default=None,
                    help="down-weight whole unreliable copies inside the iterative solve: each copy's residual energy against --sr_reweight_kappa times the median over the copies")
    ap.add_argument("--sr_reweight_kappa", type=float, default=None, help="a copy at this many times the median energy gets weight 1/2 (cauchy) or is the last kept (hard); finite, > 0 (default 2)")
    ap.add_argument("--sr_reweight_every", type=int, default=None, help="reweight every this many iterations (default 10)")
    ap.add_argument("--sr_reweight_start", type=int, default=None, help="first reweighting iteration (default 10)")
    ap.add_argument("--sr_optimizer", choices=["primal_dual"], default=None,
                    help="update rule of the iterative solve: primal_dual needs no learning rate (default: the reference's AMSGrad schedule)")
    ap.add_argument("--pd_bound_iters", type=int, default=None, help="repetitions of the primal-dual step bound, 1..64 (default 6); needs --sr_optimizer primal_dual")
    args = ap.parse_args()
    from asr_amd.ops import check_data_term
    from asr_amd.superresolution_scripts.optimizer import Optimizer
    from asr_amd.superresolution_scripts.superresolution import Superresolution as _Sr
    try:
        check_data_term(args.df_loss, args.df_delta, "--df_loss/--df_delta")
        optimizer_obj = Optimizer.from_flags(HYPER, args.sr_optimizer, args.pd_bound_iters, args.df_loss)
    except ValueError as e:
        ap.error(str(e))
    stop_kw = {k: v for k, v in (("stop_patience", args.sr_stop_patience), ("stop_every", args.sr_stop_every),
                                 ("stop_min_iter", args.sr_stop_min_iter)) if v is not None}
    if args.sr_stop_tol is None:
        if stop_kw:
            ap.error("--sr_stop_patience, --sr_stop_every and --sr_stop_min_iter need --sr_stop_tol")
    else:
        stop_kw["stop_rel_tol"] = args.sr_stop_tol
        try:
            _Sr.check_stop(**stop_kw)
        except ValueError as e:
            ap.error(f"--sr_stop_*: {e}")
    rw_flags = {"kappa": args.sr_reweight_kappa, "every": args.sr_reweight_every, "start": args.sr_reweight_start}
    sr_reweight = None
    if args.sr_reweight is None:
        if any(v is not None for v in rw_flags.values()):
            ap.error("--sr_reweight_kappa, --sr_reweight_every and --sr_reweight_start need --sr_reweight")
    else:
        sr_reweight = dict({k: v for k, v in rw_flags.items() if v is not None}, kind=args.sr_reweight)
        try:
            from asr_amd.ops import check_sr_reweight
            check_sr_reweight(sr_reweight, "--sr_reweight_*")
        except ValueError as e:
            ap.error(str(e))
    extra = tuple(t for t in args.extra_sr_types.split(",") if t)
    out_dir = args.out or os.path.join(ROOT, "data", "superres_root", "superres_output")

    import torch
    from asr_amd import distributed as D
    from asr_amd.evaluation import evaluate_precomputed, interchange_files, mean_over_valid, valid_rows
    from asr_amd.superresolution_scripts.superresolution import Superresolution

    rank, world, local_rank = D.init_from_env()
    torch.cuda.set_device(local_rank)
    sr =Superresolution(lambda_df=HYPER["lambda_df"], lambda_tv=HYPER["lambda_tv"], lambda_L2=HYPER["lambda_L2"],
                         lambda_L1=HYPER["lambda_L1"], num_iter=HYPER["num_iter"], num_aug=args.num_aug,
                         optimizer=optimizer_obj, feature_size=(args.feature_size, args.feature_size), trim=args.trim,
                         cover=args.cover, df_loss=args.df_loss, df_delta=args.df_delta, **stop_kw,
                         **(dict(adjoint="exact") if args.sr_adjoint == "exact" else {}),
                         **Superresolution.reweight_keywords(sr_reweight))
    paths = interchange_files(args.data)[:args.num_samples]
    res = evaluate_precomputed(sr, paths, args.gt, args.standard, num_aug=args.num_aug, class_id=args.class_id,
                               th_factor=args.th_factor, img_size=IMG_SIZE, out_dir=out_dir, rank=rank, world=world,
                               extra_sr_types=extra, save_extra_output=bool(extra) and args.out is not None)
    table, valid = res[0], res[1]
    if rank == 0:
        m = mean_over_valid(table, valid)
        print(f"Avg. Standard IoUs (No bg): {m['standard_single']},  Avg. Augmented SR IoUs (No bg): {m['aug_single']}")
        print(f"Avg. Standard IoUs (with bg): {m['standard_bg']},  Avg. Augmented SR IoUs (with bg): {m['aug_bg']}")
        print(f"Avg. Max SR IoUs: {m['max']}, Avg. Mean SR IoUs: {m['mean']}")
        if extra:
            import numpy as np
            rows = valid_rows(res[2], valid)
            for j, t in enumerate(extra):
                mean = float(np.mean(rows[:, j])) if len(rows) else float("nan")
                print(f"Avg. {t.replace('_', ' ').capitalize()} SR IoUs: {mean}")
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
