#!/usr/bin/env python3
"""Per-class validation table in one run: every image goes through DeepLabV3+ ONCE for all the classes its ground truth
holds (HotPath.run_image_classes), where the reference runs generate_augmented_copies.py + SR_single_class.py once per class.
Writes the reference's experiments_data/final_validations/*.csv layout ("Name", the six IoU means, one "Class c" row per
class found in at least one image) plus a column n_images.

Each class keeps the reference's single-class meaning (scripts/validate_labelmap.py fuses them into label maps).  One augmentation draw
serves all classes of an image: image g gets draw g of the seeded stream over the whole --images list, where a reference
per-class run draws along its own filtered list -- so each row equals a per-class run FED THE SAME DRAWS.  The Adam step
counter of class c on image g is what a per-class run over the images holding c reaches (asr_amd.evaluation.evaluate_classes).
With one process per GPU (torch.distributed.run) images are dealt round-robin over the ranks; one all-gather at the end."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 1234
IMG_SIZE = (512, 512)
BATCH_SIZE = 16
# SR_single_class.py's solver constants (num_iter from --num_iter)
HYPER = dict(lambda_df=1, lambda_tv=0.3, lambda_L2=0.7, lambda_L1=0.0, optimizer="adam", learning_rate=1e-3, amsgrad=True,
             lr_scheduler=True, decay_steps=60, decay_rate=0.3)

parser = argparse.ArgumentParser()
parser.add_argument("--images", required=True, help="folder of .jpg images or a text file with one path per line")
parser.add_argument("--gt", required=True, help="folder of ground-truth label PNGs named <image stem>.png")
parser.add_argument("--num_aug", help="Number of augmented copies created for each image", type=int, default=100)
parser.add_argument("--num_samples", help="Number of samples taken from the list", type=int, default=500)
parser.add_argument("--mode", type=str, choices=["slice_max", "slice", "argmax"], default="argmax")
parser.add_argument("--angle_max", help="Max angle value (in radians) used for rotations", type=float, default=0.3)
parser.add_argument("--shift_max", help="Max shift value used for traslations", type=int, default=30)
parser.add_argument("--backbone", type=str, choices=["mobilenet", "xception"], default="xception")
parser.add_argument("--weights", default=None, help="local Keras .h5 checkpoint or .npz of Keras weights")
parser.add_argument("--th_factor", type=float, default=0.65)
parser.add_argument("--num_iter", type=int, default=300)
parser.add_argument("--df_loss", choices=["l2", "l1", "huber"], default="l2", help="data term of the iterative solve: l2 (the reference's), l1, or huber with threshold --df_delta")
parser.add_argument("--df_delta", type=float, default=0.1, help="Huber threshold, in units of the stacks (normalised to [0, 1]); finite, > 0")
parser.add_argument("--sr_adjoint", choices=["registered", "exact"], default="registered",
                    help="the data-term gradient of the iterative solve: TensorFlow's registered gradient of the rotate (the reference's) or its exact transpose")
parser.add_argument("--sr_reweight", choices=["cauchy", "hard"], default=None,
                    help="down-weight whole unreliable copies inside the iterative solve: each copy's residual energy against --sr_reweight_kappa times the median over the copies")
parser.add_argument("--sr_reweight_kappa", type=float, default=None, help="a copy at this many times the median energy gets weight 1/2 (cauchy) or is the last kept (hard); finite, > 0 (default 2)")
parser.add_argument("--sr_reweight_every", type=int, default=None, help="reweight every this many iterations (default 10)")
parser.add_argument("--sr_reweight_start", type=int, default=None, help="first reweighting iteration (default 10)")
parser.add_argument("--sr_optimizer", choices=["primal_dual"], default=None,
                    help="update rule of the iterative solve: primal_dual needs no learning rate (default: the reference's AMSGrad schedule)")
parser.add_argument("--pd_bound_iters", type=int, default=None, help="repetitions of the primal-dual step bound, 1..64 (default 6); needs --sr_optimizer primal_dual")
parser.add_argument("--class_ids", type=int, nargs="+", default=list(range(1, 21)),
                    help="classes to evaluate (0 and 255 never count)")
parser.add_argument("--out", default=os.path.join(ROOT, "data", "superres_root", "class_validation.csv"),
                    help="CSV file to write")


def main():
    args = parser.parse_args()
    from asr_amd.ops import check_data_term
    try:
        check_data_term(args.df_loss, args.df_delta, "--df_loss/--df_delta")
    except ValueError as e:
        parser.error(str(e))
    from asr_amd.superresolution_scripts.optimizer import Optimizer
    try:
        opt = Optimizer.from_flags(HYPER, args.sr_optimizer, args.pd_bound_iters, args.df_loss)
    except ValueError as e:
        parser.error(str(e))
    rw_flags = {"kappa": args.sr_reweight_kappa, "every": args.sr_reweight_every, "start": args.sr_reweight_start}
    sr_reweight = None
    if args.sr_reweight is None:
        if any(v is not None for v in rw_flags.values()):
            parser.error("--sr_reweight_kappa, --sr_reweight_every and --sr_reweight_start need --sr_reweight")
    else:
        sr_reweight = dict({k: v for k, v in rw_flags.items() if v is not None}, kind=args.sr_reweight)
        try:
            from asr_amd.ops import check_sr_reweight
            check_sr_reweight(sr_reweight, "--sr_reweight_*")
        except ValueError as e:
            parser.error(str(e))
    import torch
    from asr_amd import distributed as D
    from asr_amd.evaluation import class_rows, evaluate_classes, write_class_csv
    from asr_amd.model import DeeplabV3Plus
    from asr_amd.pipeline import HotPath
    from asr_amd.superresolution_scripts.superresolution import Superresolution
    from generate_augmented_copies import list_images

    rank, world, local_rank = D.init_from_env()
    torch.cuda.set_device(D.local_device(local_rank))
    paths = list_images(args.images, args.num_samples)
    gts = [os.path.join(args.gt, os.path.splitext(os.path.basename(p))[0] + ".png") for p in paths]
    class_ids = [c for c in dict.fromkeys(args.class_ids) if c not in (0, 255)]
    model = DeeplabV3Plus(input_shape=IMG_SIZE + (3,), classes=21, OS=16, last_activation=None, load_weights=True,
                          backbone=args.backbone, weights_path=args.weights).build_model(final_upsample=False)
    feat = IMG_SIZE[0] // (4 if args.backbone == "xception" else 8)
    sr = Superresolution(lambda_df=HYPER["lambda_df"], lambda_tv=HYPER["lambda_tv"], lambda_L2=HYPER["lambda_L2"],
                         lambda_L1=HYPER["lambda_L1"], num_iter=args.num_iter, num_aug=args.num_aug, optimizer=opt,
                         feature_size=(feat, feat), output_size=IMG_SIZE, df_loss=args.df_loss, df_delta=args.df_delta,
                         **(dict(adjoint="exact") if args.sr_adjoint == "exact" else {}),
                         **Superresolution.reweight_keywords(sr_reweight))
    path = HotPath(model, sr, mode=args.mode, th_factor=args.th_factor, batch_size=BATCH_SIZE)
    table, presence = evaluate_classes(path, paths, gts, class_ids, num_aug=args.num_aug, angle_max=args.angle_max,
                                       shift_max=args.shift_max, img_size=IMG_SIZE, rank=rank, world=world, seed=SEED)
    if rank == 0:
        rows = class_rows(table, presence, class_ids)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        write_class_csv(args.out, rows)
        for name, means, count in rows:
            print(f"{name} ({count} images): " + ", ".join(f"{m:.4f}" for m in means))
        print(f"Wrote {args.out}")
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
