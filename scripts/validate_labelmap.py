#!/usr/bin/env python3
"""One label map per image and its mean IoU: every image goes through DeepLabV3+ ONCE, the classes of --class_ids are solved
from that pass (those that win no pixel of any copy are left out, which changes no result: argmax mode) and fused into one
label map per SR type (HotPath.run_image_labels; the rule is in include/asr_hip.h at asr_fuse_labels_f32).  The class set is
the same for every image and is never read from the ground truth, so a class predicted where it is absent costs IoU.

Writes a CSV with one row per label the ground truths hold (its IoU from the counts summed over the images, for the standard,
augmented, max and mean label maps) and both means: "dataset_mIoU", the VOC convention (mean over labels of the IoUs from the
summed counts), and "mean_image_mIoU", the reference's (np.mean of the per-image Mean_IOU).  Void (255) never counts.
--save_dir: the label maps as <image stem>_<standard|aug|max|mean>.png.  Draws and Adam step counters as validate_classes.py
(image g gets draw g of the seeded stream; class c of image g starts where g earlier solves of c leave the counter).  With one
process per GPU (torch.distributed.run) images are dealt round-robin over the ranks; one all-gather at the end.

--band_widths 1,2,4,8,16,32 --trimap_out trimap.csv: the trimap curve as well -- each label map scored only on the pixels within
w pixels of a ground-truth label boundary (include/asr_hip.h, "trimap"), void (255) pixels left out, one CSV row per width
(evaluation.write_trimap_csv).  Without these two flags nothing else is computed or written.

--confusion_out conf.csv [--confusion_labels 21] [--class_names FILE]: the confusion matrix of every label map against the ground
truth, summed over the images, in long form (evaluation.write_confusion_csv: key, truth label, predicted label, pixels, share of
the truth label's pixels; "other" holds void and every value outside 0..labels-1), and next to it <stem>_metrics.csv with pixel
accuracy, mean class accuracy, mIoU, frequency-weighted IoU and per-label precision / recall / IoU, once with the other bin left
out (the VOC protocol) and once with it kept as a label (Mean_IOU's convention).  FILE: one label name per line.

--th_factors 0.1,0.15,... or --th_sweep (the 17 factors 0.10 ... 0.90 of threshold_tests.py) [--th_sweep_out FILE]: the curve of
label-map mIoU against the threshold factor, from the SR outputs this one run already holds -- no further forward pass or solve
(include/asr_hip.h at asr_fuse_labels_sweep_counts_f32; not in slice_max mode, where the threshold plays no part).  One CSV row
per factor (evaluation.write_labelmap_threshold_csv) and the best factor per SR type by dataset mIoU on the console.  Without
these flags nothing else is computed or written.

--guide_radius R [--guide_eps E]: every SR score map is refined with the guided filter (include/asr_hip.h, "guided filter";
window radius R in 0..32, regulariser E, default 1e-3) against its own image before the label fusion, which moves the maps'
boundaries onto the image's edges; compare the --band_widths curve with and without it.  Off when omitted: every CSV keeps its
columns either way.

--tv_guide_beta B: the image goes INTO the iterative solve instead -- the TV prior of every "aug" solve is weighted by the image's
own edges (include/asr_hip.h, "edge-weighted TV": w = 1 / (1 + B * |forward difference of the image|^2), B finite and >= 0; 100
is a good start for images in [0, 1]), so a boundary is cheap where the image has an edge and costs full price elsewhere.
Independent of --guide_radius and combinable with it; compare the --band_widths curve with and without it.  Off when omitted:
nothing else is launched and every CSV is what it was.

--crf_iters T [--crf_radius R --crf_dilation D --crf_w_app A --crf_w_smooth S --crf_theta_pos P --crf_theta_rgb C --crf_theta_smooth G
--crf_tau U --crf_standard_conf F]: every SR label map is decided by the windowed CRF (include/asr_hip.h, "windowed CRF": T mean-field
iterations in a (2R+1)^2 window of dilation D) over all classes and the image at once, instead of pixel by pixel: the unaries are
each class's margin over its threshold divided by U (default 0.1), and neighbours that look alike in the image vote jointly.  With
--crf_standard_conf F the standard label map is refined too, from unaries that trust the map with confidence F.  Not in slice_max
mode and not together with --th_sweep / --th_factors.  What it does to real network output is not known: compare the --band_widths
curve with and without it.  Off when omitted: nothing else is launched and every CSV keeps its columns either way.

--couple_classes (needs --sr_optimizer primal_dual; argmax mode; not with --th_sweep / --th_factors or --crf_iters): the classes of an
image are ONE coupled solve (include/asr_hip.h, "multi-label coupling": every pixel's class values stay >= 0 and sum to at most 1, the
rest being "no class"), and the "aug" label map takes the class of largest share wherever that share exceeds the background's -- no
threshold factor plays a part.  The other label maps are untouched.  What it does to real network output is not known: compare the
CSV with and without it.  Off when omitted: nothing else is launched and every CSV is what it was.

--coverages 50,60,70,80,90,100 [--coverage_out FILE] [--uncertainty_dir DIR]: the risk-coverage curve as well -- the variance of
the class stacks over the realigned copies (include/asr_hip.h at asr_realign_moments_f32; utils.uncertainty_map) says where the
copies disagreed, and every label map is scored on each image's p % most certain non-void pixels (asr_binned_class_counts_f32),
with no further forward pass or solve.  One CSV row per percentage (evaluation.write_coverage_csv: dataset mIoU, mean per-image
mIoU and the share actually retained, which is >= p % because ties stay in); a curve that rises as p falls says the map knows
where the labels are wrong.  DIR: sqrt(u), the standard deviation over the copies, per image as <image stem>.npy (+inf where
fewer than two copies saw the pixel).  Without these flags nothing else is computed or written.

--min_region A [--region_connectivity {4,8}] [--regions_out FILE]: every label map is cleaned of its connected regions of fewer than
A pixels before it is scored and saved (include/asr_hip.h, "regions": a small region takes the one value of its non-small
surround, or 0), so every CSV above is the cleaned maps'; FILE (evaluation.write_regions_csv) holds, per label map, how many
regions there were, how many were small, how many pixels changed, and both mIoUs before and after.  Not together with
--th_sweep / --th_factors, whose label maps are never written.  Without --min_region nothing else is computed or written.

--segments_out seg.csv [--segment_labels 21] [--segment_connectivity {4,8}] [--segment_zero] [--class_names FILE]: the region-level
score as well -- the connected segments of every label map matched against those of the ground truth (include/asr_hip.h,
"segments": equal values and IoU > 1/2), summed over the images, in long form (evaluation.write_segments_csv: key, stage, label,
TP, FP, FN, precision, recall, SQ, RQ, PQ and a mean row).  With --min_region the maps before the clean-up are matched too (stage
"raw" next to "final"): fewer FPs at the same TPs says the clean-up removed spurious segments and lost no true one.  Value 0 makes
segments only with --segment_zero.  Not together with --th_sweep / --th_factors.  Without --segments_out nothing else is computed
or written."""
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
parser.add_argument("--class_ids", type=int, nargs="+", default=list(range(1, 21)),
                    help="the class set of every image (0 and 255 are never candidates)")
parser.add_argument("--out", default=os.path.join(ROOT, "data", "superres_root", "labelmap_validation.csv"),
                    help="CSV file to write")
parser.add_argument("--save_dir", default=None, help="folder for the label maps as PNG (not written when omitted)")
parser.add_argument("--band_widths", default=None,
                    help="comma-separated band widths in pixels (1..64, at most 16), e.g. 1,2,4,8,16,32: score the trimap too")
parser.add_argument("--trimap_out", default=None, help="CSV file for the trimap (default: <--out stem>_trimap.csv)")
parser.add_argument("--confusion_out", default=None, help="CSV file for the confusion matrices (not counted when omitted)")
parser.add_argument("--confusion_labels", type=int, default=21, help="labels 0..N-1 of the confusion matrix (1..64)")
parser.add_argument("--class_names", default=None, help="text file with one label name per line (default: the numbers)")
parser.add_argument("--th_factors", default=None,
                    help="comma-separated threshold factors (at most 64), e.g. 0.1,0.15,0.2: the label maps' threshold curve too")
parser.add_argument("--th_sweep", action="store_true", help="the 17 factors 0.10 ... 0.90 of threshold_tests.py as --th_factors")
parser.add_argument("--th_sweep_out", default=None, help="CSV file for the threshold curve (default: <--out stem>_thresholds.csv)")
parser.add_argument("--guide_radius", type=int, default=None,
                    help="refine the SR score maps with the guided filter of this window radius (0..32) against the image")
parser.add_argument("--guide_eps", type=float, default=None, help="the guided filter's regulariser (default 1e-3)")
parser.add_argument("--tv_guide_beta", type=float, default=None,
                    help="weight the solver's TV prior by the image's edges with this beta (finite, >= 0; e.g. 100)")
parser.add_argument("--df_loss", choices=["l2", "l1", "huber"], default="l2", help="data term of the iterative solve: l2 (the reference's), l1, or huber with threshold --df_delta")
parser.add_argument("--df_delta", type=float, default=0.1, help="Huber threshold, in units of the stacks (normalised to [0, 1]); finite, > 0")
parser.add_argument("--df_weights", choices=["maxprob", "margin"], default=None,
                    help="weight every measurement of the solve's data term by the network's confidence there")
parser.add_argument("--sr_stop_tol", type=float, default=None,
                    help="stop each class's iterative solve once its loss has not improved by this relative amount (finite, >= 0; e.g. 1e-4)")
parser.add_argument("--sr_stop_patience", type=int, default=None, help="evaluations in a row without that improvement before a solve stops (default 3)")
parser.add_argument("--sr_stop_every", type=int, default=None, help="evaluate the loss every this many iterations (default 1)")
parser.add_argument("--sr_stop_min_iter", type=int, default=None, help="no solve stops before this iteration (default 0)")
parser.add_argument("--sr_adjoint", choices=["registered", "exact"], default="registered",
                    help="the data-term gradient of the iterative solve: TensorFlow's registered gradient of the rotate (the reference's) or its exact transpose")
parser.add_argument("--sr_reweight", choices=["cauchy", "hard"], default=None,
                    help="down-weight whole unreliable copies inside the iterative solve: each copy's residual energy against --sr_reweight_kappa times the median over the copies")
parser.add_argument("--sr_reweight_kappa", type=float, default=None, help="a copy at this many times the median energy gets weight 1/2 (cauchy) or is the last kept (hard); finite, > 0 (default 2)")
parser.add_argument("--sr_reweight_every", type=int, default=None, help="reweight every this many iterations (default 10)")
parser.add_argument("--sr_reweight_start", type=int, default=None, help="first reweighting iteration (default 10)")
parser.add_argument("--copy_weights_out", default=None, help="CSV file (image, class, copy, weight) of the final weight of every copy in each solve; needs --sr_reweight")
parser.add_argument("--sr_iters_out", default=None, help="CSV file (image, class, iterations) of the iterations each solve ran; needs --sr_stop_tol")
parser.add_argument("--sr_optimizer", choices=["primal_dual"], default=None,
                    help="update rule of the iterative solve: primal_dual needs no learning rate (default: the reference's AMSGrad schedule)")
parser.add_argument("--pd_bound_iters", type=int, default=None, help="repetitions of the primal-dual step bound, 1..64 (default 6); needs --sr_optimizer primal_dual")
parser.add_argument("--couple_classes", action="store_true",
                    help="solve the classes of an image as one coupled problem (x >= 0, sum <= 1 per pixel) and fuse the 'aug' map "
                         "without a threshold; needs --sr_optimizer primal_dual")
parser.add_argument("--crf_iters", type=int, default=None,
                    help="decide the SR label maps with the windowed CRF of this many mean-field iterations (0..32)")
parser.add_argument("--crf_radius", type=int, default=None, help="the CRF's window radius (1..7, default 3)")
parser.add_argument("--crf_dilation", type=int, default=None, help="the CRF window's dilation (radius x dilation <= 16, default 1)")
parser.add_argument("--crf_w_app", type=float, default=None, help="weight of the CRF's appearance kernel (default 4)")
parser.add_argument("--crf_w_smooth", type=float, default=None, help="weight of the CRF's smoothness kernel (default 1)")
parser.add_argument("--crf_theta_pos", type=float, default=None, help="spatial width of the appearance kernel (default 2)")
parser.add_argument("--crf_theta_rgb", type=float, default=None, help="colour width of the appearance kernel (default 0.1)")
parser.add_argument("--crf_theta_smooth", type=float, default=None, help="width of the smoothness kernel (default 1)")
parser.add_argument("--crf_tau", type=float, default=None, help="temperature of the CRF's unaries (default 0.1)")
parser.add_argument("--crf_standard_conf", type=float, default=None,
                    help="also refine the standard label map with the CRF, its unaries from the map at this confidence")
parser.add_argument("--coverages", default=None,
                    help="comma-separated whole percentages (1..100, at most 16), e.g. 50,60,70,80,90,100: the risk-coverage curve too")
parser.add_argument("--coverage_out", default=None, help="CSV file for the risk-coverage curve (default: <--out stem>_coverage.csv)")
parser.add_argument("--uncertainty_dir", default=None, help="folder for sqrt(u) per image as .npy (needs --coverages)")
parser.add_argument("--min_region", type=int, default=None,
                    help="remove connected regions of fewer than this many pixels from every label map before scoring it")
parser.add_argument("--region_connectivity", type=int, choices=[4, 8], default=4, help="the regions' connectivity (default 4)")
parser.add_argument("--regions_out", default=None, help="CSV file for the region statistics (default: <--out stem>_regions.csv)")
parser.add_argument("--segments_out", default=None, help="CSV file for the region-level scores (not matched when omitted)")
parser.add_argument("--segment_labels", type=int, default=21, help="labels 0..N-1 whose regions are segments (1..64)")
parser.add_argument("--segment_connectivity", type=int, choices=[4, 8], default=8, help="the segments' connectivity (default 8)")
parser.add_argument("--segment_zero", action="store_true", help="regions of value 0 are segments too")
parser.add_argument("--no_prune",action="store_true", help="solve every class, also those that win no pixel (same results)")


def main():
    args = parser.parse_args()
    import torch
    from asr_amd import distributed as D
    from asr_amd.evaluation import (LABELMAP_KEYS, best_threshold_factors, dataset_miou, evaluate_labelmaps,
                                    write_confusion_csv, write_confusion_metrics_csv, write_labelmap_csv,
                                    write_coverage_csv, write_labelmap_threshold_csv, write_regions_csv, write_segments_csv,
                                    write_sr_iters_csv, write_trimap_csv)
    from asr_amd.ops import check_coverages, check_crf, check_data_term, check_min_region, check_segments, check_tv_beta
    from asr_amd.model import DeeplabV3Plus
    from asr_amd.pipeline import HotPath
    from asr_amd.superresolution_scripts.optimizer import Optimizer
    from asr_amd.superresolution_scripts.superresolution import Superresolution
    from generate_augmented_copies import list_images

    if args.trimap_out and not args.band_widths:
        parser.error("--trimap_out needs --band_widths")
    bands = [int(v) for v in args.band_widths.split(",")] if args.band_widths else None
    if args.confusion_out and not 1 <= args.confusion_labels <= 64:
        parser.error("--confusion_labels must lie in 1..64")
    factors = None
    if args.th_factors and args.th_sweep:
        parser.error("--th_factors and --th_sweep are two ways to name the factors: give one")
    if args.th_factors:
        factors = [float(v) for v in args.th_factors.split(",")]
    elif args.th_sweep:
        from asr_amd.sweep import TH_FACTORS
        factors = [float(v) for v in TH_FACTORS]
    if args.th_sweep_out and factors is None:
        parser.error("--th_sweep_out needs --th_factors or --th_sweep")
    if factors is not None:
        try:                # their number, and no sweep in slice_max mode: the library's own check, ahead of the model
            HotPath(None, None, mode=args.mode).label_options(None, True, th_factors=factors)
        except ValueError as e:
            parser.error(f"--th_factors / --th_sweep: {e}")
    if args.regions_out and args.min_region is None:
        parser.error("--regions_out needs --min_region")
    min_region = None
    if args.min_region is not None:
        if factors is not None:
            parser.error("--min_region with --th_sweep / --th_factors: the sweep counts label maps that are never written, so "
                         "there is nothing to clean")
        try:
            min_region = check_min_region((args.min_region, args.region_connectivity))
        except ValueError as e:
            parser.error(f"--min_region: {e}")
    segments = None
    if args.segments_out:
        if factors is not None:
            parser.error("--segments_out with --th_sweep / --th_factors: the sweep counts label maps that are never written, so "
                         "there are no segments to match")
        try:
            segments = check_segments((args.segment_labels, args.segment_connectivity, args.segment_zero))
        except ValueError as e:
            parser.error(f"--segment_labels: {e}")
    if args.guide_eps is not None and args.guide_radius is None:
        parser.error("--guide_eps needs --guide_radius")
    guide = None
    if args.guide_radius is not None:
        if not 0 <= args.guide_radius <= 32:
            parser.error("--guide_radius must lie in 0..32")
        guide = (args.guide_radius, 1e-3 if args.guide_eps is None else args.guide_eps)
        if not 0.0 < guide[1] < float("inf"):
            parser.error("--guide_eps must be finite and > 0")
    if args.tv_guide_beta is not None:
        try:
            check_tv_beta(args.tv_guide_beta, "--tv_guide_beta")
        except ValueError as e:
            parser.error(str(e))
    try:
        check_data_term(args.df_loss, args.df_delta, "--df_loss/--df_delta")
        opt = Optimizer.from_flags(HYPER, args.sr_optimizer, args.pd_bound_iters, args.df_loss)
    except ValueError as e:
        parser.error(str(e))
    stop_flags = {"patience": args.sr_stop_patience, "every": args.sr_stop_every, "min_iter": args.sr_stop_min_iter}
    sr_stop = None
    if args.sr_stop_tol is None:
        if args.sr_iters_out or any(v is not None for v in stop_flags.values()):
            parser.error("--sr_stop_patience, --sr_stop_every, --sr_stop_min_iter and --sr_iters_out need --sr_stop_tol")
    else:
        sr_stop = dict({k: v for k, v in stop_flags.items() if v is not None}, rel_tol=args.sr_stop_tol)
        try:
            if HotPath.check_sr_stop(sr_stop)["patience"] < 1:
                raise ValueError("--sr_stop_patience must be >= 1")
        except ValueError as e:
            parser.error(f"--sr_stop_*: {e}")
    rw_flags = {"kappa": args.sr_reweight_kappa, "every": args.sr_reweight_every, "start": args.sr_reweight_start}
    sr_reweight = None
    if args.sr_reweight is None:
        if args.copy_weights_out or any(v is not None for v in rw_flags.values()):
            parser.error("--sr_reweight_kappa, --sr_reweight_every, --sr_reweight_start and --copy_weights_out need --sr_reweight")
    else:
        sr_reweight = dict({k: v for k, v in rw_flags.items() if v is not None}, kind=args.sr_reweight)
        try:
            from asr_amd.ops import check_sr_reweight
            check_sr_reweight(sr_reweight, "--sr_reweight_*")
        except ValueError as e:
            parser.error(str(e))
    crf_flags = {"radius": args.crf_radius, "dilation": args.crf_dilation, "w_app": args.crf_w_app, "w_smooth": args.crf_w_smooth,
                 "theta_pos": args.crf_theta_pos, "theta_rgb": args.crf_theta_rgb, "theta_smooth": args.crf_theta_smooth,
                 "tau": args.crf_tau, "standard_conf": args.crf_standard_conf}
    crf = None
    if args.crf_iters is None:
        if any(v is not None for v in crf_flags.values()):
            parser.error("the --crf_* flags need --crf_iters")
    else:
        crf = dict({k: v for k, v in crf_flags.items() if v is not None}, iterations=args.crf_iters)
        if args.mode == "slice_max":
            parser.error("--crf_iters in slice_max mode: a class passes against its max map there, so there is no unary")
        if factors is not None:
            parser.error("--crf_iters with --th_sweep / --th_factors: the sweep counts the fusion rule's label maps")
        try:                # every field's range: the library's own check, ahead of the model
            check_crf({k: v for k, v in crf.items() if k not in ("tau", "standard_conf")})
        except ValueError as e:
            parser.error(f"--crf_*: {e}")
    if args.couple_classes:
        if args.sr_optimizer != "primal_dual":
            parser.error("--couple_classes needs --sr_optimizer primal_dual: the coupling is a prox step of that rule")
        if args.mode != "argmax":
            parser.error(f"--couple_classes in {args.mode} mode: the classes' normalised stacks do not sum to at most 1 there")
        if factors is not None:
            parser.error("--couple_classes with --th_sweep / --th_factors: the coupled label map has no threshold to sweep")
        if crf is not None:
            parser.error("--couple_classes with --crf_iters: the CRF's unaries are margins over the threshold rule")
    if (args.coverage_out or args.uncertainty_dir) and not args.coverages:
        parser.error("--coverage_out and --uncertainty_dir need --coverages")
    covs = None
    if args.coverages:
        try:
            covs = check_coverages([int(v) for v in args.coverages.split(",")])
        except ValueError as e:
            parser.error(f"--coverages: {e}")
    names = None
    if args.class_names:
        with open(args.class_names) as fh:
            names = [line.strip() for line in fh if line.strip()]
        if args.confusion_out and len(names) < args.confusion_labels:
            parser.error(f"--class_names holds {len(names)} names for {args.confusion_labels} labels")
        if segments is not None and len(names) < segments[0]:
            parser.error(f"--class_names holds {len(names)} names for {segments[0]} segment labels")
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
                         **(dict(adjoint="exact") if args.sr_adjoint == "exact" else {}))
    path = HotPath(model, sr, mode=args.mode, th_factor=args.th_factor, batch_size=BATCH_SIZE)
    sr_iters = []
    copy_weights = []
    out = evaluate_labelmaps(path, paths, gts, class_ids, num_aug=args.num_aug, angle_max=args.angle_max,
                             shift_max=args.shift_max, img_size=IMG_SIZE, rank=rank, world=world, seed=SEED,
                             prune=not args.no_prune, save_dir=args.save_dir, band_widths=bands,
                             confusion_labels=args.confusion_labels if args.confusion_out else None,
                             **(dict(th_factors=factors) if factors is not None else {}),
                             **(dict(guide=guide) if guide is not None else {}),
                             **(dict(tv_guide=args.tv_guide_beta) if args.tv_guide_beta is not None else {}),
                             **(dict(df_weights=args.df_weights) if args.df_weights is not None else {}),
                             **(dict(crf=crf) if crf is not None else {}),
                             **(dict(coverages=covs, uncertainty_dir=args.uncertainty_dir) if covs is not None else {}),
                             **(dict(min_region=min_region) if min_region is not None else {}),
                             **(dict(segments=segments) if segments is not None else {}),
                             **(dict(sr_stop=sr_stop, sr_iters=sr_iters) if sr_stop is not None else {}),
                             **(dict(couple=True) if args.couple_classes else {}),
                             **(dict(sr_reweight=sr_reweight, copy_weights=copy_weights) if sr_reweight is not None else {}))
    rows, counts = out.rows, out.counts
    if args.sr_iters_out:             # every rank holds the solves of its own images
        stem, ext = os.path.splitext(args.sr_iters_out)
        iters_path = args.sr_iters_out if world == 1 else f"{stem}.rank{rank}{ext}"
        os.makedirs(os.path.dirname(os.path.abspath(iters_path)), exist_ok=True)
        write_sr_iters_csv(iters_path, sr_iters)
        print(f"Wrote {iters_path}")
    if args.copy_weights_out:         # every rank holds the solves of its own images
        from asr_amd.evaluation import write_copy_weights_csv
        stem, ext = os.path.splitext(args.copy_weights_out)
        cw_path = args.copy_weights_out if world == 1 else f"{stem}.rank{rank}{ext}"
        os.makedirs(os.path.dirname(os.path.abspath(cw_path)), exist_ok=True)
        write_copy_weights_csv(cw_path, copy_weights)
        print(f"Wrote {cw_path}")
    if rank == 0:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        write_labelmap_csv(args.out, counts, rows)
        for j, key in enumerate(LABELMAP_KEYS):
            print(f"{key}: dataset mIoU {dataset_miou(counts[j]):.4f}, mean of per-image Mean_IOU {float(rows[:, j].mean()):.4f}")
        print(f"Wrote {args.out}")
        if bands:
            trimap = args.trimap_out or os.path.splitext(os.path.abspath(args.out))[0] + "_trimap.csv"
            os.makedirs(os.path.dirname(os.path.abspath(trimap)), exist_ok=True)
            write_trimap_csv(trimap, bands, out.band_counts, out.band_rows, counts=counts)
            print(f"Wrote {trimap}")
        if args.confusion_out:
            metrics = os.path.splitext(os.path.abspath(args.confusion_out))[0] + "_metrics.csv"
            os.makedirs(os.path.dirname(os.path.abspath(args.confusion_out)), exist_ok=True)
            write_confusion_csv(args.confusion_out, out.confusion, names)
            write_confusion_metrics_csv(metrics, out.confusion, names)
            print(f"Wrote {args.confusion_out} and {metrics}")
        if factors is not None:
            curve = args.th_sweep_out or os.path.splitext(os.path.abspath(args.out))[0] + "_thresholds.csv"
            os.makedirs(os.path.dirname(os.path.abspath(curve)), exist_ok=True)
            write_labelmap_threshold_csv(curve, factors, out.sweep_counts, out.sweep_rows, counts, rows)
            for key, (f, miou) in best_threshold_factors(factors, out.sweep_counts).items():
                print(f"{key}: best th_factor {f!r} by dataset mIoU ({miou:.4f})")
            print(f"Wrote {curve}")
        if covs is not None:
            cov_csv = args.coverage_out or os.path.splitext(os.path.abspath(args.out))[0] + "_coverage.csv"
            os.makedirs(os.path.dirname(os.path.abspath(cov_csv)), exist_ok=True)
            write_coverage_csv(cov_csv, covs, out.cov_counts, out.cov_rows, counts=counts)
            lo, hi = covs.index(min(covs)), covs.index(max(covs))
            for j, key in enumerate(LABELMAP_KEYS):
                if out.cov_counts[j].any():
                    print(f"{key}: dataset mIoU {dataset_miou(out.cov_counts[j, lo]):.4f} on the {covs[lo]} % most certain pixels, "
                          f"{dataset_miou(out.cov_counts[j, hi]):.4f} at {covs[hi]} %")
            print(f"Wrote {cov_csv}")
        if min_region is not None:
            reg_csv = args.regions_out or os.path.splitext(os.path.abspath(args.out))[0] + "_regions.csv"
            os.makedirs(os.path.dirname(os.path.abspath(reg_csv)), exist_ok=True)
            write_regions_csv(reg_csv, out.regions, out.raw_counts, out.raw_rows, counts, rows)
            for j, key in enumerate(LABELMAP_KEYS):
                if out.raw_counts[j].any():
                    print(f"{key}: {int(out.regions[j, 1])} of {int(out.regions[j, 0])} regions below {min_region[0]} pixels, "
                          f"{int(out.regions[j, 3])} pixels changed, dataset mIoU {dataset_miou(out.raw_counts[j]):.4f} -> "
                          f"{dataset_miou(counts[j]):.4f}")
            print(f"Wrote {reg_csv}")
        if segments is not None:
            from asr_amd.utils import metrics_from_segments
            os.makedirs(os.path.dirname(os.path.abspath(args.segments_out)), exist_ok=True)
            write_segments_csv(args.segments_out, out.segments, out.raw_segments, names)
            for j, key in enumerate(LABELMAP_KEYS):
                for stage, seg in (("raw", out.raw_segments), ("final", out.segments)):
                    if seg is not None and seg[j, :, :3].any():
                        tp, fp, fn = (int(v) for v in seg[j, :, :3].sum(axis=0))
                        print(f"{key} ({stage}): {tp} segments matched, {fp} spurious, {fn} missed, mean PQ "
                              f"{metrics_from_segments(seg[j])['mean_PQ']:.4f}")
            print(f"Wrote {args.segments_out}")
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
