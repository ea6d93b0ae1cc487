#!/usr/bin/env python3
"""Label maps against the class-set path, on the MI355X (DESIGN.md "Label maps").

    python tools/bench_labelmap.py --what kernel --impl fuse|threshold
    python tools/bench_labelmap.py --what e2e --impl labels|labels_noprune|classes [--root DIR] [--images 10]
    python tools/bench_labelmap.py --what sweep --impl sweep|fuse17|e2e [--images 10]

--what kernel: 20 calls on the same K = 4 planes of 512 x 512 floats (no max maps, th_factor 0.2): --impl threshold is
ops.threshold_classes (K int32 masks out), --impl fuse is ops.fuse_labels (one int32 label map out).  Both launch the min/max
kernel first.  Run each under rocprofv3 --kernel-trace --stats for the kernel times.
--what e2e: the configs[1] workload (512 x 512, N = 100, argmax, 50 AMSGrad iterations, forward batches of 16) with classes 3, 8
and 15 made to win by logit-bias shifts over a background that wins everywhere else, on --images synthetic images after two
warm-up images.  --impl labels: HotPath.run_image_labels(class_ids=1..20); labels_noprune: the same with prune=False; classes:
HotPath.run_image_classes fed only the three winning ids -- the cheapest way to the same masks without label maps, and it needs
the answer in advance.  Prints one JSON line with the ms per image and the number of classes each image's solver was given.
--what sweep (DESIGN.md "Threshold curve of the label maps"): the 17 factors 0.10 ... 0.90 on K = 4 planes of 512 x 512 with a
ground truth.  --impl sweep: 20 calls of ops.fuse_labels_sweep_counts (all its launches, the min/max among them); --impl fuse17:
20 times 17 calls of ops.fuse_labels with the truth, one per factor -- the way to the same counts without the sweep.  Run each
under rocprofv3 --kernel-trace --stats.  --impl e2e: the e2e workload through run_image_labels with and without th_factors,
alternated A B A B in one process (two blocks of --images images each), the ms per image of both and their difference.
--root: the tree whose asr_amd is imported (default: this one), so that an older checkout can be measured by the same code.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--what", choices=["kernel", "e2e", "sweep"], required=True)
ap.add_argument("--impl", choices=["fuse", "threshold", "labels", "labels_noprune", "classes", "sweep", "fuse17", "e2e"],
                required=True)
ap.add_argument("--images", type=int, default=10)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

import torch  # noqa: E402
from bench import synth_image  # noqa: E402
from asr_amd import distributed as D, ops, weights as W  # noqa: E402
from asr_amd.model import DeeplabModel  # noqa: E402
from asr_amd.pipeline import HotPath  # noqa: E402
from asr_amd.superresolution_scripts.optimizer import Optimizer  # noqa: E402
from asr_amd.superresolution_scripts.superresolution import Superresolution  # noqa: E402

WIN = [3, 8, 15]
ALL = list(range(1, 21))
N, ITERS, BATCH, WARM = 100, 50, 16, 2


def kernel():
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    ids = [3, 8, 12, 15]
    planes = torch.rand((4, 512, 512), generator=g, device=dev).contiguous()
    for _ in range(20):
        if args.impl == "threshold":
            ops.threshold_classes(planes, ids, th_factor=0.2)
        else:
            ops.fuse_labels(planes, ids, th_factor=0.2)
    torch.cuda.synchronize()
    moved = planes.numel() * 4 + (planes.numel() if args.impl == "threshold" else planes[0].numel()) * 4
    print(json.dumps({"what": "kernel", "impl": args.impl, "bytes_per_call_without_minmax": moved}))


def sweep_kernel():
    from asr_amd.sweep import TH_FACTORS
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    ids = [3, 8, 12, 15]
    planes = torch.rand((4, 512, 512), generator=g, device=dev).contiguous()
    truth = torch.tensor([0] + ids, dtype=torch.int32, device=dev)[torch.randint(0, 5, (512, 512), generator=g, device=dev)]
    truth = truth.contiguous()
    factors = [float(f) for f in TH_FACTORS]
    f_dev = ops.to_device(np.asarray(factors, dtype=np.float32), device=dev)
    for _ in range(20):
        if args.impl == "sweep":
            ops.fuse_labels_sweep_counts(planes, ids, truth, f_dev)
        else:
            for f in factors:
                ops.fuse_labels(planes, ids, th_factor=f, truth=truth)
    torch.cuda.synchronize()
    # what one call of the head must move: the planes and the truth in, the [T, 3, 256] counts out (min/max pass not counted)
    moved = planes.numel() * 4 + truth.numel() * 4 + len(factors) * 768 * 8
    print(json.dumps({"what": "sweep", "impl": args.impl, "factors": len(factors), "bytes_per_sweep_call_without_minmax": moved}))


def e2e_setup():
    dev = torch.device("cuda", 0)
    model = DeeplabModel(W.make_synthetic_weights(1234, 21), (512, 512, 3), 21, False, None,
                         precision=os.environ.get("ASR_PRECISION", "f16x3"))          # bench.py's default
    imgs = [ops.to_device(synth_image(np.random.default_rng(1234 + j), 512), device=dev) for j in range(WARM + args.images)]
    # A VOC image is mostly background with 1-3 classes in it.  The seeded synthetic weights let a few classes share the
    # pixels instead, so the background logit is first raised until class 0 wins every pixel of every un-augmented image,
    # then classes 3, 8 and 15 are raised in turn until each wins a fifth of image 0.
    def margin(im, c):
        logits = model.predict_device(im[None].contiguous(), batch_size=1)[0]
        other = logits.clone()
        other[..., c] = float("-inf")
        return (other.max(dim=-1).values - logits[..., c]).flatten()

    model.engine.shift_logit_bias(0, max(float(margin(im, 0).max()) for im in imgs) + 1.0)
    for c in WIN:
        model.engine.shift_logit_bias(c, float(torch.quantile(margin(imgs[0], c), 0.2)))
    params = D.replay_augmentation_stream(len(imgs), N, 0.15, 80)
    opt = Optimizer("adam", 1e-3, amsgrad=True, lr_scheduler=True, decay_steps=60, decay_rate=0.3)
    sr = Superresolution(1.0, 0.3, 0.7, 0.0, num_iter=ITERS, num_aug=N, optimizer=opt, feature_size=(128, 128),
                         output_size=(512, 512))
    path = HotPath(model, sr, mode="argmax", th_factor=0.2, batch_size=BATCH)
    gts = []
    for im in imgs:                                 # the model's own standard masks as ground truth
        logits0 = model.predict_device(im[None].contiguous(), batch_size=1)[0].contiguous()
        gts.append(ops.standard_mask_classes(logits0, (512, 512), WIN).sum(dim=0).to(torch.int32).contiguous())
    return path, imgs, gts, params


def sweep_e2e():
    from asr_amd.sweep import TH_FACTORS
    path, imgs, gts, params = e2e_setup()
    factors = [float(f) for f in TH_FACTORS]

    def block(first, last, swept):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for g in range(first, last):
            angles, shifts = params[g]
            path.run_image_labels(imgs[g], angles, shifts, ALL, gt_dev=gts[g], adam_starts={c: g * ITERS for c in ALL},
                                  **(dict(th_factors=factors) if swept else {}))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / (last - first)

    for swept in (False, True):
        block(0, WARM, swept)
    ms = {False: [], True: []}
    for _ in range(2):                              # A B A B
        for swept in (False, True):
            ms[swept].append(block(WARM, len(imgs), swept))
    plain, swept = float(np.mean(ms[False])), float(np.mean(ms[True]))
    print(json.dumps({"what": "sweep", "impl": "e2e", "images": args.images, "factors": len(factors),
                      "plain_ms_per_image": [round(v, 3) for v in ms[False]], "swept_ms_per_image": [round(v, 3) for v in ms[True]],
                      "added_ms_per_image": round(swept - plain, 3), "ratio": round(swept / plain, 4)}))


def e2e():
    path, imgs, gts, params = e2e_setup()
    solved = []

    def one(g):
        angles, shifts = params[g]
        if args.impl == "classes":
            res = path.run_image_classes(imgs[g], angles, shifts, WIN, gt_dev=gts[g], adam_starts={c: g * ITERS for c in WIN})
            return float(np.nanmean([res[c]["ious"][2] for c in WIN]))
        res = path.run_image_labels(imgs[g], angles, shifts, ALL, gt_dev=gts[g], adam_starts={c: g * ITERS for c in ALL},
                                    prune=args.impl == "labels")
        solved.append(len(res["solved_ids"]))
        return res["Mean_IOU"]["aug"]

    for g in range(WARM):
        one(g)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    scores = [one(g) for g in range(WARM, len(imgs))]
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / args.images
    print(json.dumps({"what": "e2e", "impl": args.impl, "root": args.root, "images": args.images,
                      "ms_per_image": round(ms, 3), "classes_solved_per_image": solved[WARM:],
                      "score_mean": float(np.mean(scores))}))


if __name__ == "__main__":
    if args.what == "sweep":
        sweep_e2e() if args.impl == "e2e" else sweep_kernel()
    else:
        kernel() if args.what == "kernel" else e2e()
