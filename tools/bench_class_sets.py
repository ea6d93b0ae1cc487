#!/usr/bin/env python3
"""Class sets against per-class runs, on the MI355X (DESIGN.md "Class sets").

    python tools/bench_class_sets.py --impl single|classes [--root DIR] [--what e2e|opm] [--images 10]

--what e2e: the configs[1] workload (512 x 512, N = 100, argmax, 50 AMSGrad iterations, forward batches of 16) for K = 3
classes made to win by logit-bias shifts, on --images synthetic images after two warm-up images.  --impl single: one
HotPath.run_image per class (what a per-class table costs without class sets); --impl classes: HotPath.run_image_classes.
Prints one JSON line: ms per image, and the SR-stage time per image (profile["_sr_stage_ms"], from a second, profiled pass).
--what opm: the output-processing kernels alone, 20 calls each: argmax, slice and slice_max on one configs[1] forward batch of
logits [16, 128, 128, 21], and the standard mask of its first map [128, 128, 21] at 512 x 512 (single: class 8; classes: K = 4).
--impl single times the single-class entry points, which run the K = 1 case of the class-set kernels (opm_classes_kernel,
standard_mask_classes_kernel); with --root on a checkout up to 7c09926 it times the kernels they had of their own.
Run it under rocprofv3 --kernel-trace --stats for kernel times.
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
ap.add_argument("--impl", choices=["single", "classes"], required=True)
ap.add_argument("--what", choices=["e2e", "opm"], default="e2e")
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

IDS = [3, 8, 15]
N, ITERS, BATCH, WARM = 100, 50, 16, 2


def opm():
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    logits = (torch.randn((16, 128, 128, 21), generator=g, device=dev) * 3.0).contiguous()
    single = {"argmax": ops.opm_argmax, "slice": ops.opm_slice, "slice_max": ops.opm_slice_max}
    for mode in ("argmax", "slice", "slice_max"):
        for _ in range(20):
            if args.impl == "single":
                single[mode](logits, 8)
            else:
                ops.opm_classes(logits, [3, 8, 12, 15], mode)
        torch.cuda.synchronize()
    logits0 = logits[0].contiguous()
    for _ in range(20):
        if args.impl == "single":
            ops.standard_mask(logits0, (512, 512), 8)
        else:
            ops.standard_mask_classes(logits0, (512, 512), [3, 8, 12, 15])
    torch.cuda.synchronize()
    print(json.dumps({"what": "opm", "impl": args.impl, "root": args.root}))


def e2e():
    dev = torch.device("cuda", 0)
    model = DeeplabModel(W.make_synthetic_weights(1234, 21), (512, 512, 3), 21, False, None,
                         precision=os.environ.get("ASR_PRECISION", "f16x3"))          # bench.py's default
    imgs = [ops.to_device(synth_image(np.random.default_rng(1234 + j), 512), device=dev) for j in range(WARM + args.images)]
    for c in IDS:                                   # bench.calibrate_class_bias, one class after the other
        logits = model.predict_device(imgs[0][None].contiguous(), batch_size=1)[0]
        other = logits.clone()
        other[..., c] = float("-inf")
        model.engine.shift_logit_bias(c, float(torch.quantile((other.max(dim=-1).values - logits[..., c]).flatten(), 0.2)))
    params = D.replay_augmentation_stream(len(imgs), N, 0.15, 80)
    opt = Optimizer("adam", 1e-3, amsgrad=True, lr_scheduler=True, decay_steps=60, decay_rate=0.3)
    sr = Superresolution(1.0, 0.3, 0.7, 0.0, num_iter=ITERS, num_aug=N, optimizer=opt, feature_size=(128, 128),
                         output_size=(512, 512))
    paths = {c: HotPath(model, sr, class_id=c, mode="argmax", th_factor=0.2, batch_size=BATCH) for c in IDS}
    gts = []
    for im in imgs:                                 # the model's own standard masks as ground truth
        logits0 = model.predict_device(im[None].contiguous(), batch_size=1)[0].contiguous()
        gt = torch.zeros((512, 512), dtype=torch.int32, device=dev)
        for c in IDS:
            gt += ops.standard_mask(logits0, (512, 512), c)
        gts.append(gt)

    def one(g, profile=None):
        angles, shifts = params[g]
        if args.impl == "single":
            return [paths[c].run_image(imgs[g], angles, shifts, gt_dev=gts[g], adam_start=g * ITERS, profile=profile)["ious"]
                    for c in IDS]
        res = paths[IDS[0]].run_image_classes(imgs[g], angles, shifts, IDS, gt_dev=gts[g], profile=profile,
                                              adam_starts={c: g * ITERS for c in IDS})
        return [res[c]["ious"] for c in IDS]

    for g in range(WARM):
        one(g)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    recs = [one(g) for g in range(WARM, len(imgs))]
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / args.images
    prof = {}
    for g in range(WARM, len(imgs)):
        one(g, profile=prof)
    print(json.dumps({"what": "e2e", "impl": args.impl, "root": args.root, "images": args.images, "K": len(IDS),
                      "ms_per_image": round(ms, 3), "sr_stage_ms_per_image": round(prof["_sr_stage_ms"] / args.images, 3),
                      "aug_iou_single_mean": float(np.nanmean([r[2] for rec in recs for r in rec]))}))


if __name__ == "__main__":
    opm() if args.what == "opm" else e2e()
