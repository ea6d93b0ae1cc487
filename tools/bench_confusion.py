#!/usr/bin/env python3
"""Confusion matrices of label maps against the counts the project already had, on the MI355X (DESIGN.md "Confusion matrix").

    python tools/bench_confusion.py --what kernel --impl confusion|class_counts
    python tools/bench_confusion.py --what e2e --impl confusion|plain [--root DIR] [--images 10]

--what kernel: 20 calls on the same four 512 x 512 label maps and one ground truth.  --impl confusion is one
ops.confusion_counts over the four maps with 21 labels (one launch and one memset); --impl class_counts is four ops.class_counts,
one per map: how the same four maps were scored before.  Run each under rocprofv3 --kernel-trace --stats, in a run of its own,
for the kernel times.  The label maps are mostly background with three class regions and a void ring, the predictions the truth
with shifted regions, so that the histogram adds meet what they meet on real maps.
--what e2e: the label-map workload of tools/bench_labelmap.py (512 x 512, N = 100, argmax, 50 AMSGrad iterations, forward batches
of 16, classes 3, 8 and 15 made to win) through HotPath.run_image_labels(class_ids=1..20, band_widths=None) on --images synthetic
images after two warm-up images.  --impl confusion: with confusion_labels=21; --impl plain: without.  Prints one JSON line with
the ms per image.  --root: the tree whose asr_amd is imported (default: this one), so that the parent commit's checkout can be
measured by the same code (--impl plain); alternate the two in one session.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--what", choices=["kernel", "e2e"], required=True)
ap.add_argument("--impl", choices=["confusion", "class_counts", "plain"], required=True)
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
LABELS = 21


def label_maps():
    """One 512 x 512 ground truth (three boxes with a void ring on background) and four predictions (the boxes shifted)."""
    def boxes(dy, dx, void):
        m = np.zeros((512, 512), np.int32)
        for c, (y0, y1, x0, x1) in {3: (40, 200, 60, 260), 8: (230, 470, 100, 300), 15: (120, 380, 330, 480)}.items():
            if void:
                m[y0 - 3 + dy:y1 + 3 + dy, x0 - 3 + dx:x1 + 3 + dx] = 255
            m[y0 + dy:y1 + dy, x0 + dx:x1 + dx] = c
        return m
    truth = boxes(0, 0, True)
    preds = np.stack([boxes(dy, dx, False) for dy, dx in ((0, 0), (4, -3), (-6, 5), (9, 9))])
    return truth, preds


def kernel():
    if args.impl == "plain":
        ap.error("--what kernel takes --impl confusion or class_counts")
    dev = torch.device("cuda", 0)
    truth, preds = label_maps()
    t = torch.from_numpy(truth).to(dev).reshape(-1).contiguous()
    q = torch.from_numpy(preds).to(dev).reshape(4, -1).contiguous()
    for _ in range(20):
        if args.impl == "confusion":
            ops.confusion_counts(t, q, LABELS)
        else:
            for p in range(4):
                ops.class_counts(t, q[p])
    torch.cuda.synchronize()
    print(json.dumps({"what": "kernel", "impl": args.impl, "bytes_per_call": 4 * (4 + 4) * t.numel()}))


def e2e():
    if args.impl == "class_counts":
        ap.error("--what e2e takes --impl confusion or plain")
    dev = torch.device("cuda", 0)
    model = DeeplabModel(W.make_synthetic_weights(1234, 21), (512, 512, 3), 21, False, None,
                         precision=os.environ.get("ASR_PRECISION", "f16x3"))          # bench.py's default
    imgs = [ops.to_device(synth_image(np.random.default_rng(1234 + j), 512), device=dev) for j in range(WARM + args.images)]

    # tools/bench_labelmap.py's workload: the background wins everywhere, then classes 3, 8 and 15 a fifth of image 0 each
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
    extra = {"confusion_labels": LABELS} if args.impl == "confusion" else {}

    def one(g):
        angles, shifts = params[g]
        res = path.run_image_labels(imgs[g], angles, shifts, ALL, gt_dev=gts[g], adam_starts={c: g * ITERS for c in ALL}, **extra)
        if extra:
            assert int(res["confusion"]["aug"].sum()) == 512 * 512
        return res["Mean_IOU"]["aug"]

    for g in range(WARM):
        one(g)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    scores = [one(g) for g in range(WARM, len(imgs))]
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / args.images
    print(json.dumps({"what": "e2e", "impl": args.impl, "root": args.root, "images": args.images,
                      "ms_per_image": round(ms, 3), "score_mean": float(np.mean(scores))}))


if __name__ == "__main__":
    kernel() if args.what == "kernel" else e2e()
