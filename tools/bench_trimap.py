#!/usr/bin/env python3
"""The trimap kernels and their cost in the label-map path, on the MI355X (DESIGN.md "Trimap").

    python tools/bench_trimap.py --what kernel --impl class_counts|band|dist|copy [--r_max 32] [--map synth|cat]
    python tools/bench_trimap.py --what e2e [--order none,bands,none,bands] [--images 10]

--what kernel: 20 calls; run each under rocprofv3 --kernel-trace --stats, a run of its own per kernel, for the kernel times.
  class_counts: ops.class_counts on one 512 x 512 truth and one prediction (the parent needs four such launches for the four
                label maps of an image);
  band:         ops.band_class_counts with P = 4 predictions and B = 6 widths (1, 2, 4, 8, 16, 32) on the same truth;
  dist:         ops.boundary_dist2 at --r_max on --map (synth: a 512 x 512 map of four ellipses with void rings; cat: the
                375 x 500 golden ground truth);
  copy:         the same bytes in and out as dist (int32 in, 16 bits out) as a plain element-wise conversion.
--what e2e: the configs[1] label-map workload of tools/bench_labelmap.py (512 x 512, N = 100, argmax, 20 requested classes,
  --images images after 2 warm-up images), once per entry of --order in ONE process: none = band_widths=None, bands =
  band_widths=(1, 2, 4, 8, 16, 32).  Prints one JSON line with the ms per image of every run.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--what", choices=["kernel", "e2e"], required=True)
ap.add_argument("--impl", choices=["class_counts", "band", "dist", "copy"], default="band")
ap.add_argument("--r_max", type=int, default=32)
ap.add_argument("--map", choices=["synth", "cat"], default="synth")
ap.add_argument("--order", default="none,bands,none,bands")
ap.add_argument("--images", type=int, default=10)
args = ap.parse_args()
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from bench import synth_image  # noqa: E402
from asr_amd import distributed as D, ops, weights as W  # noqa: E402
from asr_amd.model import DeeplabModel  # noqa: E402
from asr_amd.pipeline import HotPath  # noqa: E402
from asr_amd.superresolution_scripts.optimizer import Optimizer  # noqa: E402
from asr_amd.superresolution_scripts.superresolution import Superresolution  # noqa: E402

WIDTHS = (1, 2, 4, 8, 16, 32)
WIN = [3, 8, 15]
ALL = list(range(1, 21))
N, ITERS, BATCH, WARM = 100, 50, 16, 2


def blob_map(seed, h, w, labels=(3, 8, 15, 12), ring=2):
    """Background 0, one ellipse per label, each inside a ring of void (255)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    t = np.zeros((h, w), np.int32)
    for l in labels:
        cy, cx = rng.uniform(0.2, 0.8) * h, rng.uniform(0.2, 0.8) * w
        ry, rx = rng.uniform(0.08, 0.2) * h + ring + 1, rng.uniform(0.08, 0.2) * w + ring + 1
        t[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = 255
        t[((yy - cy) / (ry - ring)) ** 2 + ((xx - cx) / (rx - ring)) ** 2 <= 1.0] = l
    return t


def kernel():
    dev = torch.device("cuda", 0)
    if args.map == "cat":
        from PIL import Image
        host = np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "test_cat_gt.png"))).astype(np.int32)
    else:
        host = blob_map(11, 512, 512)
    truth = torch.from_numpy(host).to(dev)
    preds = torch.stack([torch.roll(truth, (3 * j + 1, -2 * j - 1), (0, 1)) for j in range(4)]).contiguous()
    d2 = ops.boundary_dist2(truth, 32)
    px = truth.numel()
    moved = {"class_counts": 8 * px, "band": (4 + 2 + 4) * px * 4, "dist": 6 * px, "copy": 6 * px}[args.impl]
    torch.cuda.synchronize()
    for _ in range(20):
        if args.impl == "class_counts":
            ops.class_counts(truth, preds[0])
        elif args.impl == "band":
            ops.band_class_counts(truth, preds, d2, WIDTHS, 32, 255)
        elif args.impl == "dist":
            ops.boundary_dist2(truth, args.r_max)
        else:
            truth.to(torch.int16)
    torch.cuda.synchronize()
    share = {w: round(float((d2.to(torch.int32) <= w * w).float().mean()), 4) for w in WIDTHS}
    print(json.dumps({"what": "kernel", "impl": args.impl, "map": args.map, "shape": list(host.shape), "r_max": args.r_max,
                      "bytes_per_call": moved, "band_share": share}))


def e2e():
    dev = torch.device("cuda", 0)
    model = DeeplabModel(W.make_synthetic_weights(1234, 21), (512, 512, 3), 21, False, None,
                         precision=os.environ.get("ASR_PRECISION", "f16x3"))
    imgs = [ops.to_device(synth_image(np.random.default_rng(1234 + j), 512), device=dev) for j in range(WARM + args.images)]

    def margin(im, c):                              # the workload of tools/bench_labelmap.py: background + 3 winning classes
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
    for im in imgs:
        logits0 = model.predict_device(im[None].contiguous(), batch_size=1)[0].contiguous()
        gts.append(ops.standard_mask_classes(logits0, (512, 512), WIN).sum(dim=0).to(torch.int32).contiguous())
    runs = []
    for impl in args.order.split(","):
        extra = dict(band_widths=WIDTHS) if impl == "bands" else {}

        def one(g):
            angles, shifts = params[g]
            return path.run_image_labels(imgs[g], angles, shifts, ALL, gt_dev=gts[g], adam_starts={c: g * ITERS for c in ALL},
                                         **extra)

        for g in range(WARM):
            one(g)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = [one(g) for g in range(WARM, len(imgs))]
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / args.images
        rec = {"impl": impl, "ms_per_image": round(ms, 3), "aug_mIoU": float(np.mean([r["Mean_IOU"]["aug"] for r in res]))}
        if impl == "bands":
            rec["aug_band_mIoU"] = np.mean([r["band_Mean_IOU"]["aug"] for r in res], axis=0).round(4).tolist()
            rec["standard_band_mIoU"] = np.mean([r["band_Mean_IOU"]["standard"] for r in res], axis=0).round(4).tolist()
        runs.append(rec)
    print(json.dumps({"what": "e2e", "images": args.images, "runs": runs}))


if __name__ == "__main__":
    kernel() if args.what == "kernel" else e2e()
