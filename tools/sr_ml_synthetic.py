#!/usr/bin/env python3
"""The multi-label coupling next to the independent class solves on a synthetic scene, through the device path: two classes
that share an edge, plus background, at 48^2, seen as 12 copies of 12^2.  Each copy is the scene's soft class maps through the
solver's own forward model (rotate, shift, downscale) plus N(0, 0.15) noise on every map, then the argmax over {background,
class 1, class 2}: the hard masks a network's argmax OPM would hand the solver.  Optimizer("primal_dual"), 40 iterations,
lambda = (1, lambda_tv, 0, 0), six seeds, lambda_tv in 0.05, 0.1, 0.2.

    python tools/sr_ml_synthetic.py

Prints, per lambda_tv, the mIoU over {background, class 1, class 2} (mean over the seeds) of four label maps --

  th 0.15 / th 0.5     the independent solves fused by the threshold rule (ops.fuse_labels) at th_factor 0.15 and 0.5
  indep. + simplex     the independent solves fused by the threshold-free rule (ops.fuse_labels_simplex)
  coupled + simplex    the coupled solve (couple=True) fused by the threshold-free rule

-- and what the independent solutions do that the coupled ones cannot: the largest sum over the classes and the smallest value."""
import os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from asr_amd import ops
from asr_amd.superresolution_scripts.optimizer import Optimizer
from asr_amd.superresolution_scripts.superresolution import Superresolution
from asr_amd.utils import mean_iou_from_counts
if not torch.cuda.is_available():
    sys.exit("sr_ml_synthetic.py: no GPU visible")
dev = torch.device("cuda")
H, h, N, ITERS, SIGMA = 48, 12, 12, 40, 0.15
SEEDS = range(6)
IDS = [1, 2]


def scene(rng):
    """Truth label map [H, H]: two rectangles that share a vertical edge, placed at random, background round them."""
    t = np.zeros((H, H), np.int32)
    y0, y1 = rng.integers(6, 14), rng.integers(34, 42)
    x0, xm, x1 = rng.integers(6, 12), rng.integers(20, 28), rng.integers(36, 42)
    t[y0:y1, x0:xm] = 1
    t[y0 + rng.integers(0, 6):y1 - rng.integers(0, 6), xm:x1] = 2
    return t


def copies_of(truth, rng, sr):
    """-> (hard masks [2, N, h, h] device, angles [N], shifts [N, 2])."""
    angles = rng.uniform(-0.15, 0.15, N).astype(np.float32); angles[0] = 0
    shifts = rng.uniform(-0.15 * H, 0.15 * H, (N, 2)).astype(np.float32); shifts[0] = 0
    a, s = np.repeat(angles[None], 2, axis=0), np.repeat(shifts[None], 2, axis=0)
    rot, tr = sr._transforms(a, s, dev)
    onehot = ops.to_device(np.stack([(truth == c).astype(np.float32) for c in IDS]))
    zero = torch.zeros((2, N, h, h), dtype=torch.float32, device=dev)
    soft = ops.sr_forward_residual(onehot, zero, rot, tr).cpu().numpy()             # D(T(R(x))) - 0: the soft class maps
    maps = np.concatenate([1.0 - soft.sum(0, keepdims=True), soft]).astype(np.float32)        # background first
    maps = maps + rng.normal(0, SIGMA, maps.shape).astype(np.float32)
    win = maps.argmax(0)
    return ops.to_device(np.stack([(win == k + 1).astype(np.float32) for k in range(2)])), angles, shifts


def miou(truth_dev, labels):
    return mean_iou_from_counts(ops.class_counts(truth_dev, labels)[0].cpu().numpy())


print(f"{H}^2 from {N} copies of {h}^2, noise {SIGMA}, primal-dual, {ITERS} iterations, lambda = (1, lambda_tv, 0, 0), seeds "
      f"{list(SEEDS)}: mean mIoU over background and the two classes")
print(f"  {'lambda_tv':>9s}  {'th 0.15':>8s}  {'th 0.5':>8s}  {'indep. + simplex':>16s}  {'coupled + simplex':>17s}    independent: max sum, min x")
for lam_tv in (0.05, 0.1, 0.2):
    rows, worst_sum, worst_min = [], 0.0, 0.0
    for seed in SEEDS:
        rng = np.random.default_rng(seed)
        truth = scene(rng)
        make = lambda: Superresolution(1.0, lam_tv, 0.0, 0.0, num_iter=ITERS, num_aug=N, optimizer=Optimizer("primal_dual"),
                                       feature_size=(h, h), output_size=(H, H))
        y, angles, shifts = copies_of(truth, rng, make())
        gt = ops.to_device(truth, torch.int32)
        indep, _ = make().augmented_superresolution_classes(y, angles, shifts, [0, 0])
        coupled, _ = make().augmented_superresolution_classes(y, angles, shifts, [0, 0], couple=True)
        rows.append([miou(gt, ops.fuse_labels(indep, IDS, th_factor=0.15)[0]), miou(gt, ops.fuse_labels(indep, IDS, th_factor=0.5)[0]),
                     miou(gt, ops.fuse_labels_simplex(indep, IDS)), miou(gt, ops.fuse_labels_simplex(coupled, IDS))])
        worst_sum = max(worst_sum, float(indep.sum(0).max()))
        worst_min = min(worst_min, float(indep.min()))
        assert float(coupled.min()) >= 0.0 and float(coupled.double().sum(0).max()) <= 1.0 + 2e-6
    m = np.mean(rows, axis=0)
    print(f"  {lam_tv:9.2f}  {m[0]:8.4f}  {m[1]:8.4f}  {m[2]:16.4f}  {m[3]:17.4f}    {worst_sum:.3f}, {worst_min:.3f}")
