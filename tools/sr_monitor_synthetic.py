#!/usr/bin/env python3
"""Where the stop rule stops on the synthetic construction, and what the stop costs: the rotated rectangle of
tests/sr_dt_ref.py (make_case with no replaced copies: 64^2 from 20 binarised copies of 16^2), AMSGrad, lr 1e-2,
lambda = (1, 0.05, 0, 0), 200 iterations, seeds 0..7 solved as ONE batch of 8 under the monitor, once per tolerance.

    python tools/sr_monitor_synthetic.py

Prints, for rel_tol 1e-3 and 1e-4 (patience 3, every 1), the iteration at which each seed stops and the IoU of
x > 0.5 * max(x) against the truth at the stop, next to the IoU after all 200 iterations."""
import os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from asr_amd import _lib, ops, transforms as T
import sr_dt_ref as R
if not torch.cuda.is_available():
    sys.exit("sr_monitor_synthetic.py: no GPU visible")
ITERS, SEEDS = 200, range(8)
b1, b2, eps = np.float32(0.9), np.float32(0.999), np.float32(1e-7)
cases = [R.make_case(s, n_bad=0) for s in SEEDS]
H, h, n = R.H_HR, R.H_LR, R.N_COPIES
y = ops.to_device(np.stack([c["copies"] for c in cases]))
tfs = []
for inverse in (False, True):
    rot = np.stack([T.rotation_transforms(c["angles"], H, H) for c in cases])
    tr = np.stack([T.translation_transforms(c["shifts"]) for c in cases])
    if inverse:
        rot, tr = np.stack([T.inverse_transforms(r) for r in rot]), np.stack([T.inverse_transforms(t) for t in tr])
    tfs += [ops.to_device(rot), ops.to_device(tr)]
col = np.array([T.adam_alpha(np.float32(R.LR), b1, b2, it + 1) for it in range(ITERS)], np.float32)
alphas = ops.to_device(np.repeat(col[:, None], len(cases), axis=1))
cfg = ops.sr_config(_lib.OPT_ADAM, True, np.float32(1) - b1, np.float32(1) - b2, eps)


def solve(monitor):
    x = ops.sr_init_target(y, (H, H))
    out = ops.sr_solve(x, y, *tfs, alphas, R.LAMBDAS, cfg=cfg, monitor=monitor)
    return out[0].cpu().numpy(), (out[2] if monitor is not None else None)


full, _ = solve(None)
iou_full = [R.iou(full[i], c["truth"]) for i, c in enumerate(cases)]
print(f"rotated rectangle, {H}^2 from {n} binarised copies of {h}^2, AMSGrad lr {R.LR}, lambda {R.LAMBDAS}, {ITERS} iterations")
print("seed                  " + "  ".join(f"{s:5d}" for s in SEEDS))
print("IoU after all 200     " + "  ".join(f"{v:.3f}" for v in iou_full))
for tol in (1e-3, 1e-4):
    x, trace = solve(dict(every=1, rel_tol=tol, patience=3, min_iter=0, history=False))
    done = trace.iters_done.cpu().numpy()
    ious = [R.iou(x[i], c["truth"]) for i, c in enumerate(cases)]
    print(f"rel_tol {tol:g}: stops at " + "  ".join(f"{k:5d}" for k in done))
    print(f"rel_tol {tol:g}: IoU there " + "  ".join(f"{v:.3f}" for v in ious))
