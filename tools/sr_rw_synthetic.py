#!/usr/bin/env python3
"""The synthetic construction of tests/sr_dt_ref.py (64^2 from 20 binarised copies of 16^2, 5 of them replaced by a disc) solved on
the device with and without copy reweighting: 150 AMSGrad iterations, lr 1e-2, lambda = (1, 0.05, 0, 0), seeds 0..7 in one batch.

    python tools/sr_rw_synthetic.py [--seeds 8] [--kappa 2] [--every 10] [--start 10]

Prints, per variant, the range over the seeds of the IoU of x > 0.5 max(x) against the truth, and for the reweighted ones the
largest final weight of a replaced copy and the smallest of a kept one; "clean" is the construction without replaced copies."""
import argparse, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from asr_amd import ops, transforms as T
import sr_dt_ref as R

ap = argparse.ArgumentParser()
ap.add_argument("--seeds", type=int, default=8)
ap.add_argument("--kappa", type=float, default=2.0)
ap.add_argument("--every", type=int, default=10)
ap.add_argument("--start", type=int, default=10)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("sr_rw_synthetic.py: no GPU visible -- the table comes from the device path")
b1, b2, eps = np.float32(0.9), np.float32(0.999), np.float32(1e-7)
H, h = R.H_HR, R.H_LR


def problem(cases):
    y = ops.to_device(np.stack([c["copies"] for c in cases]))
    angs, shs = np.stack([c["angles"] for c in cases]), np.stack([c["shifts"] for c in cases])
    b, n = angs.shape
    rot = T.rotation_transforms(angs.reshape(-1), H, H)
    tr = T.translation_transforms(shs.reshape(-1, 2))
    tfs = [ops.to_device(t.reshape(b, n, 8)) for t in (rot, tr, T.inverse_transforms(rot), T.inverse_transforms(tr))]
    alphas = np.zeros((R.ITERS, b), np.float32)
    for it in range(R.ITERS):
        alphas[it, :] = T.adam_alpha(np.float32(R.LR), b1, b2, it + 1)
    return y, tfs, ops.to_device(alphas)


def solve(cases, data_term, kind=None):
    y, tfs, alphas = problem(cases)
    kw = {} if kind is None else dict(reweight=dict(kind=kind, kappa=args.kappa, every=args.every, start=args.start))
    out = ops.sr_solve(ops.sr_init_target(y, (H, H)), y, *tfs, alphas, R.LAMBDAS, np.float32(1) - b1, np.float32(1) - b2, eps, True,
                       want_loss=False, data_term=data_term, **kw)
    ious = [R.iou(out[0][i].cpu().numpy(), cases[i]["truth"]) for i in range(len(cases))]
    return ious, (out[-1].weights.cpu().numpy() if kind is not None else None)


cases = [R.make_case(s) for s in range(args.seeds)]
clean = [R.make_case(s, n_bad=0) for s in range(args.seeds)]
rows = [("L2", "l2", None, cases), ("Huber 0.1", ("huber", 0.1), None, cases), ("L2 + cauchy", "l2", "cauchy", cases),
        ("L2 + hard", "l2", "hard", cases), ("Huber + cauchy", ("huber", 0.1), "cauchy", cases), ("clean L2", "l2", None, clean),
        ("clean L2 + cauchy", "l2", "cauchy", clean)]
print(f"{args.seeds} seeds, kappa {args.kappa}, every {args.every}, start {args.start}")
for name, dt, kind, cs in rows:
    ious, cw = solve(cs, dt, kind)
    line = f"{name:18s} IoU {min(ious):.3f} .. {max(ious):.3f}"
    if cw is not None and len(cs[0]["bad"]):
        bad = max(float(cw[i, c["bad"]].max()) for i, c in enumerate(cs))
        kept = min(float(np.delete(cw[i], c["bad"]).min()) for i, c in enumerate(cs))
        line += f"   replaced <= {bad:.4f}   kept >= {kept:.4f}"
    print(line + "   per seed " + " ".join(f"{v:.3f}" for v in ious))
