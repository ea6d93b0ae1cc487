#!/usr/bin/env python3
"""The exact adjoint next to the registered gradient on the two synthetic settings of tools/sr_pd_synthetic.py (tests/sr_dt_ref.py's
make_case with no replaced copies: a rotated rectangle seen through the forward model, angles within 0.3 rad, binarised), through the
device path: Superresolution(adjoint="registered" / "exact") with AMSGrad under its schedule and with Optimizer("primal_dual") at 20
and 60 iterations, seeds 0 and 1 --

  64^2 from 20 copies of 16^2, lambda = (1, 0.05, 0, 0): AMSGrad lr 1e-2, 150 iterations
  128^2 from 30 copies of 32^2, lambda = (1, 0.3, 0.7, 0): AMSGrad lr 1e-3, decay 0.3 per 60, 300 iterations

    python tools/sr_adj_synthetic.py

Prints, per setting, solver and adjoint, the scalar loss of the result (Superresolution.loss_function) and the IoU of
x > 0.5 * max(x) against the truth, for both seeds; and the step bound each adjoint gives the primal-dual solves."""
import os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from asr_amd import ops
from asr_amd.superresolution_scripts.optimizer import Optimizer
from asr_amd.superresolution_scripts.superresolution import Superresolution
import sr_dt_ref as R
if not torch.cuda.is_available():
    sys.exit("sr_adj_synthetic.py: no GPU visible")
SEEDS = (0, 1)
PD_ITERS = (20, 60)
SETTINGS = [
    ("64^2 from 20 copies of 16^2, lambda = (1, 0.05, 0, 0)", dict(H=64, h=16, n=20), (1.0, 0.05, 0.0, 0.0),
     ("AMSGrad, lr 1e-2, 150 it.", dict(learning_rate=1e-2, amsgrad=True), 150)),
    ("128^2 from 30 copies of 32^2, lambda = (1, 0.3, 0.7, 0)", dict(H=128, h=32, n=30), (1.0, 0.3, 0.7, 0.0),
     ("AMSGrad, lr 1e-3, decay 0.3 per 60, 300 it.", dict(learning_rate=1e-3, amsgrad=True, lr_scheduler=True, decay_steps=60,
                                                         decay_rate=0.3), 300)),
]
dev = torch.device("cuda")
for title, shape, lam, (adam_name, adam_kw, adam_iters) in SETTINGS:
    cases = [R.make_case(s, n_bad=0, **shape) for s in SEEDS]
    H, h, n = shape["H"], shape["h"], shape["n"]
    rows = [(adam_name, lambda: Optimizer("adam", **adam_kw), adam_iters)] + \
           [(f"primal-dual, {k} it.", lambda: Optimizer("primal_dual"), k) for k in PD_ITERS]
    print(title)
    for name, make_opt, iters in rows:
        for adjoint in ("registered", "exact"):
            losses, ious = [], []
            for c in cases:                                         # a fresh optimiser (step counter 0) for every solve
                sr = Superresolution(*lam, num_iter=iters, num_aug=n, optimizer=make_opt(), feature_size=(h, h), output_size=(H, H),
                                     adjoint=adjoint)
                x, _ = sr.augmented_superresolution(c["copies"][..., None], c["angles"], c["shifts"])
                losses.append(sr.loss_function(x, c["copies"][..., None], c["angles"], c["shifts"]))
                ious.append(R.iou(x, c["truth"]))
            print(f"  {name:44s} {adjoint:10s} loss " + " / ".join(f"{v:.2f}" for v in losses) + "   IoU " +
                  " / ".join(f"{v:.3f}" for v in ious))
    sr = Superresolution(*lam, num_iter=1, num_aug=n, optimizer=Optimizer("primal_dual"), feature_size=(h, h), output_size=(H, H))
    for s, c in zip(SEEDS, cases):
        a, sh = c["angles"][None], c["shifts"][None]
        tfs = (*sr._transforms(a, sh, dev), *sr._transforms(a, sh, dev, inverse=True))
        bounds = [float(ops.sr_data_bound(*tfs, (H, H), (h, h), lam[0], adjoint=adj)[0]) for adj in ("registered", "exact")]
        print(f"  seed {s}: bound registered {bounds[0]:.4f}, exact {bounds[1]:.4f}")
