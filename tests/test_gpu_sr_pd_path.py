"""GPU: the primal-dual rule through the upper layers -- Superresolution(optimizer=Optimizer("primal_dual")), the class-batched
solve, HotPath.run_image_labels on the small model of the label-map path tests -- and the Adam path, built through the new
constructor, against the committed golden trace."""
import json
import sys

import numpy as np
import pytest
import torch

import sr_dt_ref as RD
from test_gpu_sr_wtv import _upper

pytestmark = pytest.mark.gpu

LAM = RD.LAMBDAS                                        # (1, 0.05, 0, 0): the synthetic setting of tests/sr_dt_ref.py


def _sr(kind, n, iters, feat, out, lam=LAM, **kw):
    from asr_amd.superresolution_scripts.optimizer import Optimizer
    from asr_amd.superresolution_scripts.superresolution import Superresolution
    opt = Optimizer("primal_dual") if kind == "primal_dual" else Optimizer("adam", RD.LR, amsgrad=True)
    return Superresolution(*lam, num_iter=iters, num_aug=n, optimizer=opt, feature_size=feat, output_size=out, **kw)


@pytest.mark.parametrize("seed", [0, 1])
def test_sixty_iterations_end_below_amsgrads_hundred_and_fifty_on_the_device(dev, seed):
    """tests/test_sr_pd_host.py's inequality, both solves on the device.  Measured on the CPU restatement: 24.14 < 24.89
    (seed 0), 22.49 < 23.23 (seed 1); on an MI355X: 24.1373 < 24.8885 and 22.4856 < 23.2343."""
    from asr_amd import ops
    case = RD.make_case(seed, n_bad=0)
    n, h, H = len(case["copies"]), case["copies"].shape[-1], case["truth"].shape[-1]
    copies = case["copies"][..., None]
    adam = _sr("adam", n, RD.ITERS, (h, h), (H, H))
    x_adam, _ = adam.augmented_superresolution(copies, case["angles"], case["shifts"])
    pd = _sr("primal_dual", n, 60, (h, h), (H, H))
    x_pd, last = pd.augmented_superresolution(copies, case["angles"], case["shifts"])
    assert pd.optimizer.optimizer.iterations == 60                      # the counter advances like every other rule's
    loss_adam = adam.loss_function(x_adam, copies, case["angles"], case["shifts"])
    loss_pd = pd.loss_function(x_pd, copies, case["angles"], case["shifts"])
    print(f"seed {seed}: AMSGrad 150 it. loss {loss_adam:.4f} IoU {RD.iou(x_adam, case['truth']):.3f}; primal-dual 60 it. loss "
          f"{loss_pd:.4f} IoU {RD.iou(x_pd, case['truth']):.3f}; loss of the last iteration's x {last:.4f}")
    assert np.isfinite(x_pd).all() and np.isfinite(loss_pd)
    assert loss_pd < loss_adam
    # the same solve from its parts, with nothing read back between the bound and the result
    yd = ops.to_device(case["copies"][None])
    a, s = case["angles"][None], case["shifts"][None]
    rot, tr = pd._transforms(a, s, dev)
    irot, itr = pd._transforms(a, s, dev, inverse=True)
    x0 = ops.sr_init_target(yd, (H, H))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        bound = ops.sr_data_bound(rot, tr, irot, itr, (H, H), (h, h), LAM[0])
        steps = ops.pd_steps(bound, LAM[2], 60)
        x, _ = ops.sr_solve(x0, yd, rot, tr, irot, itr, steps, LAM, cfg=pd.optimizer.optimizer.config(), want_loss=False)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert np.array_equal(x[0].cpu().numpy(), x_pd[..., 0])
    print(f"seed {seed}: bound {float(bound[0]):.5f} tau {float(steps[0, 0]):.5f}")


def test_each_class_of_a_class_batch_is_its_own_single_solve(dev):
    from asr_amd import ops
    rng = np.random.default_rng(5)
    cases = [RD.make_case(s, H=32, h=8, n=6, n_bad=0) for s in (2, 3)]
    angles, shifts = cases[0]["angles"], cases[0]["shifts"]
    copies = ops.to_device(np.stack([c["copies"] for c in cases]) + 0.1 * rng.random((2, 6, 8, 8), dtype=np.float32))
    lam = (1.0, 0.3, 0.7, 0.0)
    both, _ = _sr("primal_dual", 6, 8, (8, 8), (32, 32), lam).augmented_superresolution_classes(copies, angles, shifts, [0, 11])
    assert both.shape == (2, 32, 32) and bool(torch.isfinite(both).all())
    for k in range(2):
        one, _ = _sr("primal_dual", 6, 8, (8, 8), (32, 32), lam).augmented_superresolution_batch(copies[k:k + 1].contiguous(),
                                                                                               angles[None], shifts[None])
        assert torch.equal(one[0], both[k]), k
    assert not torch.equal(both[0], both[1])


def test_run_image_labels_runs_with_the_rule(dev):
    from asr_amd.pipeline import HotPath
    L, small_inputs = _upper()
    model, img, gt, angles, shifts = small_inputs(dev)
    sr = _sr("primal_dual", 6, 5, (16, 16), (64, 64), (1.0, 0.3, 0.7, 0.0))
    res = HotPath(model, sr, mode="argmax", th_factor=L.TH, batch_size=4).run_image_labels(img, angles, shifts, L.REQ, gt_dev=gt,
                                                                                            keep_scores=True)
    scores = [t for t in res["scores"]["aug"] if t is not None]
    assert scores and all(bool(torch.isfinite(t).all()) for t in scores)
    assert res["aug"].dtype == torch.int32 and tuple(res["aug"].shape[-2:]) == (64, 64)
    # and the monitored form: the solves stop by themselves, the duals frozen with x
    res = HotPath(model, sr, mode="argmax", th_factor=L.TH, batch_size=4).run_image_labels(
        img, angles, shifts, L.REQ, gt_dev=gt, keep_scores=True, sr_stop=dict(rel_tol=1e-2, patience=1))
    assert all(bool(torch.isfinite(t).all()) for t in res["scores"]["aug"] if t is not None)


def test_adam_built_through_the_new_constructor_is_the_golden_run(dev):
    """Optimizer.from_flags without --sr_optimizer builds the scripts' AMSGrad schedule; run_image_labels with it returns the
    bytes of tests/golden/hotpath_traces.json, recorded before the rule existed (tests/test_gpu_hotpath_traces.py replays
    every case with the old constructor)."""
    from conftest import GOLDEN
    if GOLDEN not in sys.path:
        sys.path.insert(0, GOLDEN)
    import make_hotpath_traces as traces
    from asr_amd.pipeline import HotPath
    from asr_amd.superresolution_scripts.optimizer import Optimizer
    from asr_amd.superresolution_scripts.superresolution import Superresolution
    with open(traces.OUT) as f:
        golden = json.load(f)
    hyper = dict(optimizer="adam", learning_rate=1e-3, amsgrad=True, lr_scheduler=True, decay_steps=60, decay_rate=0.3)
    fix = traces.fixture(dev)
    model, img, gt, angles, shifts, _ = fix
    warm = HotPath(model, traces.make_sr(), class_id=8, mode="argmax", th_factor=traces.TH, batch_size=traces.BATCH)
    warm.run_image(img, angles, shifts, gt_dev=gt)
    torch.cuda.synchronize()
    name = "run_image_labels prune=1 bands=0"
    sr = Superresolution(1.0, 0.3, 0.7, 0.0, num_iter=traces.ITERS, num_aug=traces.N_AUG, optimizer=Optimizer.from_flags(hyper),
                         feature_size=(16, 16), output_size=(64, 64))
    sr.optimizer.optimizer.iterations = traces.ADAM0
    with traces.recorded_calls() as names:
        res = traces.cases(fix)[name](sr)
        torch.cuda.synchronize()
    assert list(names) == golden[name]["calls"]
    assert traces.digest(res) == golden[name]["out"]
    assert int(sr.optimizer.optimizer.iterations) == golden[name]["adam_after"]
