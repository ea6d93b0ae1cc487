"""HotPath.run_image_classes: one forward pass for every class of an image, each class's result equal bit for bit to
HotPath(model, sr, class_id=c, ...).run_image(..., adam_start=adam_starts[c]) -- masks, and IoUs including NaN positions --
across OPM modes, priors, optimisers, copy_dropout and per-class Adam starts; and the copies go through the model once."""
import math

import numpy as np
import pytest
import torch

from bench import synth_image

pytestmark = pytest.mark.gpu

IDS = [3, 8, 15]
KEYS = ("standard", "aug", "max", "mean")


def _shift_classes(model, image_dev, ids, fraction=0.25):
    """engine.shift_logit_bias for each class in turn, as bench.calibrate_class_bias does for one: class c then wins on about
    `fraction` of the un-augmented image's pixels (seeded synthetic weights never make it win by themselves)."""
    for c in ids:
        logits = model.predict_device(image_dev[None].contiguous(), batch_size=1)[0]
        other = logits.clone()
        other[..., c] = float("-inf")
        margin = (other.max(dim=-1).values - logits[..., c]).flatten()
        model.engine.shift_logit_bias(c, float(torch.quantile(margin, fraction)))


def _ground_truth(model, image_dev, ids, out_hw):
    """A label map consistent with the model: its standard-output argmax over the set (other classes -> 0), with a void
    (255) band across the middle."""
    from asr_amd import ops
    logits0 = model.predict_device(image_dev[None].contiguous(), batch_size=1)[0].contiguous()
    masks = ops.standard_mask_classes(logits0, out_hw, ids)
    gt = masks.sum(dim=0).to(torch.int32)                 # argmax masks of distinct classes are disjoint
    mid = out_hw[0] // 2
    gt[mid:mid + 2] = 255
    return gt.contiguous()


def _sr(kind, n, iters, feat, out, use_btv, dropout):
    from asr_amd.superresolution_scripts.optimizer import Optimizer
    from asr_amd.superresolution_scripts.superresolution import Superresolution
    if kind == "adam":
        opt = Optimizer("adam", 1e-3, amsgrad=True, lr_scheduler=True, decay_steps=60, decay_rate=0.3)
    else:
        opt = Optimizer("sgd", 2e-3, momentum=0.9)
    return Superresolution(1.0, 0.3, 0.7, 0.0, num_iter=iters, num_aug=n, optimizer=opt, feature_size=feat, output_size=out,
                           use_BTV=use_btv, copy_dropout=dropout)


def _count_forward(model):
    calls = []
    orig = model.predict_device

    def wrapped(*a, **kw):
        calls.append(a[0].shape[0])
        return orig(*a, **kw)

    model.predict_device = wrapped
    return calls, orig


def _compare(got, ref, c):
    for k in KEYS:
        assert torch.equal(got[k], ref[k]), (c, k)
    a, b = got["ious"], ref["ious"]
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)]), (c, a, b)


def _run_case(model, img, gt, mode, kind, use_btv, dropout, n, iters, bs, feat, out, th_factor=0.2):
    from asr_amd.pipeline import HotPath
    from asr_amd.superresolution_scripts.augmentation_utils import draw_augmentation_parameters
    np.random.seed(17)
    angles, shifts = draw_augmentation_parameters(n, 0.15, out[0] / 8)
    sr = _sr(kind, n, iters, feat, out, use_btv, dropout)            # ONE object: its frozen copy_dropout mask serves all
    starts = {3: 0, 8: 3 * iters, 15: 7 * iters + 2}                  # different per class
    sr.optimizer.optimizer.iterations = 123
    path = HotPath(model, sr, mode=mode, th_factor=th_factor, batch_size=bs)
    calls, orig = _count_forward(model)
    try:
        got = path.run_image_classes(img, angles, shifts, IDS, gt_dev=gt, adam_starts=starts)
    finally:
        model.predict_device = orig
    assert len(calls) == math.ceil(n / bs) and sum(calls) == n, calls           # one pass of the copies, not K
    assert sr.optimizer.optimizer.iterations == 123                             # explicit starts leave the counter alone
    assert sorted(got) == sorted(IDS)
    for c in IDS:
        ref = HotPath(model, sr, class_id=c, mode=mode, th_factor=th_factor, batch_size=bs).run_image(
            img, angles, shifts, gt_dev=gt, adam_start=starts[c])
        _compare(got[c], ref, c)
    return got


CASES = [
    ("argmax", "adam", False, 0.0),
    ("argmax", "sgd", True, 0.5),
    ("slice", "sgd", True, 0.0),
    ("slice", "adam", False, 0.5),
    ("slice_max", "adam", True, 0.0),
    ("slice_max", "sgd", False, 0.5),
]


@pytest.fixture(scope="module")
def small(dev):
    from asr_amd import ops, weights as W
    from asr_amd.model import DeeplabModel
    model = DeeplabModel(W.make_synthetic_weights(1234, 21), (64, 64, 3), 21, False, None)      # Xception, OS 16
    img = ops.to_device(synth_image(np.random.default_rng(21), 64), device=dev)
    _shift_classes(model, img, IDS)
    gt = _ground_truth(model, img, IDS, (64, 64))
    return model, img, gt


@pytest.mark.parametrize("mode,kind,use_btv,dropout", CASES)
def test_class_set_equals_single_class_runs(small, mode, kind, use_btv, dropout):
    model, img, gt = small
    got = _run_case(model, img, gt, mode, kind, use_btv, dropout, n=6, iters=5, bs=4, feat=(16, 16), out=(64, 64))
    if mode == "argmax":                     # non-vacuity: classes that the masks and the truth both hold
        live = [c for c in IDS if bool((got[c]["aug"] == c).any()) and bool((gt == c).any())]
        assert len(live) >= 2, live


def test_class_set_without_starts_counts_as_consecutive_runs(small):
    """adam_starts=None: the classes are solved as consecutive run_image calls in class order from the current counter,
    which then stands where those calls would leave it."""
    from asr_amd.pipeline import HotPath
    from asr_amd.superresolution_scripts.augmentation_utils import draw_augmentation_parameters
    model, img, gt = small
    np.random.seed(3)
    angles, shifts = draw_augmentation_parameters(6, 0.15, 8)
    sr_a = _sr("adam", 6, 5, (16, 16), (64, 64), False, 0.0)
    sr_b = _sr("adam", 6, 5, (16, 16), (64, 64), False, 0.0)
    sr_a.optimizer.optimizer.iterations = sr_b.optimizer.optimizer.iterations = 40
    got = HotPath(model, sr_a, mode="slice_max", batch_size=6).run_image_classes(img, angles, shifts, IDS, gt_dev=gt)
    for c in IDS:
        ref = HotPath(model, sr_b, class_id=c, mode="slice_max", batch_size=6).run_image(img, angles, shifts, gt_dev=gt)
        _compare(got[c], ref, c)
    assert sr_a.optimizer.optimizer.iterations == sr_b.optimizer.optimizer.iterations == 40 + 3 * 2 * 5


def test_class_set_configs1_size(dev):
    """configs[1]-sized: 512 x 512, N = 100, K = 3, argmax, 50 AMSGrad iterations, forward batches of 16."""
    from asr_amd import ops, weights as W
    from asr_amd.model import DeeplabModel
    model = DeeplabModel(W.make_synthetic_weights(1234, 21), (512, 512, 3), 21, False, None)
    img = ops.to_device(synth_image(np.random.default_rng(1234), 512), device=dev)
    _shift_classes(model, img, IDS)
    gt = _ground_truth(model, img, IDS, (512, 512))
    got = _run_case(model, img, gt, "argmax", "adam", False, 0.0, n=100, iters=50, bs=16, feat=(128, 128), out=(512, 512))
    live = [c for c in IDS if bool((got[c]["aug"] == c).any()) and bool((gt == c).any())]
    assert len(live) >= 2, live
