"""Class sets on the GPU: each *_classes entry point equals, bit for bit, K calls of its single-class counterpart (and the
OPM equals oracle.augment.opm per class).  The single-class OPM and standard-mask calls run the K = 1 case of the same
kernels, so for them this checks plane placement and that a class's result does not depend on the rest of the set; the
independent pin of the K = 1 bytes is tests/golden/reduce_single_class_digests.json (test_gpu_reduce_digests.py).  Logits are built so that every class of the set really decides pixels: it is the
argmax of at least 1 % of them and ties for the maximum on some, with +-0.0 entries and magnitudes up to 1e4, on pixel
counts that are not a multiple of 256."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import augment as o_aug

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))      # tests/base_kernel_cases.py, whatever pytest's import mode
from base_kernel_cases import first_argmax as _first_argmax, make_logits  # noqa: E402,F401  (make_logits: also imported from here)

pytestmark = pytest.mark.gpu

SHAPE = (3, 37, 41)          # copies, h, w: 1517 pixels per copy, 4551 in all (tails past every 256-pixel block)


def _sets(classes):
    rng = np.random.default_rng(classes)
    rest = [int(c) for c in rng.permutation(np.arange(1, classes))[:20]]
    return {1: [0], 3: [0, classes // 2 - 3, classes - 1], 21: [int(c) for c in rng.permutation([0] + rest)]}


def _bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("classes", [21, 40])           # LDS-staged rows / rows straight from global memory
@pytest.mark.parametrize("k", [1, 3, 21])
@pytest.mark.parametrize("mode", ["argmax", "slice", "slice_max"])
def test_opm_classes_equals_single_class_calls_bitwise(dev, classes, k, mode):
    from asr_amd import ops
    ids = _sets(classes)[k]
    x = make_logits(classes, ids, seed=100 * classes + k)
    xd = ops.to_device(x, device=dev)
    cls, mx = ops.opm_classes(xd, ids, mode)
    assert cls.shape == (k,) + SHAPE and ((mx is None) == (mode != "slice_max"))
    for j, c in enumerate(ids):
        if mode == "argmax":
            ref = ops.opm_argmax(xd, c)
            assert _same(cls[j], ref), (c, j)
            o_cm, _ = o_aug.opm(x, c, "argmax")
            assert np.array_equal(cls[j].cpu().numpy(), np.stack(o_cm)[..., 0]), c
            assert (cls[j] == c).float().mean().item() >= 0.01 or c == 0      # class 0's "mask" is all zeros by definition
        elif mode == "slice":
            ref = ops.opm_slice(xd, c)
            assert _same(cls[j], ref), (c, j)
            o_cm, _ = o_aug.opm(x, c, "slice")
            # values in [0, 1]: a few f32 ulps of 1.0 if numpy rounds differently anywhere
            np.testing.assert_allclose(cls[j].cpu().numpy(), np.stack(o_cm)[..., 0], rtol=0, atol=1e-6)
        else:
            rc, rm = ops.opm_slice_max(xd, c)
            assert _same(cls[j], rc) and _same(mx[j], rm), (c, j)
            o_cm, o_mm = o_aug.opm(x, c, "slice_max")
            assert np.array_equal(cls[j].cpu().numpy(), np.stack(o_cm)[..., 0]), c
            assert np.array_equal(mx[j].cpu().numpy(), np.stack(o_mm)[..., 0]), c


@pytest.mark.parametrize("mode", ["argmax", "slice", "slice_max"])
def test_opm_classes_fills_rows_of_per_class_stacks(dev, mode):
    """The class_stride form: forward batches of 2 + 1 copies write rows [i, i+b) of [K, N, h, w] stacks, as the hot path
    does; the stacks equal the single-class calls on the whole logits, and nothing outside the rows is touched."""
    from asr_amd import ops
    classes = 21
    ids = _sets(classes)[3]
    x = make_logits(classes, ids, seed=7)
    xd = ops.to_device(x, device=dev)
    sentinel = -12345.0
    y = torch.full((len(ids),) + SHAPE, sentinel, dtype=torch.float32, device=dev)
    ymax = torch.full_like(y, sentinel) if mode == "slice_max" else None
    for i, b in ((0, 2), (2, 1)):
        ops.opm_classes(xd[i:i + b].contiguous(), ids, mode, out=y[:, i:i + b],
                        out_max=ymax[:, i:i + b] if ymax is not None else None)
    for j, c in enumerate(ids):
        if mode == "argmax":
            assert _same(y[j], ops.opm_argmax(xd, c))
        elif mode == "slice":               # per-copy extrema: batching the copies changes nothing
            assert _same(y[j], ops.opm_slice(xd, c))
        else:
            rc, rm = ops.opm_slice_max(xd, c)
            assert _same(y[j], rc) and _same(ymax[j], rm)
    # a batch's call writes only its own rows
    z = torch.full_like(y, sentinel)
    ops.opm_classes(xd[1:2].contiguous(), ids, mode, out=z[:, 1:2],
                    out_max=torch.full_like(z, sentinel)[:, 1:2] if mode == "slice_max" else None)
    assert (z[:, 0] == sentinel).all() and (z[:, 2] == sentinel).all() and not (z[:, 1] == sentinel).any()


@pytest.mark.parametrize("with_mask", [False, True])
def test_threshold_classes_equals_single_class_calls_bitwise(dev, with_mask):
    from asr_amd import ops
    rng = np.random.default_rng(11)
    ids = [0, 5, 8, 15, 20]
    img = rng.standard_normal((len(ids), 67, 53)).astype(np.float32)
    img[1] *= np.float32(1e4)
    img[2, 3:9, 4:7] = np.float32(-0.0)
    img[2, 10:14, 4:7] = np.float32(0.0)
    img[3] = -np.abs(img[3])                 # a negative maximum
    d = ops.to_device(img, device=dev)
    th = ops.to_device(rng.standard_normal(img.shape).astype(np.float32), device=dev) if with_mask else None
    got = ops.threshold_classes(d, ids, th_factor=0.2, th_mask=th)
    for j, c in enumerate(ids):
        ref = ops.threshold(d[j].contiguous(), c, th_factor=0.2, th_mask=th[j].contiguous() if th is not None else None)
        assert _same(got[j], ref), c
        if j in (1, 2, 4):                    # segments with a positive maximum: some pixels on, some off
            assert 0 < (got[j] == c).float().mean().item() < 1
    # segment-wise thresholds: one segment's maximum does not leak into another's
    ref_all = ops.threshold(d, 8, th_factor=0.2, th_mask=th, segments=len(ids))
    assert _same(got[2], ref_all[2])


@pytest.mark.parametrize("k", [1, 3, 21])
@pytest.mark.parametrize("include_bg", [False, True])
def test_iou_counts_classes_equals_shared_truth_calls(dev, k, include_bg):
    from asr_amd import ops
    rng = np.random.default_rng(k)
    ids = _sets(21)[k]
    pixels = 300 * 301                        # not a multiple of 256
    labels = np.array(ids + [0, 255], np.int32)
    truth = rng.choice(labels, size=pixels).astype(np.int32)
    m = 4
    preds = np.empty((k, m, pixels), np.int32)
    for j, c in enumerate(ids):
        for r in range(m):                    # masks in {0, c} like thresholded masks, plus stray other labels
            p = np.where(rng.random(pixels) < 0.3 + 0.1 * r, c, 0).astype(np.int32)
            p[rng.random(pixels) < 0.01] = 255
            preds[j, r] = p
    td, pd = ops.to_device(truth, torch.int32, device=dev), ops.to_device(preds, torch.int32, device=dev)
    got = ops.iou_counts_classes(td, pd, ids, include_bg=include_bg).cpu().numpy()
    assert got.shape == (k, m, 4) and got.dtype == np.int64
    for j, c in enumerate(ids):
        ref = ops.iou_counts_shared_truth(td, pd[j].contiguous(), c, include_bg=include_bg).cpu().numpy()
        assert np.array_equal(got[j], ref), (c, got[j], ref)
        assert (ref[:, 0] > 0).all()          # non-empty intersections: the counts say something


@pytest.mark.parametrize("classes", [21, 40])
@pytest.mark.parametrize("k", [1, 3, 21])
def test_standard_mask_classes_equals_single_class_calls_bitwise(dev, classes, k):
    from asr_amd import ops
    ids = _sets(classes)[k]
    x = make_logits(classes, ids, seed=5 + k)[0]            # one [37, 41, C] logits map
    xd = ops.to_device(x, device=dev)
    for out_hw in ((148, 164), (37, 41), (100, 77)):
        got = ops.standard_mask_classes(xd, out_hw, ids)
        assert got.shape == (k,) + out_hw
        for j, c in enumerate(ids):
            ref = ops.standard_mask(xd, out_hw, c)
            assert _same(got[j], ref), (out_hw, c)
        if out_hw == (37, 41):                # no interpolation: the plain first-maximum argmax of the logits
            arg = _first_argmax(x)
            for j, c in enumerate(ids):
                assert np.array_equal(got[j].cpu().numpy(), np.where(arg == c, c, 0)), c
                assert c == 0 or (arg == c).any(), c
