"""The guided filter in the upper layers: HotPath.run_image_labels(guide=...) on the small model input refines exactly the
scores an unguided run fuses (ops.guided_filter of them against the image, bit for bit) and fuses those; guide=None is the call
without the keyword; compute_SR(guide=...) on the golden interchange files thresholds guided_refine of the unguided target;
scripts/validate_labelmap.py --guide_radius keeps the CSV as it is laid out."""
import csv
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_gpu_labelmap_path import ANGLE, ITERS, N_AUG, REQ, SCRIPT, SHIFT, TH, _dataset, _run, _sr, _weights
from test_gpu_realign_covered import _golden, _sr as _sr_golden

sys.path.insert(0, GOLDEN)
from make_hotpath_traces import small_inputs  # noqa: E402

pytestmark = pytest.mark.gpu

SR_KEYS = ("aug", "max", "mean")
GUIDE = (4, 1e-3)


@pytest.fixture(scope="module")
def small(dev):
    return small_inputs(dev)


def _labels(small, mode, **kw):
    from asr_amd.pipeline import HotPath
    model, img, gt, angles, shifts = small
    sr = _sr("adam", 6, 5, (16, 16), (64, 64), False)
    sr.optimizer.optimizer.iterations = 123
    starts = {c: 7 * j + 2 for j, c in enumerate(REQ)}
    return HotPath(model, sr, mode=mode, th_factor=TH, batch_size=4).run_image_labels(img, angles, shifts, REQ, gt_dev=gt,
                                                                                     adam_starts=starts, **kw)


def test_guide_none_is_the_call_without_the_keyword(small):
    plain, none = _labels(small, "argmax"), _labels(small, "argmax", guide=None)
    assert sorted(plain) == sorted(none) and plain["solved_ids"] == none["solved_ids"]
    for key in ("standard",) + SR_KEYS:
        assert torch.equal(plain[key], none[key]), key
        assert np.array_equal(plain["counts"][key], none["counts"][key]), key


@pytest.mark.parametrize("mode", ["argmax", "slice_max"])
def test_guided_scores_are_the_filter_of_the_unguided_scores_and_the_maps_their_fusion(small, mode):
    from asr_amd import ops
    img, gt = small[1], small[2]
    plain = _labels(small, mode, keep_scores=True)
    res = _labels(small, mode, keep_scores=True, guide=GUIDE)
    solved = res["solved_ids"]
    assert solved == plain["solved_ids"] and len(solved) >= 2
    assert torch.equal(res["standard"], plain["standard"])
    moved = 0
    for t in SR_KEYS:
        (s0, m0), (s1, m1) = plain["scores"][t], res["scores"][t]
        assert (m0 is None) == (m1 is None) == (mode != "slice_max")
        assert torch.equal(s1, ops.guided_filter(img, s0, *GUIDE)), t
        if m0 is not None:
            assert torch.equal(m1, ops.guided_filter(img, m0, *GUIDE)), t
        labels, counts = ops.fuse_labels(s1, solved, th_factor=TH, max_scores=m1, truth=gt, classes=21)
        assert torch.equal(res[t], labels), t
        assert np.array_equal(res["counts"][t], counts.cpu().numpy()), t
        moved += int(not torch.equal(res[t], plain[t]))
    assert moved                                                                  # the filter did change label maps


def test_refusals(small):
    from asr_amd.pipeline import HotPath
    model, img, gt, angles, shifts = small
    sr = _sr("adam", 6, 5, (16, 16), (64, 64), False)
    path = HotPath(model, sr, mode="argmax", th_factor=TH, batch_size=4)
    for bad in ((4, 0.0), (4, -1e-3), (4, float("inf")), (33, 1e-3), (-1, 1e-3), (2.5, 1e-3), 4):
        with pytest.raises(ValueError):
            path.run_image_labels(img, angles, shifts, REQ, gt_dev=gt, guide=bad)
    assert sr.optimizer.optimizer.iterations == 0


@pytest.mark.parametrize("mode", ["argmax", "slice_max"])
def test_compute_SR_with_a_guide(dev, tmp_path, mode):
    from asr_amd.superresolution_scripts.superres_utils import compute_SR, guided_refine, threshold_image
    _path, n, lr, hr, masks, max_masks, angles, shifts, name = _golden(mode)
    mm = max_masks if max_masks is not None else []
    guide = np.random.default_rng(5).uniform(0, 1, hr + (3,)).astype(np.float32)
    guide[:, hr[1] // 2:] *= 0.25
    for t in ("mean", "aug"):
        fresh = lambda: _sr_golden(lr, hr, n)                                # a fresh Adam counter for every solve
        got = compute_SR(fresh(), masks, angles, shifts, name, str(tmp_path), SR_type=t, max_masks=mm, class_id=8,
                         th_factor=0.3, guide=guide, guide_radius=2, guide_eps=1e-2)
        plain = compute_SR(fresh(), masks, angles, shifts, name, str(tmp_path), SR_type=t, max_masks=mm, class_id=8,
                           th_factor=0.3)
        sr = fresh()
        fn = sr.augmented_superresolution if t == "aug" else sr.mean_superresolution
        target = guided_refine(fn(masks, angles, shifts)[0], guide, 2, 1e-2)
        assert target.shape == hr + (1,) and target.dtype == np.float32
        if mode == "slice_max":
            want = threshold_image(target, 8, th_mask=guided_refine(fn(max_masks, angles, shifts)[0], guide, 2, 1e-2))
        else:
            want = threshold_image(target, 8, th_factor=0.3)
        assert got.shape == hr + (1,) and np.array_equal(got, want), t
        assert plain.shape == got.shape and set(np.unique(got)) <= {0, 8}
    # the three accepted layouts agree, host in gives host out and device in gives device out
    score = np.random.default_rng(6).normal(0, 1, (3,) + hr).astype(np.float32)
    q = guided_refine(score, guide, 2, 1e-2)
    assert isinstance(q, np.ndarray) and q.shape == score.shape
    assert np.array_equal(guided_refine(score[1], guide, 2, 1e-2), q[1])
    assert np.array_equal(guided_refine(score[1][..., None], guide, 2, 1e-2), q[1][..., None])
    qd = guided_refine(torch.as_tensor(score).to(dev), torch.as_tensor(guide).to(dev), 2, 1e-2)
    assert isinstance(qd, torch.Tensor) and qd.is_cuda and np.array_equal(qd.cpu().numpy(), q)


def test_validate_labelmap_script_with_a_guide(dev, tmp_path):
    root = str(tmp_path)
    img_dir, gt_dir = _dataset(root)
    weights = _weights(root, dev)
    out = os.path.join(root, "guided.csv")
    _run([sys.executable, SCRIPT, "--images", img_dir, "--gt", gt_dir, "--num_aug", str(N_AUG), "--num_iter", str(ITERS),
          "--mode", "argmax", "--angle_max", str(ANGLE), "--shift_max", str(SHIFT), "--th_factor", str(TH), "--weights", weights,
          "--out", out, "--guide_radius", "4", "--band_widths", "2,8"])
    with open(out, newline="") as fh:
        rows = list(csv.reader(fh))
    assert rows[0] == ["Name", "standard_iou", "aug_iou", "max_iou", "mean_iou", "n"]
    assert [r[0] for r in rows[1:]] == ["Label 0", "Label 8", "Label 12", "dataset_mIoU", "mean_image_mIoU"]
    assert 0.0 < float(rows[4][2]) < 1.0
    with open(os.path.join(root, "guided_trimap.csv"), newline="") as fh:
        trimap = list(csv.reader(fh))
    from asr_amd.evaluation import TRIMAP_CSV_COLUMNS
    assert trimap[0] == ["Name"] + list(TRIMAP_CSV_COLUMNS) + ["band_pixels", "band_share", "n"]
    assert [r[0] for r in trimap[1:]] == ["w=2", "w=8"]
