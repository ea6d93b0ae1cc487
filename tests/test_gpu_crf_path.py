"""The windowed CRF in the upper layers: HotPath.run_image_labels(crf=...) on the small model input decides each SR map with
ops.crf_refine of ops.crf_unaries of exactly the scores a plain run fuses, bit for bit; crf=None is the call without the
keyword; standard_conf sends the standard map through the CRF too; with guide and min_region the order is guide -> CRF ->
clean-up; scripts/validate_labelmap.py --crf_iters keeps the CSV as it is laid out."""
import csv
import os
import sys

import numpy as np
import pytest
import torch

from test_gpu_guided_path import GUIDE, SR_KEYS, _labels
from test_gpu_labelmap_path import ANGLE, ITERS, N_AUG, REQ, SCRIPT, SHIFT, TH, _dataset, _run, _weights

pytestmark = pytest.mark.gpu

CRF = {"iterations": 3}


@pytest.fixture(scope="module")
def small(dev):
    from make_hotpath_traces import small_inputs                # tests/golden, put on the path by test_gpu_guided_path
    return small_inputs(dev)


def test_crf_none_is_the_call_without_the_keyword(small):
    plain, none = _labels(small, "argmax"), _labels(small, "argmax", crf=None)
    assert sorted(plain) == sorted(none) and plain["solved_ids"] == none["solved_ids"]
    for key in ("standard",) + SR_KEYS:
        assert torch.equal(plain[key], none[key]), key
        assert np.array_equal(plain["counts"][key], none["counts"][key]), key


def test_each_map_is_the_crf_of_the_scores_the_plain_run_fuses(small):
    from asr_amd import ops
    img, gt = small[1], small[2]
    plain = _labels(small, "argmax", keep_scores=True)
    res = _labels(small, "argmax", keep_scores=True, crf=CRF)
    solved = res["solved_ids"]
    assert solved == plain["solved_ids"] and len(solved) >= 2
    assert torch.equal(res["standard"], plain["standard"])                        # standard_conf None: left alone
    assert np.array_equal(res["counts"]["standard"], plain["counts"]["standard"])
    moved = 0
    for t in SR_KEYS:
        (s0, m0), (s1, m1) = plain["scores"][t], res["scores"][t]
        assert m0 is None and m1 is None and torch.equal(s0, s1), t
        want = ops.crf_refine(img, ops.crf_unaries(s1, TH), solved, CRF)
        assert torch.equal(res[t], want), t
        assert np.array_equal(res["counts"][t], ops.class_counts(gt, want)[0].cpu().numpy()), t
        moved += int(not torch.equal(res[t], plain[t]))
    assert moved                                                                  # the CRF did change label maps


def test_standard_conf_sends_the_standard_map_through_the_crf(small):
    from asr_amd import ops
    img, gt = small[1], small[2]
    plain = _labels(small, "argmax")
    res = _labels(small, "argmax", crf=dict(CRF, standard_conf=0.7))
    want = ops.crf_refine(img, ops.crf_unaries_from_labels(plain["standard"], REQ, 0.7), REQ, CRF)
    assert torch.equal(res["standard"], want)
    assert np.array_equal(res["counts"]["standard"], ops.class_counts(gt, want)[0].cpu().numpy())
    same = _labels(small, "argmax", crf=CRF)
    for t in SR_KEYS:                                                             # the SR maps do not depend on it
        assert torch.equal(res[t], same[t]), t


def test_with_guide_and_min_region_the_order_is_guide_crf_clean_up(small):
    from asr_amd import ops
    img, gt = small[1], small[2]
    region = (12, 4)
    plain = _labels(small, "argmax", keep_scores=True)
    res = _labels(small, "argmax", keep_scores=True, guide=GUIDE, crf=CRF, min_region=region)
    solved = res["solved_ids"]
    for t in SR_KEYS:
        guided = ops.guided_filter(img, plain["scores"][t][0], *GUIDE)
        assert torch.equal(res["scores"][t][0], guided), t
        raw = ops.crf_refine(img, ops.crf_unaries(guided, TH), solved, CRF)
        assert np.array_equal(res["raw_counts"][t], ops.class_counts(gt, raw)[0].cpu().numpy()), t
        want = ops.clean_labels(raw, *region)
        assert torch.equal(res[t], want), t
        assert np.array_equal(res["counts"][t], ops.class_counts(gt, want)[0].cpu().numpy()), t


def test_refusals_come_before_the_model(small):
    from asr_amd.pipeline import HotPath
    from test_gpu_labelmap_path import _sr
    model, img, gt, angles, shifts = small
    sr = _sr("adam", 6, 5, (16, 16), (64, 64), False)
    for mode, kw in (("slice_max", dict(crf=CRF)), ("argmax", dict(crf=CRF, th_factors=[0.1, 0.2])),
                     ("argmax", dict(crf={"radius": 8})), ("argmax", dict(crf={"standard_conf": 1.0}))):
        with pytest.raises(ValueError):
            HotPath(model, sr, mode=mode, th_factor=TH, batch_size=4).run_image_labels(img, angles, shifts, REQ, gt_dev=gt, **kw)
    assert sr.optimizer.optimizer.iterations == 0


def test_validate_labelmap_script_with_the_crf(dev, tmp_path):
    root = str(tmp_path)
    img_dir, gt_dir = _dataset(root)
    weights = _weights(root, dev)
    out = os.path.join(root, "crf.csv")
    _run([sys.executable, SCRIPT, "--images", img_dir, "--gt", gt_dir, "--num_aug", str(N_AUG), "--num_iter", str(ITERS),
          "--mode", "argmax", "--angle_max", str(ANGLE), "--shift_max", str(SHIFT), "--th_factor", str(TH), "--weights", weights,
          "--out", out, "--crf_iters", "3", "--band_widths", "2,8"])
    with open(out, newline="") as fh:
        rows = list(csv.reader(fh))
    assert rows[0] == ["Name", "standard_iou", "aug_iou", "max_iou", "mean_iou", "n"]
    assert [r[0] for r in rows[1:]] == ["Label 0", "Label 8", "Label 12", "dataset_mIoU", "mean_image_mIoU"]
    assert 0.0 < float(rows[4][2]) < 1.0
    with open(os.path.join(root, "crf_trimap.csv"), newline="") as fh:
        trimap = list(csv.reader(fh))
    from asr_amd.evaluation import TRIMAP_CSV_COLUMNS
    assert trimap[0] == ["Name"] + list(TRIMAP_CSV_COLUMNS) + ["band_pixels", "band_share", "n"]
    assert [r[0] for r in trimap[1:]] == ["w=2", "w=8"]
