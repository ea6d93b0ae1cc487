"""GPU: the multi-label coupling through the upper layers -- ops.fuse_labels_simplex against the restatement
tests/sr_ml_ref.py, HotPath.run_image_labels(couple=True) on the small model of the label-map path tests, couple=False against
a run that never passes the keyword, and scripts/validate_labelmap.py --couple_classes."""
import csv
import os
import sys

import numpy as np
import pytest
import torch

from test_gpu_labelmap_path import ANGLE, ITERS, N_AUG, REQ, SCRIPT, SHIFT, TH, _dataset, _run, _weights
from test_gpu_sr_wtv import _upper

import sr_ml_ref as M

pytestmark = pytest.mark.gpu

LAM = (1.0, 0.3, 0.7, 0.0)


@pytest.fixture(scope="module")
def small(dev):
    return _upper()[1](dev)


def _sr(iters=5, **kw):
    from asr_amd.superresolution_scripts.optimizer import Optimizer
    from asr_amd.superresolution_scripts.superresolution import Superresolution
    return Superresolution(*LAM, num_iter=iters, num_aug=6, optimizer=Optimizer("primal_dual"), feature_size=(16, 16),
                           output_size=(64, 64), **kw)


def _labels(small, **kw):
    from asr_amd.pipeline import HotPath
    model, img, gt, angles, shifts = small
    return HotPath(model, _sr(), mode="argmax", th_factor=TH, batch_size=4).run_image_labels(img, angles, shifts, REQ, gt_dev=gt,
                                                                                            **kw)


# ---- the fusion kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 20])
def test_fuse_labels_simplex_is_the_restatement_bit_for_bit(dev, K):
    from asr_amd import ops
    rng = np.random.default_rng(K)
    ids = [int(v) for v in rng.permutation(np.arange(1, 40))[:K]]
    pixels = 4099
    s = (rng.random((K, pixels), dtype=np.float32) * np.float32(2.0 / K)).astype(np.float32)
    s[:, :200] = M.simplex_project(rng.normal(0.3, 0.6, (K, 200)).astype(np.float32))        # shares of a coupled solve
    # ties between the two largest, an exact S_k* == bg (0.25 against 1 - 0.75, and 0.5 against 1 - 0.5), nothing at all
    s[:, 200:210] = 0.0
    s[0, 200:205] = 0.5
    if K >= 3:
        s[:, 210:220] = 0.0
        s[0, 210:220] = s[1, 210:220] = s[2, 210:220] = 0.25
        s[K - 1, 220:230] = s[0, 220:230] = 0.4
        s[1:K - 1, 220:230] = 0.0
    s[:, 230:240] = 0.0
    want = M.fuse_labels_simplex(s, ids)
    got = ops.fuse_labels_simplex(ops.to_device(s), ids)
    assert got.dtype == torch.int32 and tuple(got.shape) == (pixels,)
    got = got.cpu().numpy()
    print(f"K={K}: {int((got != want).sum())} of {pixels} labels differ; {int((want == 0).sum())} background")
    assert np.array_equal(got, want)
    assert (want[200:205] == 0).all() and (want[230:240] == 0).all()             # S == bg is no win (strict); all zero is background
    if K >= 3:
        assert (want[210:220] == 0).all() and (want[220:230] == ids[0]).all()    # 0.25 == bg; a tie goes to the first
    assert (want != 0).any() and (want == 0).any()
    # a [K, H, W] stack and an out= destination
    out = torch.empty((64, 64), dtype=torch.int32, device=dev)
    s3 = np.ascontiguousarray(s[:, :4096].reshape(K, 64, 64))
    assert ops.fuse_labels_simplex(ops.to_device(s3), ids, out=out) is out
    assert np.array_equal(out.cpu().numpy(), want[:4096].reshape(64, 64))


# ---- run_image_labels -------------------------------------------------------------------------------------------------------------
def test_the_coupled_aug_map_is_the_fusion_of_its_own_scores(small):
    from asr_amd import ops
    gt = small[2]
    res = _labels(small, couple=True, keep_scores=True)
    plain = _labels(small, keep_scores=True)
    solved = res["solved_ids"]
    assert solved == plain["solved_ids"] and len(solved) >= 2
    tgt, tmax = res["scores"]["aug"]
    assert tmax is None
    assert torch.equal(res["aug"], ops.fuse_labels_simplex(tgt, solved))
    assert np.array_equal(res["counts"]["aug"], ops.class_counts(gt, res["aug"])[0].cpu().numpy())
    # the scores are a partition: x >= 0 and sum <= 1 (+ the rule's rounding), which the independent solves are not held to
    x = tgt.cpu().numpy()
    print(f"coupled: min {float(x.min()):.3e} max sum {float(x.astype(np.float64).sum(0).max()):.9f}; independent: min "
          f"{float(plain['scores']['aug'][0].min()):.3e} max sum {float(plain['scores']['aug'][0].double().sum(0).max()):.6f}")
    assert float(x.min()) >= 0.0 and float(x.astype(np.float64).sum(0).max()) <= 1.0 + 2e-6
    assert not torch.equal(tgt, plain["scores"]["aug"][0])
    # max, mean and standard are untouched
    for key in ("standard", "max", "mean"):
        assert torch.equal(res[key], plain[key]), key
        assert np.array_equal(res["counts"][key], plain["counts"][key]), key
    assert bool(torch.isfinite(tgt).all())


def test_couple_false_is_the_run_without_the_keyword(small):
    plain, off = _labels(small, keep_scores=True), _labels(small, keep_scores=True, couple=False)
    assert sorted(plain) == sorted(off) and plain["solved_ids"] == off["solved_ids"]
    for key in ("standard", "aug", "max", "mean"):
        assert torch.equal(plain[key], off[key]), key
        assert np.array_equal(plain["counts"][key], off["counts"][key]), key
        assert plain["Mean_IOU"][key] == off["Mean_IOU"][key], key
    for t in ("aug", "max", "mean"):
        assert torch.equal(plain["scores"][t][0], off["scores"][t][0]), t


def test_the_options_work_under_the_coupling(small):
    """guide runs before the fusion; sr_stop stops the classes together; one class left is a group of one."""
    from asr_amd import ops
    from asr_amd.pipeline import HotPath
    model, img, gt, angles, shifts = small
    res = _labels(small, couple=True, keep_scores=True, guide=(4, 1e-3), min_region=(12, 4), tv_guide=100.0)
    raw = ops.fuse_labels_simplex(res["scores"]["aug"][0], res["solved_ids"])
    assert np.array_equal(res["raw_counts"]["aug"], ops.class_counts(gt, raw)[0].cpu().numpy())
    assert torch.equal(res["aug"], ops.clean_labels(raw, 12, 4))
    res = _labels(small, couple=True, sr_stop=dict(rel_tol=1e-2, patience=1))
    its = res["sr_iters"]["aug"]
    assert len(its) == len(res["solved_ids"]) and len(set(its.tolist())) == 1
    one = HotPath(model, _sr(), mode="argmax", th_factor=TH, batch_size=4).run_image_labels(
        img, angles, shifts, res["solved_ids"][:1], gt_dev=gt, couple=True, keep_scores=True)
    x = one["scores"]["aug"][0]
    assert x.shape[0] == 1 and float(x.min()) >= 0.0 and float(x.max()) <= 1.0


# ---- scripts/validate_labelmap.py --couple_classes --------------------------------------------------------------------------------
def test_validate_labelmap_script_with_coupled_classes(dev, tmp_path):
    root = str(tmp_path)
    img_dir, gt_dir = _dataset(root)
    weights = _weights(root, dev)
    out = os.path.join(root, "ml.csv")
    _run([sys.executable, SCRIPT, "--images", img_dir, "--gt", gt_dir, "--num_aug", str(N_AUG), "--num_iter", str(ITERS),
          "--mode", "argmax", "--angle_max", str(ANGLE), "--shift_max", str(SHIFT), "--th_factor", str(TH), "--weights", weights,
          "--out", out, "--sr_optimizer", "primal_dual", "--couple_classes"])
    with open(out, newline="") as fh:
        rows = list(csv.reader(fh))
    assert rows[0] == ["Name", "standard_iou", "aug_iou", "max_iou", "mean_iou", "n"]
    assert [r[0] for r in rows[1:]] == ["Label 0", "Label 8", "Label 12", "dataset_mIoU", "mean_image_mIoU"]
    assert 0.0 < float(rows[4][2]) < 1.0
