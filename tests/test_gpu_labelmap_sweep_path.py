"""HotPath.run_image_labels(th_factors=...) on a small model input: the sweep counts of every SR type are the numpy rule applied
to the scores the fusion read, and row j is the "counts" of a fresh HotPath run at th_factor = th_factors[j]; asking for the
sweep changes nothing else of the result; the refusals; and scripts/validate_labelmap.py --th_factors on the golden cat image,
one rank and two."""
import csv
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_labelmap_host import counts_numpy
from test_labelmap_sweep_host import sweep_numpy
from test_gpu_labelmap_path import (ANGLE, ITERS, N_AUG, REQ, SCRIPT, SHIFT, TH, _dataset, _free_port, _run, _sr, _weights,
                                    _winners)

sys.path.insert(0, GOLDEN)
from make_hotpath_traces import small_inputs  # noqa: E402

pytestmark = pytest.mark.gpu

FACTORS = [0.5, 0.1, 0.2, 0.9, 0.35, 0.2, 0.65]              # unsorted, one repeat, the run's own TH = 0.2 among them
SR_KEYS = ("aug", "max", "mean")


@pytest.fixture(scope="module")
def small(dev):
    return small_inputs(dev)


def _labels(small, mode, th, starts, **kw):
    from asr_amd.pipeline import HotPath
    model, img, gt, angles, shifts = small
    sr = _sr("adam", 6, 5, (16, 16), (64, 64), False)
    sr.optimizer.optimizer.iterations = 123
    res = HotPath(model, sr, mode=mode, th_factor=th, batch_size=4).run_image_labels(img, angles, shifts, REQ, gt_dev=gt,
                                                                                     adam_starts=starts, **kw)
    return res, sr.optimizer.optimizer.iterations


@pytest.mark.parametrize("mode", ["argmax", "slice"])
def test_sweep_counts_are_the_rule_on_the_scores_and_each_factors_own_run(small, mode):
    from asr_amd.utils import mean_iou_from_counts
    truth = small[2].cpu().numpy()
    starts = {c: 7 * j + 2 for j, c in enumerate(REQ)}
    res, it = _labels(small, mode, TH, starts, th_factors=FACTORS, keep_scores=True)
    plain, it_plain = _labels(small, mode, TH, starts)
    assert sorted(res["sweep_counts"]) == sorted(SR_KEYS) == sorted(res["sweep_Mean_IOU"])
    assert "sweep_counts" not in plain and "sweep_Mean_IOU" not in plain
    solved = res["solved_ids"]
    assert len(solved) >= 2
    changed = 0
    for t in SR_KEYS:
        s, smax = res["scores"][t]
        assert smax is None
        got = res["sweep_counts"][t]
        assert got.shape == (len(FACTORS), 3, 256) and got.dtype == np.int64
        assert np.array_equal(got, sweep_numpy(s.cpu().numpy(), solved, truth, FACTORS)), t
        assert np.array_equal(got[FACTORS.index(TH)], res["counts"][t]), t                  # the run's own factor
        want = np.array([mean_iou_from_counts(c) for c in got])
        np.testing.assert_array_equal(res["sweep_Mean_IOU"][t], want)
        assert res["sweep_Mean_IOU"][t].dtype == np.float64
        changed += int(not np.array_equal(got[FACTORS.index(0.1)], got[FACTORS.index(0.9)]))
    assert changed                                                                         # the factor did move label maps
    # asking for the sweep changes nothing else
    assert it == it_plain == 123 and plain["solved_ids"] == solved
    for key in ("standard",) + SR_KEYS:
        assert torch.equal(res[key], plain[key]), key
        assert np.array_equal(res["counts"][key], plain["counts"][key]), key
        assert res["Mean_IOU"][key] == plain["Mean_IOU"][key] or np.isnan(plain["Mean_IOU"][key])
    # three factors against runs of their own
    for f in (0.1, 0.65, 0.9):
        own, _ = _labels(small, mode, f, starts)
        for t in SR_KEYS:
            assert np.array_equal(res["sweep_counts"][t][FACTORS.index(f)], own["counts"][t]), (f, t)


def test_refusals(small):
    from asr_amd.pipeline import HotPath
    model, img, gt, angles, shifts = small
    sr = _sr("adam", 6, 5, (16, 16), (64, 64), False)
    with pytest.raises(ValueError, match="plays no part"):
        HotPath(model, sr, mode="slice_max", th_factor=TH, batch_size=4).run_image_labels(img, angles, shifts, REQ, gt_dev=gt,
                                                                                           th_factors=FACTORS)
    with pytest.raises(ValueError, match="gt_dev"):
        HotPath(model, sr, mode="argmax", th_factor=TH, batch_size=4).run_image_labels(img, angles, shifts, REQ,
                                                                                        th_factors=FACTORS)
    with pytest.raises(ValueError, match="threshold factors"):
        HotPath(model, sr, mode="argmax", th_factor=TH, batch_size=4).run_image_labels(img, angles, shifts, REQ, gt_dev=gt,
                                                                                        th_factors=[0.1] * 65)
    assert sr.optimizer.optimizer.iterations == 0


def test_every_class_pruned_gives_the_zero_maps_counts_under_every_factor(small):
    from asr_amd.pipeline import HotPath
    model, img, gt, angles, shifts = small
    won = _winners(model, img, angles, shifts)
    none = [c for c in (5, 12, 17) if c not in won]
    assert len(none) >= 2
    sr = _sr("adam", 6, 5, (16, 16), (64, 64), False)
    res = HotPath(model, sr, mode="argmax", th_factor=TH, batch_size=6).run_image_labels(img, angles, shifts, none, gt_dev=gt,
                                                                                         th_factors=FACTORS)
    assert res["solved_ids"] == []
    zero = counts_numpy(gt.cpu().numpy(), np.zeros((64, 64), np.int32))
    for t in SR_KEYS:
        assert res["sweep_counts"][t].shape == (len(FACTORS), 3, 256)
        assert all(np.array_equal(row, zero) for row in res["sweep_counts"][t]), t
        assert np.array_equal(res["counts"][t], zero)


# ---- scripts/validate_labelmap.py --th_factors ------------------------------------------------------------------------------
def test_validate_labelmap_script_writes_the_threshold_curve(dev, tmp_path):
    root = str(tmp_path)
    img_dir, gt_dir = _dataset(root)
    weights = _weights(root, dev)
    args = lambda out: ["--images", img_dir, "--gt", gt_dir, "--num_aug", str(N_AUG), "--num_iter", str(ITERS), "--mode",
                        "argmax", "--angle_max", str(ANGLE), "--shift_max", str(SHIFT), "--th_factor", str(TH),
                        "--weights", weights, "--out", out]
    sweep = lambda curve: ["--th_factors", "0.1,0.2,0.5,0.9", "--th_sweep_out", curve]
    plain, out1, curve1 = os.path.join(root, "plain.csv"), os.path.join(root, "one.csv"), os.path.join(root, "one_th.csv")
    _run([sys.executable, SCRIPT] + args(plain))
    _run([sys.executable, SCRIPT] + args(out1) + sweep(curve1))
    assert not os.path.exists(os.path.join(root, "plain_thresholds.csv"))
    with open(plain, "rb") as a, open(out1, "rb") as b:
        assert a.read() == b.read()                                     # --out is what it was without the flags
    with open(curve1, newline="") as fh:
        rows = list(csv.reader(fh))
    with open(out1, newline="") as fh:
        lm = {r[0]: r for r in csv.reader(fh)}
    assert rows[0][0] == "th_factor" and [r[0] for r in rows[1:]] == ["0.1", "0.2", "0.5", "0.9"]
    own = rows[2]                                                       # the row at the run's own --th_factor
    assert [own[1], own[3], own[5], own[7]] == [lm["dataset_mIoU"][k] for k in (2, 3, 4, 1)]
    assert [own[2], own[4], own[6], own[8]] == [lm["mean_image_mIoU"][k] for k in (2, 3, 4, 1)]
    assert len({r[1] for r in rows[1:]}) >= 2                           # the curve is not flat
    assert all(r[7:] == own[7:] for r in rows[1:])                      # the standard columns are constants
    # 2 ranks (gloo collectives) on the one GPU: the same bytes
    out2, curve2 = os.path.join(root, "two.csv"), os.path.join(root, "two_th.csv")
    env = dict(os.environ, ASR_DIST_BACKEND="gloo")
    _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
          "--master-port", str(_free_port()), SCRIPT] + args(out2) + sweep(curve2), env=env)
    for a, b in ((out1, out2), (curve1, curve2)):
        with open(a, "rb") as fa, open(b, "rb") as fb:
            assert fa.read() == fb.read()
