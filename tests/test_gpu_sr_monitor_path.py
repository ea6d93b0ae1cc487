"""The convergence monitor in the upper layers, on the small model input of the label-map path tests:
HotPath.run_image_labels(sr_stop=...) -- nothing changes without it, patience 0 changes nothing but adds "sr_iters", a real
tolerance gives what Superresolution.augmented_superresolution_classes reports for the same stacks, the Adam counter ends where
it ends without -- and scripts/validate_labelmap.py --sr_stop_tol --sr_iters_out."""
import csv
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_gpu_labelmap_path import ANGLE, ITERS, N_AUG, REQ, SCRIPT, SHIFT, TH, _dataset, _run, _sr, _weights

sys.path.insert(0, GOLDEN)
from make_hotpath_traces import small_inputs  # noqa: E402

pytestmark = pytest.mark.gpu

SR_KEYS = ("aug", "max", "mean")
NUM_ITER = 12
STOP = dict(rel_tol=5e-2, patience=1, every=2, min_iter=2)       # loose enough that some class stops within 12 iterations


@pytest.fixture(scope="module")
def small(dev):
    return small_inputs(dev)


def _labels(small, mode, **kw):
    from asr_amd.pipeline import HotPath
    model, img, gt, angles, shifts = small
    sr = _sr("adam", 6, NUM_ITER, (16, 16), (64, 64), False)
    sr.optimizer.optimizer.iterations = 123
    starts = {c: 7 * j + 2 for j, c in enumerate(REQ)}
    path = HotPath(model, sr, mode=mode, th_factor=TH, batch_size=4)
    return path.run_image_labels(img, angles, shifts, REQ, gt_dev=gt, adam_starts=starts, **kw), starts, path


def _same(res, ref, extra=()):
    assert sorted(res) == sorted(list(ref) + list(extra)) and res["solved_ids"] == ref["solved_ids"]
    for key in ("standard",) + SR_KEYS:
        assert torch.equal(res[key], ref[key]), key
        assert np.array_equal(res["counts"][key], ref["counts"][key]), key
        assert res["Mean_IOU"][key] == ref["Mean_IOU"][key]


@pytest.mark.parametrize("mode", ["argmax", "slice_max"])
def test_without_sr_stop_nothing_changes_and_patience_0_only_adds_the_iterations(small, mode):
    plain, _, p0 = _labels(small, mode)
    none, _, p1 = _labels(small, mode, sr_stop=None)
    assert "sr_iters" not in plain and "sr_iters" not in none
    _same(none, plain)
    traced, _, p2 = _labels(small, mode, sr_stop=dict(patience=0, every=3))
    _same(traced, plain, extra=("sr_iters",))
    k = len(plain["solved_ids"])
    assert k >= 2 and sorted(traced["sr_iters"]) == (["aug", "aug_max"] if mode == "slice_max" else ["aug"])
    for its in traced["sr_iters"].values():
        assert its.dtype == np.int32 and np.array_equal(its, np.full(k, NUM_ITER, np.int32))
    assert p0.sr.optimizer.optimizer.iterations == p1.sr.optimizer.optimizer.iterations == p2.sr.optimizer.optimizer.iterations
    assert p2.sr.monitor is None                                         # the shared solver object is left as it was
    # without "aug" there is no solve to monitor
    no_aug, _, _ = _labels(small, mode, sr_types=("max", "mean"), sr_stop=STOP)
    assert no_aug["sr_iters"] == {}


@pytest.mark.parametrize("mode", ["argmax", "slice_max"])
def test_a_real_tolerance_reports_what_the_class_solve_reports(small, mode):
    from asr_amd import ops
    _, img, gt, angles, shifts = small
    plain, _, p0 = _labels(small, mode)
    res, starts, path = _labels(small, mode, sr_stop=STOP, keep_scores=True, coverages=[100], keep_uncertainty=True)
    solved, stacks = res["solved_ids"], res["uncertainty_stacks"]
    assert solved == plain["solved_ids"] and stacks.shape[0] == len(solved)
    its = res["sr_iters"]["aug"]
    print(mode, "sr_iters", res["sr_iters"])
    assert its.shape == (len(solved),) and its.min() >= STOP["min_iter"] and its.max() <= NUM_ITER
    assert its.min() < NUM_ITER, "the tolerance of this test is meant to stop at least one class"
    assert path.sr.optimizer.optimizer.iterations == p0.sr.optimizer.optimizer.iterations     # where it ends without sr_stop
    for t in ("max", "mean"):
        assert torch.equal(res[t], plain[t])
    assert torch.equal(res["standard"], plain["standard"])
    if mode != "argmax":
        return                      # (the stacks kept for the uncertainty are the argmax path's solver input as they are)
    fshifts = path._sr_frame(img, shifts)
    sr = _sr("adam", 6, NUM_ITER, (16, 16), (64, 64), False)
    sr.monitor = ops.check_sr_monitor(dict(STOP, history=True))
    scores = sr.augmented_superresolution_classes(stacks, angles, fshifts, [starts[c] for c in solved])[0]
    assert np.array_equal(sr.last_trace.iters_done.cpu().numpy(), its)
    assert torch.equal(scores, res["scores"]["aug"][0])
    hist = sr.last_trace.history.cpu().numpy()
    for b, k in enumerate(its):
        assert np.isnan(hist[:, b]).sum() == 4 * sum(1 for it in sr.last_trace.eval_iters if it > k)


def test_validate_labelmap_script_writes_the_iterations(dev, tmp_path):
    from asr_amd.evaluation import read_sr_iters_csv
    root = str(tmp_path)
    img_dir, gt_dir = _dataset(root)
    weights = _weights(root, dev)
    out, iters = os.path.join(root, "stop.csv"), os.path.join(root, "iters.csv")
    _run([sys.executable, SCRIPT, "--images", img_dir, "--gt", gt_dir, "--num_aug", str(N_AUG), "--num_iter", str(ITERS),
          "--mode", "argmax", "--angle_max", str(ANGLE), "--shift_max", str(SHIFT), "--th_factor", str(TH), "--weights", weights,
          "--out", out, "--no_prune", "--sr_stop_tol", "1e-2", "--sr_stop_patience", "1", "--sr_iters_out", iters])
    with open(out, newline="") as fh:
        rows = list(csv.reader(fh))
    assert rows[0] == ["Name", "standard_iou", "aug_iou", "max_iou", "mean_iou", "n"]
    got = read_sr_iters_csv(iters)
    images = sorted(os.path.splitext(f)[0] for f in os.listdir(img_dir))
    classes = sorted({c for _, c, _ in got}, key=int)
    assert len(classes) >= 2 and sorted(got) == sorted((i, c, k) for i in images for c in classes
                                                        for (gi, gc, k) in got if (gi, gc) == (i, c))
    assert len(got) == len(images) * len(classes)                       # one row per image and class
    assert all(0 <= k <= ITERS for _, _, k in got)
