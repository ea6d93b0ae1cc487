"""min_region in HotPath.run_image_labels, evaluation.evaluate_labelmaps and scripts/validate_labelmap.py on the small model input
of tests/test_gpu_confusion_path.py: the maps are ops.clean_labels of the maps of a run without the option, every score is taken
on the cleaned maps, the raw scores and the region statistics come along, and without the option nothing changes."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import regions_ref as R
from conftest import GOLDEN
from test_gpu_labelmap_path import ANGLE, ITERS, N_AUG, REQ, SCRIPT, SHIFT, TH, _dataset, _run, _sr, _weights, _winners
from test_labelmap_host import counts_numpy

sys.path.insert(0, GOLDEN)
from make_hotpath_traces import small_inputs  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("standard", "aug", "max", "mean")
A, C = 16, 8                                   # regions of fewer than 16 pixels, 8-connectivity
L = 21
NEW = {"raw_counts", "raw_Mean_IOU", "regions"}


@pytest.fixture(scope="module")
def small(dev):
    return small_inputs(dev)


def _path(model, mode="argmax"):
    from asr_amd.pipeline import HotPath
    return HotPath(model, _sr("adam", 6, 5, (16, 16), (64, 64), False), mode=mode, th_factor=TH, batch_size=4)


def _labels(small, ids=REQ, with_gt=True, **kw):
    model, img, gt, angles, shifts = small
    return _path(model).run_image_labels(img, angles, shifts, ids, gt_dev=gt if with_gt else None,
                                         adam_starts={c: 3 * j for j, c in enumerate(ids)}, **kw)


def _same(a, b):
    if isinstance(a, dict):
        return sorted(a) == sorted(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, torch.Tensor):
        return torch.equal(a, b)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return bool(np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)) if not isinstance(a, (type(None), str)) else a == b


@pytest.fixture(scope="module")
def runs(small):
    """(without the option, with min_region=(A, C)), both with every other score switched on"""
    kw = dict(band_widths=(1, 3), confusion_labels=L, coverages=(50, 100), keep_uncertainty=True)
    return _labels(small, **kw), _labels(small, min_region=(A, C), **kw)


def test_the_maps_are_the_cleaned_maps_of_a_run_without_the_option(small, runs):
    from asr_amd import ops, utils
    gt = small[2]
    ref, res = runs
    assert set(res) == set(ref) | NEW and not NEW & set(ref)
    assert res["solved_ids"] == ref["solved_ids"]
    changed = 0
    for key in KEYS:
        raw = ref[key]
        want = ops.clean_labels(raw, A, C)
        assert torch.equal(res[key], want), key
        host, stats = R.clean_labels(raw.cpu().numpy(), A, C)                      # and the restatement of the definitions
        assert np.array_equal(res[key].cpu().numpy(), host), key
        changed += int(stats[3])
        assert res["regions"][key].dtype == np.int64 and res["regions"][key].shape == (4,)
        assert np.array_equal(res["regions"][key], utils.region_stats(raw, A, C)) and np.array_equal(res["regions"][key], stats), key
        assert np.array_equal(res["counts"][key], ops.class_counts(gt.to(torch.int32).reshape(-1), res[key].reshape(-1))[0].cpu().numpy())
        assert res["Mean_IOU"][key] == utils.mean_iou_from_counts(res["counts"][key]) or np.isnan(res["Mean_IOU"][key])
        assert np.array_equal(res["raw_counts"][key], ref["counts"][key]), key
        assert _same(res["raw_Mean_IOU"][key], ref["Mean_IOU"][key]), key
        # the other scores see the cleaned maps
        assert np.array_equal(res["band_counts"][key], utils.trimap_counts(gt, res[key], (1, 3))), key
        assert np.array_equal(res["confusion"][key], utils.confusion_matrix(gt, res[key], L)), key
        assert np.array_equal(res["coverage_counts"][key], utils.risk_coverage_counts(gt, res[key], res["uncertainty"], (50, 100))), key
    assert changed > 0                                                               # the fixture has specks: nothing above is vacuous
    assert any(not torch.equal(res[key], ref[key]) for key in KEYS)


def test_without_the_option_nothing_changes_and_min_region_1_keeps_the_maps(small, runs):
    ref = runs[0]
    kw = dict(band_widths=(1, 3), confusion_labels=L, coverages=(50, 100), keep_uncertainty=True)
    again = _labels(small, min_region=None, **kw)
    assert _same(again, ref)
    one = _labels(small, min_region=1, **kw)
    assert set(one) == set(ref) | NEW
    for key in set(ref):
        assert _same(one[key], ref[key]), key
    for key in KEYS:
        assert np.array_equal(one["raw_counts"][key], ref["counts"][key]) and not one["regions"][key][1:].any()
        assert one["regions"][key][0] == np.count_nonzero(R.label_regions(ref[key].cpu().numpy(), 4)[0].ravel() == np.arange(64 * 64))


def test_without_a_ground_truth_and_with_a_subset_of_the_maps(small, runs):
    from asr_amd import ops
    ref = runs[0]
    res = _labels(small, with_gt=False, min_region=A, want_standard=False, sr_types=("mean", "aug"))
    assert set(res) == {"aug", "mean", "solved_ids", "regions"} and sorted(res["regions"]) == ["aug", "mean"]
    for key in ("aug", "mean"):
        want, stats = ops.clean_labels(ref[key], A, 4, want_stats=True)
        assert torch.equal(res[key], want) and np.array_equal(res["regions"][key], stats.cpu().numpy())


def test_no_class_left_still_runs_the_calls(small):
    model, img, gt, angles, shifts = small
    won = _winners(model, img, angles, shifts)
    none = [c for c in (5, 12, 17) if c not in won]
    assert len(none) >= 2
    ref, res = _labels(small, ids=none), _labels(small, ids=none, min_region=(A, C))
    assert res["solved_ids"] == []
    for t in ("aug", "max", "mean"):                                                # a zero map is one region, and it is not small
        assert not res[t].any() and res["regions"][t].tolist() == [1, 0, 0, 0]
        assert np.array_equal(res["counts"][t], ref["counts"][t]) and np.array_equal(res["raw_counts"][t], ref["counts"][t])
    assert torch.equal(res["standard"], __import__("asr_amd").ops.clean_labels(ref["standard"], A, C))


def test_bad_options_raise(small):
    model, img, gt, angles, shifts = small
    path = _path(model)
    with pytest.raises(ValueError, match="th_factors with min_region"):
        path.run_image_labels(img, angles, shifts, REQ, gt_dev=gt, th_factors=[0.1, 0.3], min_region=4)
    for bad in (0, (4, 6), 2.5):
        with pytest.raises(ValueError):
            path.run_image_labels(img, angles, shifts, REQ, gt_dev=gt, min_region=bad)


def test_evaluate_labelmaps_sums_the_images(small, tmp_path):
    from PIL import Image
    from bench import synth_image
    from asr_amd import utils
    from asr_amd.evaluation import LABELMAP_KEYS, evaluate_labelmaps
    model, _, gt, _, _ = small
    images, gts = [], []
    for g in range(2):
        arr = synth_image(np.random.default_rng(21 + g), 64)
        images.append(str(tmp_path / f"{g}.png"))
        Image.fromarray(np.clip(np.rint(arr * 255.0), 0, 255).astype(np.uint8), mode="RGB").save(images[-1])
        lab = gt.cpu().numpy().astype(np.uint8)
        gts.append(str(tmp_path / f"gt{g}.png"))
        Image.fromarray(lab if g == 0 else lab[::-1].copy(), mode="L").save(gts[-1])
    run = lambda save, **kw: evaluate_labelmaps(_path(model), images, gts, REQ, num_aug=6, angle_max=0.15, shift_max=8,
                                                img_size=(64, 64), save_dir=save, **kw)
    ref = run(str(tmp_path / "a"))
    out = run(str(tmp_path / "b"), min_region=(A, C))
    assert len(ref) == 2 and len(out) == 5
    assert out.raw_rows is out[2] and out.raw_counts is out[3] and out.regions is out[4] and out.rows is out[0] and out.counts is out[1]
    assert out.raw_rows.shape == (2, 4) and out.raw_counts.shape == (4, 3, 256) and out.regions.shape == (4, 4)
    assert out.regions.dtype == np.int64 and out.raw_counts.dtype == np.int64
    assert np.array_equal(out.raw_rows, ref[0], equal_nan=True) and np.array_equal(out.raw_counts, ref[1])
    png = lambda d, g, key: np.asarray(Image.open(str(tmp_path / d / f"{g}_{key}.png"))).astype(np.int32)
    changed = 0
    for j, key in enumerate(LABELMAP_KEYS):
        stats, counts = np.zeros(4, np.int64), np.zeros((3, 256), np.int64)
        for g in range(2):
            raw = png("a", g, key)
            want, s = R.clean_labels(raw, A, C)
            assert np.array_equal(png("b", g, key), want), (g, key)                  # save_dir holds the cleaned maps
            stats += s
            truth = np.asarray(Image.open(gts[g])).astype(np.int32)
            counts += counts_numpy(truth, want)
            assert out.rows[g, j] == utils.mean_iou_from_counts(counts_numpy(truth, want)), (g, key)
        assert np.array_equal(out.regions[j], stats) and np.array_equal(out.counts[j], counts), key
        changed += int(stats[3])
    assert changed > 0
    both = run(str(tmp_path / "c"), min_region=(A, C), confusion_labels=L)
    assert len(both) == 6 and both.confusion is both[2] and both.regions is both[5]
    assert np.array_equal(both[5], out.regions) and np.array_equal(both[1], out.counts) and np.array_equal(both[4], ref[1])
    with pytest.raises(ValueError):
        run(None, min_region=4, th_factors=[0.2])


def test_the_script_writes_the_regions_csv_and_is_unchanged_without_the_flag(dev, tmp_path):
    from PIL import Image
    from asr_amd import utils
    root = str(tmp_path)
    img_dir, gt_dir = _dataset(root)
    weights = _weights(root, dev)
    args = lambda tag: [sys.executable, SCRIPT, "--images", img_dir, "--gt", gt_dir, "--num_aug", str(N_AUG), "--num_iter", str(ITERS),
                        "--mode", "argmax", "--angle_max", str(ANGLE), "--shift_max", str(SHIFT), "--th_factor", str(TH), "--weights",
                        weights, "--out", os.path.join(root, tag + ".csv"), "--save_dir", os.path.join(root, tag)]
    bad = subprocess.run(args("bad") + ["--min_region", "9", "--th_sweep"], capture_output=True, text=True, timeout=300)
    assert bad.returncode == 2 and "--min_region with --th_sweep" in bad.stderr and not os.path.exists(os.path.join(root, "bad.csv"))
    _run(args("plain"))
    _run(args("clean") + ["--min_region", "40", "--region_connectivity", "8"])
    assert not os.path.exists(os.path.join(root, "plain_regions.csv"))
    assert sorted(os.listdir(root)) == sorted(["images", "gt", "weights.npz", "plain", "plain.csv", "clean", "clean.csv",
                                               "clean_regions.csv"])
    read = lambda name: list(csv.reader(open(os.path.join(root, name), newline="")))
    plain, clean, reg = read("plain.csv"), read("clean.csv"), read("clean_regions.csv")
    assert reg[0] == ["key", "regions", "small_regions", "small_region_pixels", "pixels_changed", "raw_dataset_mIoU",
                      "raw_mean_image_mIoU", "dataset_mIoU", "mean_image_mIoU"] and [r[0] for r in reg[1:]] == list(KEYS)
    by = lambda rows: {r[0]: r for r in rows}
    total_changed = 0
    for j, key in enumerate(KEYS):
        row = reg[1 + j]
        # before the clean-up: the very cells of the run without the flag; after it: those of the run's own CSV
        assert row[5] == by(plain)["dataset_mIoU"][1 + j] and row[6] == by(plain)["mean_image_mIoU"][1 + j], key
        assert row[7] == by(clean)["dataset_mIoU"][1 + j] and row[8] == by(clean)["mean_image_mIoU"][1 + j], key
        stats = np.zeros(4, np.int64)
        for g in range(2):
            raw = np.asarray(Image.open(os.path.join(root, "plain", f"{g}_{key}.png"))).astype(np.int32)
            got = np.asarray(Image.open(os.path.join(root, "clean", f"{g}_{key}.png"))).astype(np.int32)
            assert np.array_equal(got, utils.remove_small_regions(raw, 40, 8)), (g, key)
            stats += utils.region_stats(raw, 40, 8)
        assert [int(v) for v in row[1:5]] == stats.tolist(), key
        total_changed += int(stats[3])
    assert total_changed > 0
