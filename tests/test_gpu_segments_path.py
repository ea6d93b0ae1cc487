"""segments in HotPath.run_image_labels, evaluation.evaluate_labelmaps and scripts/validate_labelmap.py on the small model input
of tests/test_gpu_regions_path.py: the counts are ops.segment_match's and the restatement's on the returned maps, with min_region
the raw maps are matched too, and without the option nothing changes."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import segments_ref as S
from test_gpu_labelmap_path import ANGLE, ITERS, N_AUG, REQ, SCRIPT, SHIFT, TH, _dataset, _run, _weights
from test_gpu_regions_path import A, C, KEYS, _labels, _path, _same, small  # noqa: F401  (small: the module's fixture)

pytestmark = pytest.mark.gpu

L, CONN = 21, 8


@pytest.fixture(scope="module")
def runs(small):
    """(without the option, with segments=(L, CONN)), both with another score switched on"""
    kw = dict(confusion_labels=L)
    return _labels(small, **kw), _labels(small, segments=(L, CONN), **kw)


def _want(gt, label_map, num_labels=L, connectivity=CONN, include_zero=False):
    return S.segment_match(gt.cpu().numpy().astype(np.int32), label_map.cpu().numpy(), num_labels, connectivity, include_zero)[0]


def test_the_result_gains_the_segments_and_nothing_else_changes(small, runs):
    from asr_amd import ops, utils
    gt = small[2]
    ref, res = runs
    assert set(res) == set(ref) | {"segments"} and "segments" not in ref
    for key in set(ref):
        assert _same(res[key], ref[key]), key
    assert sorted(res["segments"]) == sorted(KEYS)
    total = 0
    for key in KEYS:
        got = res["segments"][key]
        assert got.dtype == np.int64 and got.shape == (L, 4)
        assert np.array_equal(got, ops.segment_match(gt.to(torch.int32), res[key], L, CONN).cpu().numpy()), key
        assert np.array_equal(got, utils.segment_counts(gt, res[key], L, CONN)), key
        assert np.array_equal(got, _want(gt, res[key])), key
        total += int(got[:, :3].sum())
    assert total > 0                                                                  # nothing above is vacuous


def test_with_min_region_the_raw_maps_are_matched_too(small, runs):
    gt = small[2]
    res = runs[1]
    fps = {}
    for conn, kw in ((CONN, dict(confusion_labels=L)), (4, {})):                      # the clean-up's labelling reused, and not
        both = _labels(small, min_region=(A, C), segments=(L, conn), **kw)
        clean = _labels(small, min_region=(A, C), **kw)
        assert set(both) == set(clean) | {"segments", "raw_segments"}
        for key in set(clean):
            assert _same(both[key], clean[key]), key
        for key in KEYS:
            if conn == CONN:
                assert np.array_equal(both["raw_segments"][key], res["segments"][key]), key   # = the run without min_region
            else:
                assert np.array_equal(both["raw_segments"][key], _want(gt, runs[0][key], connectivity=4)), key
            assert np.array_equal(both["segments"][key], _want(gt, both[key], connectivity=conn)), key   # on the cleaned maps
        fps[conn] = (sum(int(both["raw_segments"][k][:, 1].sum()) for k in KEYS), sum(int(both["segments"][k][:, 1].sum()) for k in KEYS))
    print(f"spurious segments (FP) over the four maps, raw -> final at min_region {A}: "
          + ", ".join(f"{c}-connected {a} -> {b}" for c, (a, b) in fps.items()))


def test_without_the_option_nothing_changes(small, runs):
    again = _labels(small, segments=None, confusion_labels=L)
    assert _same(again, runs[0])


def test_a_subset_of_the_maps_and_include_zero(small, runs):
    gt = small[2]
    res = _labels(small, segments=(L, 4, True), want_standard=False, sr_types=("mean", "aug"))
    assert sorted(res["segments"]) == ["aug", "mean"] and "raw_segments" not in res
    for key in ("aug", "mean"):
        assert torch.equal(res[key], runs[0][key])
        assert np.array_equal(res["segments"][key], _want(gt, res[key], connectivity=4, include_zero=True)), key
        row = res["segments"][key][0]
        assert bool(row[0] + row[2] > 0) == bool((gt == 0).any())                    # the truth's 0-regions are segments now


def test_bad_options_raise(small):
    model, img, gt, angles, shifts = small
    path = _path(model)
    with pytest.raises(ValueError, match="th_factors with segments"):
        path.run_image_labels(img, angles, shifts, REQ, gt_dev=gt, th_factors=[0.1, 0.3], segments=L)
    with pytest.raises(ValueError, match="segments needs gt_dev"):
        path.run_image_labels(img, angles, shifts, REQ, gt_dev=None, segments=L)
    for bad in (0, 65, (L, 6), 2.5):
        with pytest.raises(ValueError):
            path.run_image_labels(img, angles, shifts, REQ, gt_dev=gt, segments=bad)


def test_evaluate_labelmaps_sums_the_images(small, tmp_path):
    from PIL import Image
    from bench import synth_image
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
    out = run(str(tmp_path / "b"), segments=(L, CONN))
    assert len(ref) == 2 and len(out) == 3 and out.segments is out[2] and out.raw_segments is None and ref.segments is None
    assert np.array_equal(out.rows, ref.rows, equal_nan=True) and np.array_equal(out.counts, ref.counts)
    assert out.segments.shape == (4, L, 4) and out.segments.dtype == np.int64
    png = lambda d, g, key: np.asarray(Image.open(str(tmp_path / d / f"{g}_{key}.png"))).astype(np.int32)
    truth = [np.asarray(Image.open(p)).astype(np.int32) for p in gts]
    for j, key in enumerate(LABELMAP_KEYS):
        want = sum(S.segment_match(truth[g], png("b", g, key), L, CONN)[0] for g in range(2))
        assert np.array_equal(out.segments[j], want), key
    assert out.segments[:, :, :3].sum() > 0
    both = run(str(tmp_path / "c"), segments=(L, CONN), min_region=(A, C))
    assert len(both) == 7 and both.segments is both[5] and both.raw_segments is both[6] and both.regions is both[4]
    assert np.array_equal(both.raw_segments, out.segments)
    for j, key in enumerate(LABELMAP_KEYS):
        want = sum(S.segment_match(truth[g], png("c", g, key), L, CONN)[0] for g in range(2))
        assert np.array_equal(both.segments[j], want), key
    with pytest.raises(ValueError):
        run(None, segments=L, th_factors=[0.2])


def test_the_script_writes_the_segments_csv_and_is_unchanged_without_the_flag(dev, tmp_path):
    from PIL import Image
    from asr_amd import utils
    root = str(tmp_path)
    img_dir, gt_dir = _dataset(root)
    weights = _weights(root, dev)
    args = lambda tag: [sys.executable, SCRIPT, "--images", img_dir, "--gt", gt_dir, "--num_aug", str(N_AUG), "--num_iter", str(ITERS),
                        "--mode", "argmax", "--angle_max", str(ANGLE), "--shift_max", str(SHIFT), "--th_factor", str(TH), "--weights",
                        weights, "--out", os.path.join(root, tag, "miou.csv"), "--save_dir", os.path.join(root, tag, "maps")]
    seg_csv = os.path.join(root, "seg", "segments.csv")
    bad = subprocess.run(args("bad") + ["--segments_out", seg_csv, "--th_sweep"], capture_output=True, text=True, timeout=300)
    assert bad.returncode == 2 and "--segments_out with --th_sweep" in bad.stderr and not os.path.exists(os.path.join(root, "bad"))
    _run(args("plain"))
    _run(args("seg") + ["--segments_out", seg_csv])
    assert sorted(os.listdir(os.path.join(root, "plain"))) == ["maps", "miou.csv"]
    assert sorted(os.listdir(os.path.join(root, "seg"))) == ["maps", "miou.csv", "segments.csv"]
    # the flag changes no other output: miou.csv byte for byte
    assert open(os.path.join(root, "plain", "miou.csv"), "rb").read() == open(os.path.join(root, "seg", "miou.csv"), "rb").read()
    with open(seg_csv, newline="") as fh:
        got = list(csv.reader(fh))
    assert got[0] == ["key", "stage", "label", "TP", "FP", "FN", "precision", "recall", "SQ", "RQ", "PQ"]
    rows = got[1:]
    assert [r[0] for r in rows] == sorted((r[0] for r in rows), key=KEYS.index)
    for key in KEYS:
        counts = np.zeros((21, 4), np.int64)
        for g in range(2):
            truth = np.asarray(Image.open(os.path.join(gt_dir, f"{g}.png"))).astype(np.int32)
            label_map = np.asarray(Image.open(os.path.join(root, "seg", "maps", f"{g}_{key}.png"))).astype(np.int32)
            assert np.array_equal(label_map, np.asarray(Image.open(os.path.join(root, "plain", "maps", f"{g}_{key}.png")))), (g, key)
            counts += utils.segment_counts(truth, label_map, 21, 8)          # (checked against the restatement above and in the kernel tests)
        m = utils.metrics_from_segments(counts)
        mine = [r for r in rows if r[0] == key]
        seen = np.nonzero(counts[:, :3].sum(axis=1) > 0)[0].tolist()
        assert [r[1] for r in mine] == ["final"] * (len(seen) + 1) and [r[2] for r in mine] == [str(l) for l in seen] + ["mean"], key
        for r, l in zip(mine, seen):
            assert r[3:6] == [str(int(v)) for v in counts[l, :3]], (key, l)
            assert r[6:] == [repr(float(m[k][l])) for k in ("precision", "recall", "SQ", "RQ", "PQ")], (key, l)
        assert mine[-1][3:6] == [str(int(v)) for v in counts[:, :3].sum(axis=0)], key
        assert mine[-1][6:] == ["", ""] + [repr(m[k]) for k in ("mean_SQ", "mean_RQ", "mean_PQ")], key
    assert sum(int(r[3]) + int(r[4]) + int(r[5]) for r in rows if r[2] == "mean") > 0
