"""The confusion matrices of HotPath.run_image_labels, evaluation.evaluate_labelmaps and scripts/validate_labelmap.py on the small
model input of tests/test_gpu_labelmap_path.py: asking for them changes no label map, count or score; they are the matrices of
the returned label maps (utils.confusion_matrix and the numpy restatement); their rows, columns and diagonals are the "counts"
of the same call; the dataset matrix is the sum of the images'; and the script's CSV holds every pixel of every image once."""
import csv
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_confusion_host import confusion_numpy
from test_gpu_labelmap_path import ANGLE, ITERS, N_AUG, REQ, SCRIPT, SHIFT, TH, _dataset, _run, _sr, _weights, _winners

sys.path.insert(0, GOLDEN)
from make_hotpath_traces import small_inputs  # noqa: E402

pytestmark = pytest.mark.gpu

L = 21


@pytest.fixture(scope="module")
def small(dev):
    return small_inputs(dev)


def _labels(small, mode="argmax", ids=REQ, **kw):
    from asr_amd.pipeline import HotPath
    model, img, gt, angles, shifts = small
    sr = _sr("adam", 6, 5, (16, 16), (64, 64), False)
    path = HotPath(model, sr, mode=mode, th_factor=TH, batch_size=4)
    return path.run_image_labels(img, angles, shifts, ids, gt_dev=gt, adam_starts={c: 3 * j for j, c in enumerate(ids)}, **kw)


def _check(res, ref, gt, keys):
    """res (with confusion_labels=L) against ref (the same call without) and against its own maps and counts."""
    from asr_amd.utils import confusion_matrix
    truth = gt.cpu().numpy()
    assert sorted(res["confusion"]) == sorted(keys)
    assert set(res) - {"confusion"} == set(ref)
    assert res["solved_ids"] == ref["solved_ids"]
    for key in keys:
        assert torch.equal(res[key], ref[key]), key
        assert np.array_equal(res["counts"][key], ref["counts"][key]), key
        a, b = res["Mean_IOU"][key], ref["Mean_IOU"][key]
        assert a == b or (np.isnan(a) and np.isnan(b)), key
        m = res["confusion"][key]
        assert m.dtype == np.int64 and m.shape == (L + 1, L + 1)
        assert np.array_equal(m, confusion_matrix(gt, res[key], L)), key
        assert np.array_equal(m, confusion_numpy(truth, res[key].cpu().numpy(), L)), key
        c = res["counts"][key]
        assert np.array_equal(m.sum(axis=1)[:L], c[0, :L]) and np.array_equal(m.sum(axis=0)[:L], c[1, :L]), key
        assert np.array_equal(np.diagonal(m)[:L], c[2, :L]) and int(m.sum()) == truth.size, key
    for extra in ("band_counts", "band_Mean_IOU"):
        if extra in ref:
            for key in keys:
                assert np.array_equal(res[extra][key], ref[extra][key], equal_nan=True), (extra, key)


def test_the_matrices_are_those_of_the_returned_maps_and_change_nothing(small):
    gt = small[2]
    ref, res = _labels(small), _labels(small, confusion_labels=L)
    assert "confusion" not in ref
    _check(res, ref, gt, ("standard", "aug", "max", "mean"))
    m = res["confusion"]["aug"]
    assert m[L].sum() == 2 * 64                                              # the void band of the ground truth, in the other row
    assert np.count_nonzero(m[:L, :L] - np.diag(np.diagonal(m[:L, :L]))) >= 2   # class-against-class confusion to look at
    assert m[12].sum() == 64                                                 # the 8 x 8 block of class 12 in the ground truth


def test_with_band_widths_the_band_counts_and_the_matrices_share_the_copy(small):
    gt = small[2]
    bands = dict(band_widths=(1, 4, 2), band_ignore_label=255)
    _check(_labels(small, confusion_labels=L, **bands), _labels(small, **bands), gt, ("standard", "aug", "max", "mean"))


def test_without_the_standard_map_and_with_one_sr_type(small):
    gt = small[2]
    kw = dict(want_standard=False, sr_types=("mean", "aug"))
    _check(_labels(small, confusion_labels=L, **kw), _labels(small, **kw), gt, ("aug", "mean"))


def test_no_class_left_fills_the_matrices_too(small):
    model, img, gt, angles, shifts = small
    won = _winners(model, img, angles, shifts)
    none = [c for c in (5, 12, 17) if c not in won]
    assert len(none) >= 2
    ref, res = _labels(small, ids=none), _labels(small, ids=none, confusion_labels=L)
    assert res["solved_ids"] == []
    _check(res, ref, gt, ("standard", "aug", "max", "mean"))
    for t in ("aug", "max", "mean"):
        assert np.count_nonzero(res["confusion"][t][:, 1:]) == 0 and res["confusion"][t][:, 0].sum() == 64 * 64


def test_a_matrix_needs_a_truth_and_1_to_64_labels(small):
    from asr_amd.pipeline import HotPath
    model, img, gt, angles, shifts = small
    path = HotPath(model, _sr("adam", 6, 5, (16, 16), (64, 64), False), mode="argmax", th_factor=TH, batch_size=4)
    with pytest.raises(ValueError):
        path.run_image_labels(img, angles, shifts, REQ, confusion_labels=L)
    for bad in (0, 65):
        with pytest.raises(ValueError):
            path.run_image_labels(img, angles, shifts, REQ, gt_dev=gt, confusion_labels=bad)


def test_evaluate_labelmaps_sums_the_images_matrices(small, tmp_path):
    from PIL import Image
    from bench import synth_image
    from asr_amd.evaluation import LABELMAP_KEYS, evaluate_labelmaps
    from asr_amd.pipeline import HotPath
    model, _, gt, _, _ = small
    images, gts = [], []
    for g in range(2):
        arr = synth_image(np.random.default_rng(21 + g), 64)
        images.append(str(tmp_path / f"{g}.png"))
        Image.fromarray(np.clip(np.rint(arr * 255.0), 0, 255).astype(np.uint8), mode="RGB").save(images[-1])
        lab = gt.cpu().numpy().astype(np.uint8)
        gts.append(str(tmp_path / f"gt{g}.png"))
        Image.fromarray(lab if g == 0 else lab[::-1].copy(), mode="L").save(gts[-1])
    run = lambda save, **kw: evaluate_labelmaps(
        HotPath(model, _sr("adam", 6, 5, (16, 16), (64, 64), False), mode="argmax", th_factor=TH, batch_size=4), images, gts,
        REQ, num_aug=6, angle_max=0.15, shift_max=8, img_size=(64, 64), save_dir=save, **kw)
    ref = run(str(tmp_path / "a"))
    out = run(str(tmp_path / "b"), confusion_labels=L)
    assert len(ref) == 2 and len(out) == 3
    assert np.array_equal(out[0], ref[0], equal_nan=True) and np.array_equal(out[1], ref[1])
    conf = out[2]
    assert conf.dtype == np.int64 and conf.shape == (4, L + 1, L + 1)
    for j, key in enumerate(LABELMAP_KEYS):
        want = sum(confusion_numpy(np.asarray(Image.open(gts[g])), np.asarray(Image.open(str(tmp_path / "b" / f"{g}_{key}.png"))), L)
                   for g in range(2))
        assert np.array_equal(conf[j], want), key
        assert np.array_equal(conf[j].sum(axis=1)[:L], out[1][j, 0, :L]) and int(conf[j].sum()) == 2 * 64 * 64
    with_bands = run(str(tmp_path / "c"), confusion_labels=L, band_widths=(2, 1))
    assert len(with_bands) == 5 and np.array_equal(with_bands[4], conf) and np.array_equal(with_bands[1], ref[1])


def test_the_script_writes_every_pixel_once_per_label_map(dev, tmp_path):
    from asr_amd.utils import metrics_from_confusion
    root = str(tmp_path)
    img_dir, gt_dir = _dataset(root)
    weights = _weights(root, dev)
    names = os.path.join(root, "names.txt")
    with open(names, "w") as fh:
        fh.write("\n".join(["background"] + [f"class{c}" for c in range(1, L)]) + "\n")
    conf = os.path.join(root, "conf.csv")
    _run([sys.executable, SCRIPT, "--images", img_dir, "--gt", gt_dir, "--num_aug", str(N_AUG), "--num_iter", str(ITERS), "--mode",
          "argmax", "--angle_max", str(ANGLE), "--shift_max", str(SHIFT), "--th_factor", str(TH), "--weights", weights, "--out",
          os.path.join(root, "one.csv"), "--confusion_out", conf, "--confusion_labels", str(L), "--class_names", names])
    with open(conf, newline="") as fh:
        rows = list(csv.reader(fh))
    assert rows[0] == ["key", "truth", "predicted", "pixels", "share_of_truth"]
    mats = {}
    for key in ("standard", "aug", "max", "mean"):
        mine = [r for r in rows[1:] if r[0] == key]
        assert len(mine) == (L + 1) ** 2 and mine[0][1:3] == ["background", "background"] and mine[-1][1:3] == ["other", "other"]
        assert sum(int(r[3]) for r in mine) == 2 * 512 * 512, key
        mats[key] = np.array([int(r[3]) for r in mine], np.int64).reshape(L + 1, L + 1)
        assert mats[key][L].sum() > 0 and mats[key][8].sum() > 0 and mats[key][12].sum() > 0       # void edge, both boxes
    with open(os.path.join(root, "conf_metrics.csv"), newline="") as fh:
        mrows = list(csv.reader(fh))
    got = {(r[0], r[1], r[2], r[3]): float(r[4]) for r in mrows[1:]}
    for key, m in mats.items():
        for other in ("ignore", "label"):
            assert got[(key, other, "Mean_IOU", "")] == metrics_from_confusion(m, other=other)["Mean_IOU"]
    # other="label" is the whole-image convention of the label-map CSV written by the same run
    with open(os.path.join(root, "one.csv"), newline="") as fh:
        one = {r[0]: r for r in csv.reader(fh)}
    for j, key in enumerate(("standard", "aug", "max", "mean")):
        assert float(one["dataset_mIoU"][1 + j]) == got[(key, "label", "Mean_IOU", "")], key
