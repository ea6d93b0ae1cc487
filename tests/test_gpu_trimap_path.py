"""The trimap through the label-map path: HotPath.run_image_labels(band_widths=...) changes nothing it returned before and its
band counts are utils.trimap_counts of the label maps it returns (and the numpy restatement's); scripts/validate_labelmap.py
with --band_widths writes a trimap CSV whose cells are recomputed here from the saved PNGs, and the same main CSV bytes as
without the flags."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_gpu_labelmap_path import KEYS, REQ, SCRIPT, TH, _dataset, _sr, _weights, _winners, small  # noqa: F401
from test_labelmap_host import counts_numpy
from test_trimap_host import assert_bands_say_something, band_counts_numpy, blob_map, dist2_numpy

pytestmark = pytest.mark.gpu

BANDS = [3, 1, 2, 1]                      # unsorted, with a repeat


def _gt(dev):
    t = blob_map(20, 64, 64, labels=(3, 8), ring=1)
    assert_bands_say_something(t, dist2_numpy(t, 3), BANDS)
    return t, torch.from_numpy(t).to(dev)


def _same(a, b):
    return (a == b) or (np.isnan(a) and np.isnan(b))


@pytest.mark.parametrize("mode,prune", [("argmax", True), ("argmax", False), ("slice_max", True)])
def test_band_widths_add_the_band_counts_and_change_nothing_else(small, dev, mode, prune):
    from asr_amd import utils
    from asr_amd.pipeline import HotPath
    model, img, _gt_small, angles, shifts = small
    truth, gt = _gt(dev)
    out = {}
    for bands in (None, BANDS):
        sr = _sr("adam", 6, 5, (16, 16), (64, 64), False)
        sr.optimizer.optimizer.iterations = 40
        extra = {} if bands is None else dict(band_widths=bands, band_ignore_label=255)
        res = HotPath(model, sr, mode=mode, th_factor=TH, batch_size=4).run_image_labels(img, angles, shifts, REQ, gt_dev=gt,
                                                                                         prune=prune, **extra)
        out[bands is None] = (res, sr.optimizer.optimizer.iterations)
    (a, it_a), (b, it_b) = out[True], out[False]
    assert sorted(a) == sorted(k for k in b if not k.startswith("band_")) and "band_counts" in b and "band_Mean_IOU" in b
    assert it_a == it_b and a["solved_ids"] == b["solved_ids"]
    for key in KEYS:
        assert torch.equal(a[key], b[key]), key
        assert np.array_equal(a["counts"][key], b["counts"][key]), key
        assert _same(a["Mean_IOU"][key], b["Mean_IOU"][key]), key
        lab = b[key].cpu().numpy()
        assert np.array_equal(b["counts"][key], counts_numpy(truth, lab)), key
        got = b["band_counts"][key]
        assert got.dtype == np.int64 and got.shape == (len(BANDS), 3, 256)
        assert np.array_equal(got, utils.trimap_counts(gt, b[key], BANDS)), key
        assert np.array_equal(got, utils.trimap_counts(truth, lab, BANDS)), key                      # numpy in, the same
        assert np.array_equal(got, band_counts_numpy(truth, lab, dist2_numpy(truth, 3), BANDS, 255)), key
        for j in range(len(BANDS)):
            assert _same(b["band_Mean_IOU"][key][j], utils.mean_iou_from_counts(got[j]))
        assert np.array_equal(utils.trimap_IoU(gt, b[key], BANDS), b["band_Mean_IOU"][key], equal_nan=True)
        c = got[:, :, 3]
        with np.errstate(divide="ignore", invalid="ignore"):
            want = np.float64(c[:, 2]) / np.float64(c[:, 0] + c[:, 1] - c[:, 2])
        assert np.array_equal(utils.trimap_IoU(gt, b[key], BANDS, class_id=3), want, equal_nan=True)
    # ignoring nothing counts the void ring too
    sr = _sr("adam", 6, 5, (16, 16), (64, 64), False)
    res = HotPath(model, sr, mode=mode, th_factor=TH, batch_size=4).run_image_labels(
        img, angles, shifts, REQ, gt_dev=gt, prune=prune, sr_types=("aug",), band_widths=[2], band_ignore_label=None)
    assert sorted(res["band_counts"]) == ["aug", "standard"] and res["band_counts"]["aug"][0, 0, 255] > 0
    assert np.array_equal(res["band_counts"]["aug"], band_counts_numpy(truth, res["aug"].cpu().numpy(), dist2_numpy(truth, 2), [2], -1))


def test_band_counts_when_no_class_is_left(small, dev):
    from asr_amd.pipeline import HotPath
    model, img, _gt_small, angles, shifts = small
    truth, gt = _gt(dev)
    none = [c for c in (5, 12, 17) if c not in _winners(model, img, angles, shifts)]
    assert len(none) >= 2
    sr = _sr("adam", 6, 5, (16, 16), (64, 64), False)
    res = HotPath(model, sr, mode="argmax", th_factor=TH, batch_size=6).run_image_labels(img, angles, shifts, none, gt_dev=gt,
                                                                                       band_widths=BANDS)
    assert res["solved_ids"] == []
    zero = np.zeros((64, 64), np.int32)
    for t in ("aug", "max", "mean"):
        assert int(res[t].abs().sum()) == 0
        assert np.array_equal(res["band_counts"][t], band_counts_numpy(truth, zero, dist2_numpy(truth, 3), BANDS, 255))
    # without a ground truth there is nothing to score, bands or not
    res = HotPath(model, sr, mode="argmax", th_factor=TH, batch_size=6).run_image_labels(img, angles, shifts, none,
                                                                                       band_widths=BANDS)
    assert "band_counts" not in res and "counts" not in res


# ---- scripts/validate_labelmap.py --band_widths ---------------------------------------------------------------------------
N_AUG, ITERS, ANGLE, SHIFT = 8, 10, 0.15, 20
SCRIPT_BANDS = [1, 2, 4, 8, 16, 32]


def _run(cmd):
    """A fresh process under a time limit of its own."""
    r = subprocess.run(["timeout", "-k", "10", "600"] + cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def test_validate_labelmap_script_writes_the_trimap(dev, tmp_path):
    from PIL import Image
    from asr_amd import evaluation as E
    from asr_amd.utils import mean_iou_from_counts
    root = str(tmp_path)
    img_dir, gt_dir = _dataset(root)
    weights = _weights(root, dev)
    args = lambda out, save: [sys.executable, SCRIPT, "--images", img_dir, "--gt", gt_dir, "--num_aug", str(N_AUG), "--num_iter",
                              str(ITERS), "--mode", "argmax", "--angle_max", str(ANGLE), "--shift_max", str(SHIFT),
                              "--th_factor", str(TH), "--weights", weights, "--out", out, "--save_dir", save]
    plain, banded, trimap = os.path.join(root, "plain.csv"), os.path.join(root, "banded.csv"), os.path.join(root, "trimap.csv")
    _run(args(plain, os.path.join(root, "maps0")))
    assert sorted(os.listdir(root)) == sorted(["images", "gt", "weights.npz", "plain.csv", "maps0"])     # no trimap unasked
    save = os.path.join(root, "maps1")
    _run(args(banded, save) + ["--band_widths", ",".join(str(v) for v in SCRIPT_BANDS), "--trimap_out", trimap])
    with open(plain, "rb") as a, open(banded, "rb") as b:
        assert a.read() == b.read()                                           # the flags change no byte of the main CSV
    with open(trimap, newline="") as fh:
        rows = list(csv.reader(fh))
    assert rows[0] == ["Name"] + list(E.TRIMAP_CSV_COLUMNS) + ["band_pixels", "band_share", "n"]
    assert [r[0] for r in rows[1:]] == [f"w={v}" for v in SCRIPT_BANDS]
    # the cells again, from the saved PNGs and the ground-truth PNGs with numpy alone
    gts = [np.asarray(Image.open(os.path.join(gt_dir, f"{g}.png"))).astype(np.int32) for g in range(2)]
    d2s = [dist2_numpy(t, 32) for t in gts]
    for t, d2 in zip(gts, d2s):
        assert_bands_say_something(t, d2, SCRIPT_BANDS)
    counted = sum(int(((t != 255) & (t >= 0) & (t < 256)).sum()) for t in gts)
    for j, key in enumerate(KEYS):
        labs = [np.asarray(Image.open(os.path.join(save, f"{g}_{key}.png"))).astype(np.int32) for g in range(2)]
        per = [band_counts_numpy(gts[g], labs[g], d2s[g], SCRIPT_BANDS, 255) for g in range(2)]
        for b in range(len(SCRIPT_BANDS)):
            r = rows[1 + b]
            assert float(r[1 + 2 * j]) == mean_iou_from_counts(per[0][b] + per[1][b]), (key, b)
            assert float(r[2 + 2 * j]) == float(np.mean([mean_iou_from_counts(per[g][b]) for g in range(2)])), (key, b)
            pixels = int((per[0][b] + per[1][b])[0].sum())
            assert int(r[9]) == pixels and float(r[10]) == pixels / counted and r[11] == "2"
    assert 0.0 < float(rows[1][3]) < 1.0 and float(rows[1][10]) < float(rows[-1][10]) < 0.6
