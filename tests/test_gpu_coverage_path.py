"""HotPath.run_image_labels(coverages=...) on the small model input of tests/test_gpu_labelmap_path.py: the uncertainty map
is utils.uncertainty_map of ops.realign_moments on the stacks the solver read, the coverage counts are ops.class_counts over
each label map's most certain non-void pixels, nothing the call returned before moves by a bit; evaluate_labelmaps sums the
images' records; and scripts/validate_labelmap.py --coverages writes the curve and leaves its other CSV byte for byte."""
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

COVS = (50, 75, 100)
KEYS = ("standard", "aug", "max", "mean")


@pytest.fixture(scope="module")
def small(dev):
    model, img, gt, angles, shifts = small_inputs(dev)
    gt = gt.clone()
    gt[:3, 10:40] = 255                      # a void strip: never counted, never among the retained pixels
    return model, img, gt, angles, shifts


def _labels(small, mode="argmax", ids=REQ, **kw):
    from asr_amd.pipeline import HotPath
    model, img, gt, angles, shifts = small
    sr = _sr("adam", 6, 5, (16, 16), (64, 64), False)
    path = HotPath(model, sr, mode=mode, th_factor=TH, batch_size=4)
    res = path.run_image_labels(img, angles, shifts, ids, gt_dev=gt, adam_starts={c: 3 * j for j, c in enumerate(ids)}, **kw)
    return res, path


def _same(a, b, what):
    if isinstance(a, torch.Tensor):
        assert torch.equal(a, b), what
    elif isinstance(a, dict):
        assert sorted(a) == sorted(b), what
        for k in a:
            _same(a[k], b[k], (what, k))
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, (what, i))
    elif a is None:
        assert b is None, what
    else:
        assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), what


NEW = {"coverage_counts", "coverage_Mean_IOU", "coverage_share", "uncertainty", "uncertainty_stacks"}


@pytest.mark.parametrize("mode", ["argmax", "slice", "slice_max"])
def test_the_curve_of_one_image(small, mode):
    from asr_amd import ops, utils
    model, img, gt, angles, shifts = small
    extra = dict(band_widths=(2, 4), confusion_labels=21, keep_scores=True)
    if mode != "slice_max":
        extra["th_factors"] = (0.1, 0.3)
    ref, _ = _labels(small, mode, **extra)
    res, path = _labels(small, mode, coverages=COVS, keep_uncertainty=True, **extra)
    # every key the call returned before is bitwise what it was
    assert set(res) - NEW == set(ref) and NEW <= set(res)
    for key in ref:
        _same(res[key], ref[key], key)
    truth = path._gt_int32(gt).reshape(-1)
    keep = truth != 255
    assert 0 < int((~keep).sum()) < truth.numel()
    # u is the rule applied to the moments of the stacks the solver read, frame coverage, valid_min 0.5
    y = res["uncertainty_stacks"]
    k = len(res["solved_ids"])
    assert k >= 2 and tuple(y.shape) == (k, len(angles), 16, 16)
    a = np.repeat(np.asarray(angles, np.float32)[None], k, axis=0)
    s = np.repeat(np.asarray(shifts, np.float32)[None], k, axis=0)
    rot, tr = path.sr._transforms(a, s, y.device, negate=True)
    mom = ops.realign_moments(y, tr, rot, (64, 64), want=("var", "nv"), wgt=torch.ones((16, 16), device=y.device), valid_min=0.5)
    u = utils.uncertainty_map(mom["var"], mom["nv"], utils.opm_scales(res["solved_ids"], mode))
    assert res["uncertainty"].dtype == torch.float32 and tuple(res["uncertainty"].shape) == (64, 64)
    assert torch.equal(res["uncertainty"], u)
    finite = torch.isfinite(u)
    assert finite.any() and (u[finite] > 0).any() and (u[finite] >= 0).all()
    if mode == "argmax":                     # normalised two-valued stacks: a variance over the copies is at most 1 / 4
        assert float(u[finite].max()) <= 0.25
    by_max = torch.stack([mom["var"][j] for j in range(k)]).amax(dim=0)
    assert torch.equal(u[finite], by_max[finite]) and (mom["nv"][:, ~finite] < 2).any(dim=0).all()
    # the counts: ops.class_counts over the retained non-void pixels, the 100 % row over all of them
    edges = utils.coverage_edges(u, truth, COVS)
    assert sorted(res["coverage_counts"]) == sorted(KEYS)
    share = res["coverage_share"]
    assert share.shape == (3,) and (share >= np.array(COVS) / 100).all() and share[2] == 1.0 and share[0] < 1.0
    for key in KEYS:
        c = res["coverage_counts"][key]
        assert c.shape == (3, 3, 256) and c.dtype == np.int64
        flat = res[key].reshape(-1)
        for b in range(3):
            held = keep & (u.reshape(-1) <= edges[b])
            want = ops.class_counts(truth[held].contiguous(), flat[held].contiguous())[0].cpu().numpy()
            assert np.array_equal(c[b], want), (key, b)
            assert int(c[b, 0].sum()) == int(held.sum()) == round(share[b] * int(keep.sum()))
        whole = res["counts"][key].copy()
        assert np.array_equal(c[2, 0, :255], whole[0, :255]) and c[2, 0, 255] == 0 and whole[0, 255] == int((~keep).sum())
        assert (np.diff(c, axis=0) >= 0).all()                                    # nested: c0, c1, c2 never fall as p grows
        m = res["coverage_Mean_IOU"][key]
        assert m.shape == (3,) and m.dtype == np.float64
        for b in range(3):
            w = utils.mean_iou_from_counts(c[b])
            assert m[b] == w or (np.isnan(m[b]) and np.isnan(w))
        assert np.array_equal(utils.risk_coverage_counts(gt, res[key], u, COVS), c), key


def test_a_subset_of_the_maps_and_no_class_left(small):
    from asr_amd import ops
    model, img, gt, angles, shifts = small
    res, _ = _labels(small, coverages=(100, 50), sr_types=("mean",), want_standard=False)
    assert sorted(res["coverage_counts"]) == ["mean"] and "uncertainty" not in res
    c = res["coverage_counts"]["mean"]
    assert (c[0] >= c[1]).all() and np.array_equal(c[0, 0, :255], res["counts"]["mean"][0, :255])       # the caller's order
    # classes that never win: nothing is solved, u is +inf everywhere, every percentage retains every non-void pixel
    from test_gpu_labelmap_path import _winners
    none = [cid for cid in (5, 12, 17) if cid not in _winners(model, img, angles, shifts)]
    assert len(none) >= 2
    res, _ = _labels(small, ids=none, coverages=COVS, keep_uncertainty=True)
    assert res["solved_ids"] == [] and res["uncertainty_stacks"] is None and torch.isinf(res["uncertainty"]).all()
    assert (res["coverage_share"] == 1.0).all()
    truth = gt.to(torch.int32).reshape(-1)
    keep = truth != 255
    for key in KEYS:
        want = ops.class_counts(truth[keep].contiguous(), res[key].reshape(-1)[keep].contiguous())[0].cpu().numpy()
        for b in range(3):
            assert np.array_equal(res["coverage_counts"][key][b], want), (key, b)


def test_evaluate_labelmaps_sums_the_images_records(small, tmp_path):
    from PIL import Image
    from bench import synth_image
    from asr_amd.evaluation import evaluate_labelmaps, write_coverage_csv
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
    run = lambda **kw: evaluate_labelmaps(
        HotPath(model, _sr("adam", 6, 5, (16, 16), (64, 64), False), mode="argmax", th_factor=TH, batch_size=4), images, gts,
        REQ, num_aug=6, angle_max=0.15, shift_max=8, img_size=(64, 64), **kw)
    ref = run(th_factors=(0.2, 0.4))
    udir = tmp_path / "u"
    out = run(th_factors=(0.2, 0.4), coverages=COVS, uncertainty_dir=str(udir))
    assert len(ref) == 4 and len(out) == 6
    for a, b in zip(ref, out[:4]):
        assert np.array_equal(a, b, equal_nan=True)
    cov_rows, cov_counts = out[4], out[5]
    assert cov_rows.shape == (2, 4, 3) and cov_counts.shape == (4, 3, 3, 256) and cov_counts.dtype == np.int64
    assert np.array_equal(cov_counts[:, 2, 0, :255], out[1][:, 0, :255])            # the 100 % rows: every non-void pixel
    assert (np.diff(cov_counts, axis=1) >= 0).all() and np.isfinite(cov_rows[:, :, 2]).all()
    for g in range(2):
        sd = np.load(udir / f"{g}.npy")
        assert sd.shape == (64, 64) and sd.dtype == np.float32 and (sd[np.isfinite(sd)] <= 0.5).all() and (sd > 0).any()
    path = tmp_path / "cov.csv"
    write_coverage_csv(str(path), COVS, cov_counts, cov_rows, counts=out[1])
    with open(path, newline="") as fh:
        table = list(csv.reader(fh))
    assert [r[0] for r in table[1:]] == ["50", "75", "100"]
    head = table[0]
    for r, p in zip(table[1:], COVS):
        for key in KEYS:
            assert float(r[head.index(f"{key}_retained_share")]) >= p / 100
        assert float(table[3][head.index("aug_retained_share")]) == 1.0


def test_the_script_writes_the_curve_and_leaves_its_csv_alone(dev, tmp_path):
    root = str(tmp_path)
    img_dir, gt_dir = _dataset(root)
    weights = _weights(root, dev)
    args = lambda out: [sys.executable, SCRIPT, "--images", img_dir, "--gt", gt_dir, "--num_samples", "1", "--num_aug", str(N_AUG),
                        "--num_iter", str(ITERS), "--mode", "argmax", "--angle_max", str(ANGLE), "--shift_max", str(SHIFT),
                        "--th_factor", str(TH), "--weights", weights, "--out", out]
    plain, with_cov = os.path.join(root, "plain.csv"), os.path.join(root, "cov", "run.csv")
    _run(args(plain))
    _run(args(with_cov) + ["--coverages", "50,75,100", "--uncertainty_dir", os.path.join(root, "u")])
    with open(plain, "rb") as a, open(with_cov, "rb") as b:
        assert a.read() == b.read()
    assert not os.path.exists(os.path.join(root, "plain_coverage.csv"))
    with open(os.path.join(root, "cov", "run_coverage.csv"), newline="") as fh:
        rows = list(csv.reader(fh))
    assert rows[0] == ["coverage"] + [f"{k}_{c}" for k in KEYS for c in ("dataset_mIoU", "mean_image_mIoU", "retained_share")] + ["n"]
    assert [r[0] for r in rows[1:]] == ["50", "75", "100"] and all(r[-1] == "1" for r in rows[1:])
    for key in KEYS:
        col = rows[0].index(f"{key}_retained_share")
        assert [float(r[col]) >= p / 100 for r, p in zip(rows[1:], (50, 75, 100))] == [True] * 3 and float(rows[3][col]) == 1.0
        for r in rows[1:]:
            assert 0.0 <= float(r[rows[0].index(f"{key}_dataset_mIoU")]) <= 1.0
    sd = np.load(os.path.join(root, "u", "0.npy"))
    assert sd.shape == (512, 512) and sd.dtype == np.float32 and (sd > 0).any()
