"""Host side of the risk-coverage curve (asr_binned_class_counts_f32, utils.coverage_edges, HotPath.run_image_labels'
coverages, evaluation.write_coverage_csv): what is decided before any launch, and the parts that are plain tensor or numpy
arithmetic.  No GPU is needed."""
import csv
import inspect

import numpy as np
import pytest
import torch

ERR_INVALID = -1
FAKE = 1 << 20                    # non-null and aligned; never dereferenced on the host


def _binned(lib, truth=FAKE, preds=FAKE, u=FAKE, edges=FAKE, counts=FAKE, pixels=100, num_preds=4, num_bins=5, ignore=255):
    return lib.asr_binned_class_counts_f32(truth, preds, u, edges, counts, pixels, num_preds, num_bins, ignore, None)


def test_argument_validation_needs_no_gpu(lib):
    for name in ("truth", "preds", "u", "edges", "counts"):
        assert _binned(lib, **{name: None}) == ERR_INVALID and b"null pointer" in lib.asr_last_error(), name
    for pixels in (0, -1, -(1 << 40)):
        assert _binned(lib, pixels=pixels) == ERR_INVALID and b"bad shape" in lib.asr_last_error(), pixels
    for p in (0, 9, -1):
        assert _binned(lib, num_preds=p) == ERR_INVALID and b"predictions (1..8)" in lib.asr_last_error(), p
    for b in (0, 17, -1):
        assert _binned(lib, num_bins=b) == ERR_INVALID and b"bins (1..16)" in lib.asr_last_error(), b


def test_check_coverages():
    from asr_amd import ops
    assert ops.MAX_COVERAGE_BINS == 16
    assert ops.check_coverages([50, 60, 100]) == [50, 60, 100]
    assert ops.check_coverages((100, 1, 50, 50)) == [100, 1, 50, 50]                 # any order, repeats allowed
    assert ops.check_coverages(np.array([10, 20])) == [10, 20] and ops.check_coverages([50.0]) == [50]
    assert ops.check_coverages(range(1, 17)) == list(range(1, 17))
    for bad in ([], [0], [101], [-5], [50.5], [50, "60"], "50,60", None, 50, [True], list(range(1, 18)), [float("nan")],
                [float("inf")], [[50]]):
        with pytest.raises(ValueError):
            ops.check_coverages(bad)


def _edges_numpy(u, truth, percents, ignore):
    u = np.asarray(u, np.float32).reshape(-1)
    t = np.asarray(truth).reshape(-1)
    counted = np.ones(t.shape, bool) if ignore in (None, -1) else t != ignore
    m = int(counted.sum())
    s = np.sort(u[counted])
    return np.array([s[(p * m + 99) // 100 - 1] if m else np.inf for p in percents], np.float32)


def test_coverage_edges_against_numpy():
    from asr_amd import utils
    rng = np.random.default_rng(3)
    percents = [50, 75, 100, 1, 99, 50]
    for pixels in (1, 2, 7, 100, 1001):
        truth = rng.choice(np.array([0, 3, 20, 255], np.int32), pixels)
        for kind in ("distinct", "ties", "inf"):
            if kind == "distinct":
                u = rng.permutation(pixels).astype(np.float32)
            elif kind == "ties":                          # heavy ties at 0 and a few other plateaus
                u = rng.choice(np.array([0.0, 0.0, 0.0, 0.25, 0.5], np.float32), pixels)
            else:
                u = np.where(rng.uniform(size=pixels) < 0.5, np.float32(np.inf), rng.uniform(size=pixels).astype(np.float32))
            for ignore in (255, -1, None, 3):
                got = utils.coverage_edges(torch.as_tensor(u), torch.as_tensor(truth), percents, ignore_label=ignore)
                assert got.dtype == torch.float32 and tuple(got.shape) == (len(percents),)
                want = _edges_numpy(u, truth, percents, ignore)
                assert np.array_equal(got.numpy(), want), (pixels, kind, ignore, got, want)
                # ties stay in: the share retained is at least p %, and dropping the edge's own plateau would fall below it
                kept = utils.coverage_retained(torch.as_tensor(u), torch.as_tensor(truth), got, ignore_label=ignore).numpy()
                m = kept[-1]
                for j, p in enumerate(percents):
                    assert 100 * kept[j] >= p * m
                    counted = np.ones(pixels, bool) if ignore in (None, -1) else truth != ignore
                    assert 100 * int((counted & (u < want[j])).sum()) < p * m or m == 0
    # a [H, W] map and a numpy ground truth of as many pixels
    got = utils.coverage_edges(torch.arange(12, dtype=torch.float32).view(3, 4), np.zeros((3, 4), np.int32), [50])
    assert got.tolist() == [5.0]
    with pytest.raises(ValueError):
        utils.coverage_edges(torch.zeros(5), torch.zeros(4, dtype=torch.int32), [50])
    with pytest.raises(ValueError):
        utils.coverage_edges(torch.zeros(5), torch.zeros(5, dtype=torch.int32), [0])


def test_coverage_edges_nothing_counted():
    from asr_amd import utils
    u = torch.tensor([0.5, 0.25, 1.0])
    void = torch.full((3,), 255, dtype=torch.int32)
    got = utils.coverage_edges(u, void, [1, 50, 100])
    assert torch.isinf(got).all() and (got > 0).all()
    assert utils.coverage_retained(u, void, got).tolist() == [0, 0, 0, 0]


def test_uncertainty_map_on_host_tensors():
    from asr_amd import utils
    var = torch.tensor([[[0.0, 4.0], [1.0, 9.0]], [[2.0, 2.0], [0.5, 0.0]]])
    nv = torch.tensor([[[5.0, 2.0], [1.0, 3.0]], [[5.0, 2.0], [4.0, 0.0]]])
    got = utils.uncertainty_map(var, nv, [2.0, 1.0])
    inf = float("inf")
    assert got.dtype == torch.float32 and got.tolist() == [[2.0, 2.0], [inf, inf]]
    assert utils.uncertainty_map(var[:1], nv[:1], [1.0]).tolist() == [[0.0, 4.0], [inf, 9.0]]
    assert utils.opm_scales([3, 15], "argmax", normalised=False) == [3.0, 15.0]
    for mode in ("argmax", "slice", "slice_max"):
        assert utils.opm_scales([3, 15], mode) == [1.0, 1.0]
    assert utils.opm_scales([3, 15], "slice", normalised=False) == [1.0, 1.0]
    for bad in ([1.0], [1.0, 0.0], [1.0, float("nan")], [1.0, 2.0, 3.0]):
        with pytest.raises(ValueError):
            utils.uncertainty_map(var, nv, bad)
    with pytest.raises(ValueError):
        utils.uncertainty_map(var, nv[:1], [1.0, 1.0])


def test_run_image_labels_refuses_before_the_model():
    from asr_amd.pipeline import HotPath
    params = inspect.signature(HotPath.run_image_labels).parameters
    assert params["coverages"].default is None and params["keep_uncertainty"].default is False
    path = HotPath(model=None, superresolution=None, mode="argmax")
    with pytest.raises(ValueError, match="gt_dev"):
        path.run_image_labels(None, None, None, class_ids=[1, 2], gt_dev=None, coverages=(50, 75, 100))
    for bad in ((), (0,), (50.5,), tuple(range(1, 18))):
        with pytest.raises(ValueError):
            path.run_image_labels(None, None, None, class_ids=[1, 2], gt_dev=torch.zeros((4, 4), dtype=torch.int32), coverages=bad)
    with pytest.raises(ValueError, match="keep_uncertainty"):
        path.run_image_labels(None, None, None, class_ids=[1, 2], gt_dev=None, keep_uncertainty=True)


def test_evaluate_labelmaps_keywords():
    from asr_amd import evaluation as E
    params = inspect.signature(E.evaluate_labelmaps).parameters
    assert params["coverages"].default is None and params["uncertainty_dir"].default is None
    assert list(params)[-2:] == ["coverages", "uncertainty_dir"]


def test_gather_appends_the_coverage_records_last():
    from asr_amd import evaluation as E
    rng = np.random.default_rng(0)
    n, C, T = 3, 2, 2
    miou = rng.uniform(size=(n, 4))
    counts = rng.integers(0, 100, (n, 4, 3, 256))
    sweep_m, sweep_c = rng.uniform(size=(n, 3, T)), rng.integers(0, 100, (n, 3, T, 3, 256))
    cov_m, cov_c = rng.uniform(size=(n, 4, C)), rng.integers(0, 100, (n, 4, C, 3, 256))
    local = {"": (miou, counts), "sweep_": (sweep_m, sweep_c), "coverage_": (cov_m, cov_c)}
    gather = lambda fields: E.gather_labelmap_records(list(range(n)), fields, {f: local[f.prefix] for f in fields}, n)
    plain = gather(E.label_fields(E.LABELMAP_KEYS, n_factors=T))
    out = gather(E.label_fields(E.LABELMAP_KEYS, n_factors=T, n_cov=C))
    assert len(plain) == 4 and len(out) == 6
    for a, b in zip(plain, out[:4]):
        assert np.array_equal(a, b)
    assert out[4].shape == (n, 4, C) and np.array_equal(out[4], cov_m)
    assert out[5].shape == (4, C, 3, 256) and out[5].dtype == np.int64 and np.array_equal(out[5], cov_c.sum(axis=0))


def test_write_coverage_csv(tmp_path):
    from asr_amd import evaluation as E
    from asr_amd.utils import mean_iou_from_counts
    assert E.COVERAGE_CSV_COLUMNS == tuple(f"{k}_{c}" for k in ("standard", "aug", "max", "mean")
                                           for c in ("dataset_mIoU", "mean_image_mIoU", "retained_share"))
    percents = [50, 100]
    cov = np.zeros((4, 2, 3, 256), np.int64)
    # standard: at 50 % label 0 keeps 40 truth / 40 predicted / 40 both, label 1 keeps 10 / 20 / 5; at 100 % everything
    cov[0, 0, :, 0], cov[0, 0, :, 1] = (40, 40, 40), (10, 20, 5)
    cov[0, 1, :, 0], cov[0, 1, :, 1] = (60, 50, 45), (40, 50, 30)
    cov[1] = cov[0]
    cov[1, 0, 2, 1] = 10                                 # aug: label 1 fully right at 50 %
    rows = np.full((2, 4, 2), np.nan)                    # max / mean were not produced
    rows[:, 0] = [[0.9, 0.7], [0.7, 0.5]]
    rows[:, 1] = [[1.0, 0.7], [0.8, 0.5]]
    whole = np.zeros((4, 3, 256), np.int64)
    whole[:2, 0, 0], whole[:2, 0, 1], whole[:2, 0, 255] = 60, 40, 25          # 25 void pixels never count
    path = tmp_path / "cov.csv"
    E.write_coverage_csv(str(path), percents, cov, rows, counts=whole)
    with open(path, newline="") as fh:
        table = list(csv.reader(fh))
    assert tuple(table[0]) == ("coverage",) + E.COVERAGE_CSV_COLUMNS + ("n",) and len(table) == 3
    r50, r100 = dict(zip(table[0], table[1])), dict(zip(table[0], table[2]))
    assert r50["coverage"] == "50" and r100["coverage"] == "100" and r50["n"] == "2"
    assert float(r50["standard_dataset_mIoU"]) == mean_iou_from_counts(cov[0, 0]) == (1.0 + 5 / 25) / 2
    assert float(r100["standard_dataset_mIoU"]) == (45 / 65 + 30 / 60) / 2
    assert float(r50["aug_dataset_mIoU"]) == (1.0 + 10 / 20) / 2
    assert float(r50["standard_mean_image_mIoU"]) == np.mean([0.9, 0.7]) and float(r100["aug_mean_image_mIoU"]) == np.mean([0.7, 0.5])
    assert float(r50["standard_retained_share"]) == 0.5 and float(r100["aug_retained_share"]) == 1.0
    for key in ("max", "mean"):
        for col in ("dataset_mIoU", "mean_image_mIoU", "retained_share"):
            assert r50[f"{key}_{col}"] == "nan" and r100[f"{key}_{col}"] == "nan"
    # without the whole-image counts the 100 % row is the denominator; without either the share is nan
    E.write_coverage_csv(str(path), percents, cov, rows)
    with open(path, newline="") as fh:
        table = list(csv.reader(fh))
    assert float(dict(zip(table[0], table[1]))["standard_retained_share"]) == 0.5
    E.write_coverage_csv(str(path), [50], cov[:, :1], rows[:, :, :1])
    with open(path, newline="") as fh:
        table = list(csv.reader(fh))
    assert dict(zip(table[0], table[1]))["standard_retained_share"] == "nan" and len(table) == 2
    with pytest.raises(ValueError):
        E.write_coverage_csv(str(path), [0], cov[:, :1], rows[:, :, :1])
