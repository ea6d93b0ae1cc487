"""The confusion matrix without a GPU: utils.metrics_from_confusion on hand-made matrices with known answers, under both
conventions for the "other" bin; other="label" against mean_iou_from_counts on counts built by numpy from the same maps;
evaluation.write_confusion_csv read back; the constants of the launcher in the header and in _lib; and the argument checks of
ops.confusion_counts, run_image_labels and asr_confusion_counts_i32 that run before anything is launched."""
import csv
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_labelmap_host import counts_numpy

FAKE = C.c_void_p(1 << 20)          # non-null; never dereferenced on the host


def confusion_numpy(truth, pred, num_labels):
    """The definition of include/asr_hip.h restated: bin, then np.add.at over the (truth bin, predicted bin) pairs."""
    L = int(num_labels)
    t = np.asarray(truth).astype(np.int64).reshape(-1)
    p = np.asarray(pred).astype(np.int64).reshape(-1)
    bt = np.where((t >= 0) & (t < L), t, L)
    bp = np.where((p >= 0) & (p < L), p, L)
    m = np.zeros((L + 1, L + 1), np.int64)
    np.add.at(m, (bt, bp), 1)
    return m


def _metrics(m, other):
    from asr_amd.utils import metrics_from_confusion
    return metrics_from_confusion(np.asarray(m, np.int64), other=other)


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


@pytest.mark.parametrize("other", ["ignore", "label"])
def test_a_perfect_prediction_scores_one_everywhere(other):
    r = _metrics([[50, 0, 0, 0], [0, 30, 0, 0], [0, 0, 20, 0], [0, 0, 0, 0]], other)
    for k in ("pixel_accuracy", "mean_accuracy", "Mean_IOU", "fw_iou"):
        assert r[k] == 1.0, k
    for k in ("precision", "recall", "iou"):
        assert r[k].dtype == np.float64 and _same(r[k], [1.0, 1.0, 1.0]), k


@pytest.mark.parametrize("other", ["ignore", "label"])
def test_one_class_entirely_predicted_as_another(other):
    # 60 pixels of label 0 right, all 40 of label 1 predicted as label 2, all 20 of label 2 right
    r = _metrics([[60, 0, 0, 0], [0, 0, 40, 0], [0, 0, 20, 0], [0, 0, 0, 0]], other)
    assert r["pixel_accuracy"] == 80 / 120
    assert _same(r["recall"], [1.0, 0.0, 1.0])
    assert _same(r["precision"], [1.0, np.nan, 20 / 60])            # label 1 is never predicted
    assert _same(r["iou"], [1.0, 0.0, 20 / 60])
    assert r["mean_accuracy"] == float(np.mean([1.0, 0.0, 1.0]))
    assert r["Mean_IOU"] == float(np.mean([1.0, 0.0, 20 / 60]))
    assert r["fw_iou"] == (60 * 1.0 + 40 * 0.0 + 20 * (20 / 60)) / 120


@pytest.mark.parametrize("other", ["ignore", "label"])
def test_a_class_in_neither_map_is_nan_and_leaves_the_means(other):
    r = _metrics([[70, 10, 0, 0], [5, 15, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]], other)
    for k in ("precision", "recall", "iou"):
        assert np.isnan(r[k][2]) and not np.isnan(r[k][:2]).any(), k
    iou = [70 / 85, 15 / 30]
    assert _same(r["iou"][:2], iou)
    assert r["Mean_IOU"] == float(np.mean(iou))
    assert r["mean_accuracy"] == float(np.mean([70 / 80, 15 / 20]))
    assert r["fw_iou"] == (80 * iou[0] + 20 * iou[1]) / 100
    assert r["pixel_accuracy"] == 85 / 100


def test_a_class_predicted_but_absent_from_the_truth_has_iou_zero_and_is_not_in_the_mean():
    """Mean_IOU's rule (utils.mean_iou_from_counts): the mean runs over the labels the truth holds."""
    r = _metrics([[90, 0, 10, 0], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]], "ignore")
    assert _same(r["iou"], [0.9, np.nan, 0.0]) and _same(r["recall"], [0.9, np.nan, np.nan])
    assert r["Mean_IOU"] == 0.9 and r["mean_accuracy"] == 0.9 and r["fw_iou"] == 0.9


def test_void_pixels_under_both_conventions():
    # truth: 50 of label 0, 30 of label 1, 20 void; the void pixels are predicted 12 as label 0 and 8 as label 1; 4 pixels of
    # label 1 are predicted outside the labels
    m = [[45, 5, 0], [6, 20, 4], [12, 8, 0]]
    ig = _metrics(m, "ignore")                      # [[45, 5], [6, 20]] alone
    assert ig["pixel_accuracy"] == 65 / 76
    assert _same(ig["iou"], [45 / 56, 20 / 31]) and ig["Mean_IOU"] == float(np.mean([45 / 56, 20 / 31]))
    assert _same(ig["recall"], [45 / 50, 20 / 26]) and _same(ig["precision"], [45 / 51, 20 / 25])
    assert ig["fw_iou"] == (50 * (45 / 56) + 26 * (20 / 31)) / 76
    lb = _metrics(m, "label")                       # the void pixels enter the unions, the lost pixels the recall
    assert lb["pixel_accuracy"] == 65 / 100
    assert _same(lb["iou"], [45 / (50 + 63 - 45), 20 / (30 + 33 - 20)])
    assert lb["Mean_IOU"] == float(np.mean([45 / 68, 20 / 43]))
    assert _same(lb["recall"], [45 / 50, 20 / 30]) and _same(lb["precision"], [45 / 63, 20 / 33])
    assert lb["mean_accuracy"] == float(np.mean([45 / 50, 20 / 30]))
    assert lb["fw_iou"] == (50 * (45 / 68) + 30 * (20 / 43)) / 80
    # a matrix without other pixels reads the same under both
    clean = [[45, 5, 0], [6, 20, 0], [0, 0, 0]]
    a, b = _metrics(clean, "ignore"), _metrics(clean, "label")
    assert all(_same(a[k], b[k]) for k in a)


@pytest.mark.parametrize("void", [255, -1, 1000], ids=["void 255", "void -1", "void 1000"])
@pytest.mark.parametrize("L", [21, 4])
def test_other_as_a_label_reproduces_mean_iou_from_counts(L, void):
    from asr_amd.utils import mean_iou_from_counts
    rng = np.random.default_rng(L * 7 + (void & 0xFF))
    for case in range(4):
        values = np.array([0, 1, 3, L - 1, void])
        truth = rng.choice(values, (48, 64), p=[0.5, 0.2, 0.1, 0.1, 0.1]).astype(np.int32)
        pred = rng.choice(np.array([0, 1, 2, 3, L - 1]), (48, 64)).astype(np.int32)
        if case == 1:
            pred = truth.copy()                     # void predicted as void: the other bin's diagonal
        if case == 2:
            truth[truth == 3] = 0                   # label 3 only predicted
        if case == 3:
            pred[::5, ::3] = void
        m = confusion_numpy(truth, pred, L)
        assert m.sum() == truth.size
        want = mean_iou_from_counts(counts_numpy(truth, pred))
        assert _metrics(m, "label")["Mean_IOU"] == want, (case, want)
        cc = counts_numpy(truth, pred)              # the identities of include/asr_hip.h
        assert np.array_equal(m.sum(axis=1)[:L], cc[0, :L]) and np.array_equal(m.sum(axis=0)[:L], cc[1, :L])
        assert np.array_equal(np.diagonal(m)[:L], cc[2, :L])


def test_metrics_refuse_what_is_no_confusion_matrix():
    from asr_amd.utils import metrics_from_confusion
    for bad in (np.zeros((3, 4), np.int64), np.zeros((1, 1), np.int64), np.zeros(9, np.int64)):
        with pytest.raises(ValueError):
            metrics_from_confusion(bad)
    with pytest.raises(ValueError):
        metrics_from_confusion(np.zeros((3, 3), np.int64), other="void")
    empty = metrics_from_confusion(np.zeros((3, 3), np.int64))
    assert all(np.isnan(empty[k]) for k in ("pixel_accuracy", "mean_accuracy", "Mean_IOU", "fw_iou"))


def test_confusion_csv_round_trip_and_row_shares(tmp_path):
    from asr_amd.evaluation import (CONFUSION_CSV_COLUMNS, CONFUSION_METRICS_CSV_COLUMNS, write_confusion_csv,
                                    write_confusion_metrics_csv)
    from asr_amd.utils import metrics_from_confusion
    rng = np.random.default_rng(5)
    L = 3
    mats = np.zeros((4, L + 1, L + 1), np.int64)
    mats[0] = rng.integers(1, 1000, (L + 1, L + 1))
    mats[1] = rng.integers(1, 1000, (L + 1, L + 1))
    mats[1, 2] = 0                                   # a label the ground truths do not hold
    mats[3] = rng.integers(1, 10 ** 12, (L + 1, L + 1))      # (max: not produced, all zero)
    path = str(tmp_path / "conf.csv")
    for names, want in ((None, ["0", "1", "2", "other"]), (["bg", "cat", "dog", "spare"], ["bg", "cat", "dog", "other"])):
        write_confusion_csv(path, mats, class_names=names)
        with open(path, newline="") as fh:
            rows = list(csv.reader(fh))
        assert tuple(rows[0]) == CONFUSION_CSV_COLUMNS == ("key", "truth", "predicted", "pixels", "share_of_truth")
        body = rows[1:]
        assert [r[0] for r in body[:: (L + 1) ** 2]] == ["standard", "aug", "mean"] and len(body) == 3 * (L + 1) ** 2
        for key, j in (("standard", 0), ("aug", 1), ("mean", 3)):
            mine = [r for r in body if r[0] == key]
            assert [r[1] for r in mine] == [t for t in want for _ in want] and [r[2] for r in mine] == want * (L + 1)
            back = np.array([int(r[3]) for r in mine], np.int64).reshape(L + 1, L + 1)
            assert np.array_equal(back, mats[j])
            shares = np.array([float(r[4]) for r in mine]).reshape(L + 1, L + 1)
            for i in range(L + 1):
                if mats[j, i].sum():
                    assert abs(shares[i].sum() - 1.0) <= 4 * np.finfo(np.float64).eps * (L + 1), (key, i)
                    assert np.array_equal(shares[i], mats[j, i] / np.float64(mats[j, i].sum()))
                else:
                    assert np.isnan(shares[i]).all()
    # the same file from a dict of the produced maps
    write_confusion_csv(str(tmp_path / "dict.csv"), {"mean": mats[3], "standard": mats[0], "aug": mats[1]}, ["bg", "cat", "dog"])
    with open(path, "rb") as a, open(str(tmp_path / "dict.csv"), "rb") as b:
        assert a.read() == b.read()
    with pytest.raises(ValueError):
        write_confusion_csv(path, mats, class_names=["bg", "cat"])
    # the metrics file: every value of metrics_from_confusion, per key and convention
    mpath = str(tmp_path / "conf_metrics.csv")
    write_confusion_metrics_csv(mpath, mats)
    with open(mpath, newline="") as fh:
        rows = list(csv.reader(fh))
    assert tuple(rows[0]) == CONFUSION_METRICS_CSV_COLUMNS
    got = {(r[0], r[1], r[2], r[3]): float(r[4]) for r in rows[1:]}
    assert len(got) == len(rows) - 1 == 3 * 2 * (4 + 3 * L)
    for key, j in (("standard", 0), ("aug", 1), ("mean", 3)):
        for other in ("ignore", "label"):
            res = metrics_from_confusion(mats[j], other=other)
            for k in ("pixel_accuracy", "mean_accuracy", "Mean_IOU", "fw_iou"):
                assert _same(got[(key, other, k, "")], res[k])
            for k in ("precision", "recall", "iou"):
                assert _same([got[(key, other, k, str(l))] for l in range(L)], res[k])


def test_the_launcher_constants_are_the_headers():
    from asr_amd import _lib
    text = open(os.path.join(ROOT, "include", "asr_hip.h")).read()
    define = lambda name: int(re.search(r"#define\s+" + name + r"\s+(\d+)", text).group(1))
    assert define("ASR_CONFUSION_MAX_LABELS") == _lib.MAX_CONFUSION_LABELS == 64
    assert define("ASR_CONFUSION_MAX_PREDS") == _lib.MAX_CONFUSION_PREDS == 8
    assert define("ASR_CONFUSION_SPAN") == _lib.CONFUSION_SPAN and _lib.CONFUSION_SPAN % 256 == 0
    assert define("ASR_CONFUSION_GRID") == _lib.CONFUSION_GRID


class _Fake:
    """Enough of a tensor for the checks that run before the library is touched."""

    def __init__(self, n):
        self._n = n
        self.device = "nowhere"

    def numel(self):
        return self._n


@pytest.mark.parametrize("bad", [0, 65, -1, 2.5, "21", None, True])
def test_ops_refuses_label_counts_outside_1_to_64(bad):
    from asr_amd import ops
    with pytest.raises(ValueError):
        ops.confusion_counts(_Fake(64), _Fake(64), bad)
    with pytest.raises(ValueError):
        ops.check_confusion_labels(bad)


def test_ops_takes_whole_label_counts_and_refuses_sizes_that_do_not_fit():
    from asr_amd import ops
    from asr_amd._lib import AsrError
    assert [ops.check_confusion_labels(v) for v in (1, 21, 64, 21.0, np.int64(5))] == [1, 21, 64, 21, 5]
    for truth, preds in ((0, 0), (64, 65), (64, 0), (64, 9 * 64)):
        with pytest.raises(AsrError):
            ops.confusion_counts(_Fake(truth), _Fake(preds), 21)


def test_run_image_labels_refuses_a_matrix_without_a_truth_or_with_bad_labels():
    from asr_amd.pipeline import HotPath
    path = HotPath.__new__(HotPath)                  # the checks run before the object is touched
    with pytest.raises(ValueError, match="gt_dev"):
        path.run_image_labels(None, None, None, [3, 8], confusion_labels=21)
    for bad in (0, 65):
        with pytest.raises(ValueError):
            path.run_image_labels(None, None, None, [3, 8], gt_dev=object(), confusion_labels=bad)


def _refused(lib, rc, msg):
    err = lib.asr_last_error()
    assert rc == -1 and err.startswith(b"asr_confusion_counts_i32: ") and msg in err, (rc, err)


def test_the_entry_point_refuses_bad_arguments_before_any_launch(lib):
    call = lambda t, p, c, pixels, n, labels: lib.asr_confusion_counts_i32(t, p, c, pixels, n, labels, None)
    _refused(lib, call(None, FAKE, FAKE, 64, 1, 21), b"null pointer")
    _refused(lib, call(FAKE, None, FAKE, 64, 1, 21), b"null pointer")
    _refused(lib, call(FAKE, FAKE, None, 64, 1, 21), b"null pointer")
    _refused(lib, call(FAKE, FAKE, FAKE, 0, 1, 21), b"bad shape (pixels=0)")
    _refused(lib, call(FAKE, FAKE, FAKE, -5, 1, 21), b"bad shape (pixels=-5)")
    _refused(lib, call(FAKE, FAKE, FAKE, 64, 0, 21), b"0 predictions (1..8)")
    _refused(lib, call(FAKE, FAKE, FAKE, 64, 9, 21), b"9 predictions (1..8)")
    _refused(lib, call(FAKE, FAKE, FAKE, 64, 1, 0), b"0 labels (1..64)")
    _refused(lib, call(FAKE, FAKE, FAKE, 64, 1, 65), b"65 labels (1..64)")
