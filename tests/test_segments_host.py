"""The "segments" rule of include/asr_hip.h on the host: the numpy restatement (tests/segments_ref.py) against a brute-force form
and hand-drawn cases, the derived metrics, the option checks, the record layout, the CSV and the library's refusals.  No GPU."""
import csv
import inspect

import numpy as np
import pytest

import segments_ref as S
from segments_cases import CASES, ONE, expected


def test_the_restatement_equals_the_brute_force_form_on_random_maps():
    rng = np.random.default_rng(11)
    matched = 0
    for k in range(120):
        L, c, zero = (1, 3, 21)[k % 3], (4, 8)[k % 2], k % 5 == 0
        truth = rng.choice(np.array([0, 1, 2, 255, -3], np.int32), size=(12, 12), p=[0.3, 0.3, 0.3, 0.05, 0.05])
        pred = truth.copy()
        flip = rng.random((12, 12)) < (0.05, 0.15, 0.4)[k % 3]
        pred[flip] = rng.choice(np.array([0, 1, 2, 40], np.int32), size=int(flip.sum()))
        counts, pred_match, truth_match = S.segment_match(truth, pred, L, c, zero)
        brute, most = S.brute_force(truth, pred, L, c, zero)
        assert counts.dtype == np.int64 and counts.shape == (L, 4) and counts.tolist() == brute, k
        assert most <= 1, k                                          # never two matches for one segment
        matched += int(counts[:, 0].sum())
        # the planes say the same as the counts: matched roots pair up, -1 marks the FPs and FNs
        v0 = 0 if zero else 1
        flat_p, flat_t = pred_match.ravel(), truth_match.ravel()
        for p in np.unique(flat_t[flat_t >= 0]).tolist():           # p: a matched predicted root; its pixels name the truth root
            g = int(flat_p[p])
            assert g >= 0 and flat_t[g] == p and truth.ravel()[g] == pred.ravel()[p] >= v0
        assert np.all(flat_t[~((truth.ravel() >= v0) & (truth.ravel() < L))] == -2)
        assert np.all(flat_p[~((pred.ravel() >= v0) & (pred.ravel() < L))] == -2)
    assert matched > 100


@pytest.mark.parametrize("case", CASES, ids=[k[0] for k in CASES])
def test_the_hand_drawn_cases(case):
    _, truth, pred, L, c, zero, _ = case
    counts, pred_match, truth_match = S.segment_match(truth, pred, L, c, zero)
    assert np.array_equal(counts, expected(case))
    assert S.brute_force(truth, pred, L, c, zero)[0] == expected(case).tolist()
    assert pred_match.shape == truth_match.shape == truth.shape and pred_match.dtype == truth_match.dtype == np.int32


def test_the_planes_of_the_void_cases():
    by = {k[0].split(":")[0]: k for k in CASES}
    under = by["a predicted segment wholly under void is dropped"]
    _, pm, tm = S.segment_match(*under[1:6])
    assert pm.tolist() == [[-2, -2, -2, -2]] and tm.tolist() == [[-2, -2, -2, -2]]
    stripe = by["a predicted segment crossing a void stripe stays one, A_p without the stripe"]
    _, pm, tm = S.segment_match(*stripe[1:6])
    assert pm.tolist() == [[2, 2, 2, 2]]                             # the stripe's pixel belongs to the matched segment too
    assert tm.tolist() == [[-1, -2, 0, 0]]


def test_metrics_from_segments():
    from asr_amd.utils import metrics_from_segments
    counts = np.zeros((5, 4), np.int64)
    counts[1] = (3, 1, 0, 2 * ONE + ONE // 2)                        # SQ 2.5 / 3, RQ 3 / 3.5
    counts[2] = (0, 2, 1, 0)                                         # segments and no match: RQ = PQ = 0, SQ NaN
    counts[4] = (2, 0, 2, 2 * ONE)                                   # SQ 1, RQ 2 / 3
    m = metrics_from_segments(counts)
    assert sorted(m) == sorted(["PQ", "SQ", "RQ", "precision", "recall", "mean_PQ", "mean_SQ", "mean_RQ"])
    for name in ("PQ", "SQ", "RQ", "precision", "recall"):
        assert m[name].shape == (5,) and m[name].dtype == np.float64
        assert np.isnan(m[name][0]) and np.isnan(m[name][3])        # no segment of the label anywhere: every denominator is 0
    assert m["RQ"][1] == 3 / 3.5 and m["SQ"][1] == 2.5 / 3 and m["PQ"][1] == 2.5 / 3.5
    assert m["precision"][1] == 0.75 and m["recall"][1] == 1.0
    assert m["RQ"][2] == 0.0 and np.isnan(m["SQ"][2]) and m["PQ"][2] == 0.0 and m["precision"][2] == 0.0 and m["recall"][2] == 0.0
    assert m["SQ"][4] == 1.0 and m["RQ"][4] == 2 / 3 and m["PQ"][4] == 2 / 3 and m["precision"][4] == 1.0 and m["recall"][4] == 0.5
    assert m["mean_RQ"] == np.mean([3 / 3.5, 0.0, 2 / 3]) and m["mean_PQ"] == np.mean([2.5 / 3.5, 0.0, 2 / 3])
    assert m["mean_SQ"] == np.mean([2.5 / 3, 1.0])
    none = metrics_from_segments(np.zeros((3, 4), np.int64))
    assert all(np.isnan(none[k]) for k in ("mean_PQ", "mean_SQ", "mean_RQ")) and np.isnan(none["PQ"]).all()
    for bad in (np.zeros((4,)), np.zeros((3, 3)), np.zeros((2, 3, 4))):
        with pytest.raises(ValueError):
            metrics_from_segments(bad)
    # the hand-drawn match of 2 pixels inside 3: SQ is the IoU 2 / 3 to within 2^-30
    m = metrics_from_segments(expected(CASES[2]))
    assert abs(m["SQ"][1] - 2 / 3) < 2.0 ** -30 and m["RQ"][1] == 1.0


def test_check_segments():
    from asr_amd.ops import check_segments
    assert check_segments(21) == (21, 8, False) and check_segments((5, 4)) == (5, 4, False)
    assert check_segments([64, 8, True]) == (64, 8, True) and check_segments((1, 4, 0)) == (1, 4, False)
    assert check_segments(np.int64(3)) == (3, 8, False) and check_segments(4.0) == (4, 8, False) and check_segments((7,)) == (7, 8, False)
    for bad in (0, -3, 65, 2.5, "5", None, True, (), (5, 8, True, 1), (5, 6), (5, 0), (0, 4), (2.5, 4), (5, "8"), (5, None),
                (5, 8, 2), (5, 8, "yes"), (5, 8, None), (5, 8, 0.5)):
        with pytest.raises(ValueError):
            check_segments(bad)


def test_label_fields_with_segments_appends_after_everything():
    from asr_amd.label_record import Field, label_fields, label_layout
    keys = ("standard", "aug", "max", "mean")
    assert list(inspect.signature(label_fields).parameters) == ["keys", "n_bands", "n_conf", "n_factors", "n_cov", "n_regions",
                                                                "n_segments"]
    assert label_fields(keys, 2, 3, 0, 4, 1) == label_fields(keys, 2, 3, 0, 4, 1, 0) == label_fields(keys, 2, 3, 0, 4, 1, n_segments=0)
    for before in ((0, 0, 0, 0, 0), (2, 21, 0, 3, 0), (0, 0, 0, 0, 1), (2, 21, 0, 3, 1)):
        plain = label_fields(keys, *before)
        fields = label_fields(keys, *before, n_segments=21)
        new = (Field("segments", keys, (21, 4), False),) + ((Field("raw_segments", keys, (21, 4), False),) if before[4] else ())
        assert fields[:len(plain)] == plain and fields[len(plain):] == new
        for with_miou in (True, False):
            spans0, end0 = label_layout(plain, with_miou)
            spans, end = label_layout(fields, with_miou)
            assert spans[:len(plain)] == spans0                                    # every earlier span is where it was
            assert spans[len(plain)] == (None, slice(end0, end0 + 4 * 84)) and end == end0 + len(new) * 4 * 84
            assert spans[-1] == (None, slice(end - 4 * 84, end))


def test_label_options_with_segments():
    from asr_amd.pipeline import HotPath, LabelOptions
    path = HotPath(None, None, mode="argmax")
    assert LabelOptions._fields[-1] == "segments" and LabelOptions._fields[-2] == "min_region"
    off = path.label_options(None, True, band_widths=(1, 2))
    assert off.segments is None and off.sizes == (2, 0, 0, 0, 0)
    on = path.label_options(None, True, segments=21)
    assert on.segments == (21, 8, False) and on.sizes == (0, 0, 0, 0, 0) and len(on.sizes) == 5
    both = path.label_options(None, True, min_region=(3, 4), segments=(5, 4, True))
    assert both.segments == (5, 4, True) and both.min_region == (3, 4) and both.sizes == (0, 0, 0, 0, 1)
    with pytest.raises(ValueError, match="segments needs gt_dev"):
        path.label_options(None, False, segments=21)
    with pytest.raises(ValueError, match="th_factors with segments"):
        path.label_options(None, True, th_factors=[0.1, 0.2], segments=21)
    for bad in (0, 65, (21, 5), 1.5):
        with pytest.raises(ValueError):
            path.label_options(None, True, segments=bad)
    # refused before the model: HotPath(None, None) has none
    with pytest.raises(ValueError, match="gt_dev"):
        path.run_image_labels(None, None, None, class_ids=[1, 2], gt_dev=None, segments=21)


def test_the_signature_positions():
    from asr_amd import evaluation as E
    from asr_amd import ops, utils
    from asr_amd.pipeline import HotPath
    params = list(inspect.signature(E.evaluate_labelmaps).parameters)
    assert params[-3:] == ["segments", "coverages", "uncertainty_dir"] and params[-4] == "min_region"
    assert inspect.signature(E.evaluate_labelmaps).parameters["segments"].default is None
    assert list(inspect.signature(HotPath.run_image_labels).parameters)[-1] == "segments"
    assert list(inspect.signature(HotPath.label_options).parameters)[-1] == "segments"
    assert inspect.signature(HotPath.run_image_labels).parameters["segments"].default is None
    assert list(inspect.signature(ops.segment_match).parameters) == [
        "truth", "preds", "num_labels", "connectivity", "include_zero", "truth_regions", "pred_regions", "want_planes", "out"]
    assert [p.default for p in inspect.signature(ops.segment_match).parameters.values()][2:] == [21, 8, False, None, None, False, None]
    assert list(inspect.signature(utils.segment_counts).parameters) == ["truth", "pred", "num_labels", "connectivity", "include_zero"]
    assert list(inspect.signature(E.write_segments_csv).parameters) == ["path", "segments", "raw_segments", "class_names"]


def test_labelmap_scores_name_the_new_entries():
    from asr_amd import evaluation as E
    n, rng = 3, np.random.default_rng(2)

    def gather(fields):
        local = {}
        for f in fields:
            hi = ONE * 1000 if f.prefix.endswith("segments") else 1000               # Q sums are large and must stay exact
            counts = rng.integers(0, hi, size=(n, len(f.keys)) + f.shape)
            local[f] = (rng.random((n, len(f.keys)) + f.shape[:-2]) if f.scored else None, counts)
        return E.gather_labelmap_records(list(range(n)), fields, local, n), local

    fields = E.label_fields(E.LABELMAP_KEYS, n_conf=2, n_segments=21)
    out, local = gather(fields)
    assert len(out) == 4 and out.segments is out[3] and out.raw_segments is None and out.regions is None and out.confusion is out[2]
    assert out.segments.shape == (4, 21, 4) and out.segments.dtype == np.int64
    assert np.array_equal(out.segments, local[fields[-1]][1].sum(axis=0))
    fields = E.label_fields(E.LABELMAP_KEYS, n_regions=1, n_segments=5)
    out, local = gather(fields)
    assert len(out) == 7 and out.regions is out[4] and out.segments is out[5] and out.raw_segments is out[6]
    assert np.array_equal(out.segments, local[fields[-2]][1].sum(axis=0))
    assert np.array_equal(out.raw_segments, local[fields[-1]][1].sum(axis=0)) and out.raw_segments.shape == (4, 5, 4)
    assert E.LabelmapScores().segments is None and E.LabelmapScores().raw_segments is None


def test_write_segments_csv(tmp_path):
    from asr_amd import evaluation as E
    seg, raw = np.zeros((4, 3, 4), np.int64), np.zeros((4, 3, 4), np.int64)
    raw[1, 1], raw[1, 2] = (2, 2, 0, ONE + ONE // 2), (0, 1, 1, 0)                    # "aug" before the clean-up
    seg[1, 1], seg[1, 2] = (2, 0, 0, ONE + ONE // 2), (0, 0, 1, 0)                    # ... and after: the three FPs are gone
    seg[0, 1] = raw[0, 1] = (1, 0, 1, ONE // 4)                                       # "standard": unchanged; max, mean: not produced
    path = str(tmp_path / "seg.csv")
    E.write_segments_csv(path, seg, raw, ["bg", "cat", "dog"])
    assert open(path).read().splitlines()[0] == ",".join(f'"{c}"' for c in E.SEGMENTS_CSV_COLUMNS)    # every cell quoted
    with open(path, newline="") as fh:
        got = list(csv.reader(fh))
    assert got[0] == ["key", "stage", "label", "TP", "FP", "FN", "precision", "recall", "SQ", "RQ", "PQ"]
    nan = repr(float("nan"))
    std = ["cat", "1", "0", "1", repr(1.0), repr(0.5), repr(0.25), repr(1 / 1.5), repr(0.25 / 1.5)]
    std_mean = ["mean", "1", "0", "1", "", "", repr(0.25), repr(1 / 1.5), repr(0.25 / 1.5)]
    assert got[1:5] == [["standard", "raw"] + std, ["standard", "raw"] + std_mean, ["standard", "final"] + std,
                        ["standard", "final"] + std_mean]
    assert got[5] == ["aug", "raw", "cat", "2", "2", "0", repr(0.5), repr(1.0), repr(0.75), repr(2 / 3), repr(0.5)]
    assert got[6] == ["aug", "raw", "dog", "0", "1", "1", repr(0.0), repr(0.0), nan, repr(0.0), repr(0.0)]
    assert got[7] == ["aug", "raw", "mean", "2", "3", "1", "", "", repr(0.75), repr(1 / 3), repr(0.25)]
    assert got[8] == ["aug", "final", "cat", "2", "0", "0", repr(1.0), repr(1.0), repr(0.75), repr(1.0), repr(0.75)]
    assert got[9] == ["aug", "final", "dog", "0", "0", "1", nan, repr(0.0), nan, repr(0.0), repr(0.0)]
    assert got[10] == ["aug", "final", "mean", "2", "0", "1", "", "", repr(0.75), repr(0.5), repr(0.375)]
    empty = ["mean", "0", "0", "0", "", "", nan, nan, nan]
    assert got[11:] == [[key, stage] + empty for key in ("max", "mean") for stage in ("raw", "final")]
    # without the raw stage and without names: "final" rows alone, labels by number
    E.write_segments_csv(path, seg)
    with open(path, newline="") as fh:
        got = list(csv.reader(fh))
    assert [r[:3] for r in got[1:]] == [["standard", "final", "1"], ["standard", "final", "mean"], ["aug", "final", "1"],
                                        ["aug", "final", "2"], ["aug", "final", "mean"], ["max", "final", "mean"],
                                        ["mean", "final", "mean"]]
    with pytest.raises(ValueError):
        E.write_segments_csv(path, seg, class_names=["bg", "cat"])


def test_the_library_refuses_bad_arguments_before_any_launch(lib):
    from asr_amd import _lib
    header = open(__import__("os").path.join(__import__("conftest").ROOT, "include", "asr_hip.h")).read()
    assert "#define ASR_SEGMENTS_MAX_LABELS 64\n" in header and "#define ASR_SEGMENTS_IOU_ONE (1 << 30)\n" in header
    assert (_lib.MAX_SEGMENT_LABELS, _lib.SEGMENTS_IOU_ONE) == (64, ONE) and S.IOU_ONE == ONE
    assert lib.asr_abi_version() == 3
    fake, big = 1 << 20, 1 << 40                               # non-null, aligned; never dereferenced on the host
    INVALID, WORKSPACE = -1, -4

    def match(truth=fake, truth_root=fake, truth_area=fake, preds=fake, pred_root=fake, counts=fake, pred_match=None,
              truth_match=None, ws=fake, ws_bytes=big, maps=1, h=8, w=8, labels=21, zero=0):
        return lib.asr_segment_match_i32(truth, truth_root, truth_area, preds, pred_root, counts, pred_match, truth_match, ws,
                                         ws_bytes, maps, h, w, labels, zero, None)

    for name in ("truth", "truth_root", "truth_area", "preds", "pred_root", "counts", "ws"):
        assert match(**{name: None}) == INVALID and b"null pointer" in lib.asr_last_error()
    for labels in (0, -1, 65, 256):
        assert match(labels=labels) == INVALID and b"labels" in lib.asr_last_error()
    for kw in (dict(h=0), dict(w=0), dict(h=-1), dict(w=-5)):
        assert match(**kw) == INVALID and b"bad shape" in lib.asr_last_error()
    assert match(h=1 << 16, w=1 << 15) == INVALID and b"2^31 - 1" in lib.asr_last_error()          # h*w = 2^31
    assert match(h=46341, w=46341) == INVALID                                                       # just above
    for maps in (0, -1, 65536):
        assert match(maps=maps) == INVALID and b"maps" in lib.asr_last_error()
    need = lib.asr_segment_match_workspace_bytes(2, 8, 9)
    assert need >= 2 * (12 * 2 * 72 + 12 * 72)
    assert match(maps=2, h=8, w=9, ws_bytes=need - 1) == WORKSPACE and b"workspace" in lib.asr_last_error()


def test_the_workspace_size_is_host_arithmetic(lib):
    fn = lib.asr_segment_match_workspace_bytes
    for bad in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (1, -4, 4), (1, 4, -4)):
        assert fn(*bad) == 0
    assert fn(1, 1, 1) == 12 * 2 + 12 and fn(1, 32, 32) == 12 * 2048 + 12 * 1024 and fn(3, 32, 32) == 3 * fn(1, 32, 32)
    # the table: a power of two of at least 2 h w slots, so that no input can fill it
    for h, w in ((5, 7), (163, 167), (512, 512), (46340, 46340)):
        slots = (fn(1, h, w) - 12 * h * w) // 12
        assert slots & (slots - 1) == 0 and 2 * h * w <= slots < 4 * h * w, (h, w)
    assert fn(65535, 46340, 46340) > 1 << 50                       # size_t arithmetic


def test_the_product_refuses_cpu_tensors(lib):
    import torch
    from asr_amd import _lib, ops
    m = torch.zeros((4, 4), dtype=torch.int32)
    with pytest.raises(_lib.AsrError):
        ops.segment_match(m, m)
    with pytest.raises(ValueError):
        ops.segment_match(m, m, 0)
