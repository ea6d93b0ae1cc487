"""Label maps without a GPU: the numpy restatement of the fusion rule (used by the GPU tests too) against answers worked out
by hand, argument validation of the two entry points, the dataset mIoU from summed counts, the CSV writer, and a world-size-2
gloo run of the record gathering that equals the one-rank result row for row."""
import csv
import ctypes as C
import os
import socket

import numpy as np
import torch.multiprocessing as mp

F = np.float32


def fuse_numpy(scores, ids, th_factor=0.15, max_scores=None):
    """The fusion rule, plane by plane in float32: class k passes where its single-class mask is set (S_k > th_factor *
    max(S_k), the f32 product, strict; with max maps S_k >= Smax_k), its rank value is S_k (or the one f32 subtraction
    S_k - Smax_k), the passing class of greatest rank labels the pixel, equal values go to the lowest k (a later class must be
    strictly greater; -0.0 > +0.0 is false), and 0 stays where none passes."""
    s = np.asarray(scores, dtype=F)
    k_set = s.shape[0]
    assert k_set == len(ids)
    label = np.zeros(s.shape[1:], np.int32)
    best = np.zeros(s.shape[1:], F)
    have = np.zeros(s.shape[1:], bool)
    for k in range(k_set):
        if max_scores is None:
            th = F(F(s[k].max()) * F(th_factor))
            passing, rank = s[k] > th, s[k]
        else:
            m = np.asarray(max_scores[k], dtype=F)
            passing, rank = s[k] >= m, (s[k] - m).astype(F)
        take = passing & (~have | (rank > best))
        label[take] = int(ids[k])
        best[take] = rank[take]
        have |= passing
    return label


def masks_numpy(scores, ids, th_factor=0.15, max_scores=None):
    """The K single-class masks (threshold_image per plane)."""
    s = np.asarray(scores, dtype=F)
    out = np.zeros(s.shape, np.int32)
    for k in range(s.shape[0]):
        if max_scores is None:
            on = s[k] > F(F(s[k].max()) * F(th_factor))
        else:
            on = s[k] >= np.asarray(max_scores[k], dtype=F)
        out[k][on] = int(ids[k])
    return out


def counts_numpy(truth, pred):
    """ops.class_counts: [3, 256] = |truth == l|, |pred == l|, both; labels outside 0..255 are not counted."""
    t, p = np.asarray(truth).reshape(-1), np.asarray(pred).reshape(-1)
    c = np.zeros((3, 256), np.int64)
    for l in range(256):
        c[0, l], c[1, l], c[2, l] = (t == l).sum(), (p == l).sum(), ((t == l) & (p == l)).sum()
    return c


# ---- known answers by hand ---------------------------------------------------------------------------------------------
def test_two_passing_classes_the_greater_score_wins():
    #            p0   p1   p2   p3(max of both planes sits here)
    s = np.array([[0.9, 0.2, 0.5, 1.0],
                  [0.4, 0.8, 0.6, 1.0]], F)
    # thresholds 0.5 * 1.0 = 0.5 for both: plane 0 passes at p0, p3; plane 1 at p1, p2, p3
    assert fuse_numpy(s, [3, 7], 0.5).tolist() == [3, 7, 7, 3]                   # p3: 1.0 against 1.0 -> the lowest k
    assert fuse_numpy(s[::-1], [7, 3], 0.5).tolist() == [3, 7, 7, 7]             # the same planes in the other order


def test_ties_go_to_the_lowest_k_and_signed_zeros_tie():
    s = np.array([[2.0, 2.0, 8.0], [2.0, 2.0, 8.0], [2.0, 3.0, 8.0]], F)        # th 0.8 each
    assert fuse_numpy(s, [5, 4, 9], 0.1).tolist() == [5, 9, 5]
    # max-map form: the ranks -0.0 - 0.0 = -0.0 and 0.0 - -0.0 = +0.0 are equal: the lowest k keeps the pixel
    sc = np.array([[-0.0, 1.0], [0.0, 1.0]], F)
    mx = np.array([[0.0, 1.0], [-0.0, 1.0]], F)
    r0, r1 = (sc[0] - mx[0]).astype(F), (sc[1] - mx[1]).astype(F)
    assert np.signbit(r0[0]) and not np.signbit(r1[0]) and r0[0] == r1[0]          # -0.0 against +0.0: equal
    assert fuse_numpy(sc, [2, 1], max_scores=mx).tolist() == [2, 2]
    assert fuse_numpy(sc[::-1], [1, 2], max_scores=mx[::-1]).tolist() == [1, 1]
    # threshold form on a plane of signed zeros: the threshold is 0 and the comparison strict
    z = np.array([[0.0, -0.0, 0.0]], F)
    assert fuse_numpy(z, [6], 0.5).tolist() == [0, 0, 0]                          # 0 > 0 is false whatever the sign


def test_no_class_passes_gives_zero():
    s = np.array([[0.0, 0.0, 4.0], [1.0, 0.0, 10.0]], F)                         # th 2.0 and 5.0
    assert fuse_numpy(s, [1, 2], 0.5).tolist() == [0, 0, 2]
    sc = np.array([[1.0, 5.0]], F)
    mx = np.array([[2.0, 6.0]], F)
    assert fuse_numpy(sc, [4], max_scores=mx).tolist() == [0, 0]


def test_max_map_form_passes_on_equality_and_ranks_by_margin():
    sc = np.array([[3.0, 3.0, 9.0], [5.0, 1.0, 2.0]], F)
    mx = np.array([[3.0, 4.0, 1.0], [4.5, 1.0, 0.5]], F)
    # class 0: passes p0 (3 >= 3, margin 0), p2 (margin 8); class 1: p0 (margin 0.5), p1 (1 >= 1, margin 0), p2 (margin 1.5)
    assert fuse_numpy(sc, [11, 12], max_scores=mx).tolist() == [12, 12, 11]


def test_k1_is_the_single_class_mask():
    rng = np.random.default_rng(0)
    s = rng.standard_normal((1, 7, 9)).astype(F)
    assert np.array_equal(fuse_numpy(s, [8], 0.3), masks_numpy(s, [8], 0.3)[0])
    m = rng.standard_normal((1, 7, 9)).astype(F)
    assert np.array_equal(fuse_numpy(s, [8], max_scores=m), masks_numpy(s, [8], max_scores=m)[0])


def test_contract_against_the_masks_on_random_planes():
    rng = np.random.default_rng(1)
    vals = np.array([0.0, -0.0, 0.5, 1.0], F)
    for with_max in (False, True):
        s = vals[rng.integers(0, 4, (5, 400))]
        m = vals[rng.integers(0, 4, (5, 400))] if with_max else None
        ids = [9, 2, 14, 1, 20]
        lab = fuse_numpy(s, ids, 0.4, m)
        masks = masks_numpy(s, ids, 0.4, m)
        for k, c in enumerate(ids):
            assert (masks[k][lab == c] == c).all()
        assert np.array_equal(lab == 0, (masks == 0).all(axis=0))


# ---- argument validation needs no GPU ----------------------------------------------------------------------------------
def _ids(*v):
    return (C.c_int * max(len(v), 1))(*v)


def test_fuse_labels_rejects_bad_arguments_before_any_launch(lib):
    fake = C.c_void_p(1 << 20)                                          # non-null; never dereferenced on the host
    args = lambda scores, labels, ids, k: (scores, None, fake, None, labels, None, 64, k, 0.15, ids, 21, None)
    assert lib.asr_fuse_labels_f32(*args(None, fake, _ids(1, 2), 2)) == -1 and b"null pointer" in lib.asr_last_error()
    assert lib.asr_fuse_labels_f32(*args(fake, None, _ids(1, 2), 2)) == -1 and b"null pointer" in lib.asr_last_error()
    assert lib.asr_fuse_labels_f32(*args(fake, fake, None, 2)) == -1 and b"null class id array" in lib.asr_last_error()
    assert lib.asr_fuse_labels_f32(*args(fake, fake, _ids(1), 0)) == -1 and b"0 class ids" in lib.asr_last_error()
    assert lib.asr_fuse_labels_f32(*args(fake, fake, _ids(*range(1, 34)), 33)) == -1 and b"33 class ids" in lib.asr_last_error()
    assert lib.asr_fuse_labels_f32(*args(fake, fake, _ids(3, 5, 3), 3)) == -1 and b"given twice" in lib.asr_last_error()
    assert lib.asr_fuse_labels_f32(*args(fake, fake, _ids(3, 0), 2)) == -1 and b"fallback label" in lib.asr_last_error()
    assert lib.asr_fuse_labels_f32(*args(fake, fake, _ids(3, 21), 2)) == -1 and b"out of range" in lib.asr_last_error()
    # truth without counts (and the reverse), a missing extrema workspace
    assert lib.asr_fuse_labels_f32(fake, None, fake, fake, fake, None, 64, 1, 0.15, _ids(1), 21, None) == -1
    assert b"truth and counts" in lib.asr_last_error()
    assert lib.asr_fuse_labels_f32(fake, None, None, None, fake, None, 64, 1, 0.15, _ids(1), 21, None) == -1
    assert b"minmax workspace" in lib.asr_last_error()


def test_standard_labels_rejects_bad_arguments_before_any_launch(lib):
    fake = C.c_void_p(1 << 20)
    call = lambda logits, labels, ids, k: lib.asr_standard_labels_i32(logits, labels, 8, 8, 21, 32, 32, ids, k, None)
    assert call(None, fake, _ids(1), 1) == -1 and b"null pointer" in lib.asr_last_error()
    assert call(fake, fake, None, 1) == -1 and b"null class id array" in lib.asr_last_error()
    assert call(fake, fake, _ids(1), 0) == -1 and b"0 class ids" in lib.asr_last_error()
    assert call(fake, fake, _ids(*range(1, 34)), 33) == -1 and b"33 class ids" in lib.asr_last_error()
    assert call(fake, fake, _ids(4, 4), 2) == -1 and b"given twice" in lib.asr_last_error()
    assert call(fake, fake, _ids(0, 4), 2) == -1 and b"fallback label" in lib.asr_last_error()


def test_run_image_labels_refuses_class_zero():
    import pytest
    from asr_amd.pipeline import HotPath
    with pytest.raises(ValueError):
        HotPath(None, None).run_image_labels(None, [], [], class_ids=[0, 3])
    with pytest.raises(ValueError, match="sr_types"):
        HotPath(None, None).run_image_labels(None, [], [], class_ids=[3], sr_types=("aug", "median"))
    with pytest.raises(ValueError, match="no label map"):
        HotPath(None, None).run_image_labels(None, [], [], class_ids=[3], sr_types=(), want_standard=False)


# ---- dataset mIoU, CSV ------------------------------------------------------------------------------------------------
def _counts(rng, labels, pixels=1000):
    t = rng.choice(labels + [255], pixels)
    p = rng.choice(labels, pixels)
    return counts_numpy(t, p)


def _counts_per_key(rng, labels, pixels=1000):
    """[4, 3, 256]: four predictions scored against ONE ground truth, as the four label maps of an image are."""
    t = rng.choice(labels + [255], pixels)
    return np.stack([counts_numpy(t, rng.choice(labels, pixels)) for _ in range(4)])


def test_dataset_miou_comes_from_the_summed_counts():
    from asr_amd import evaluation as E
    from asr_amd.utils import mean_iou_from_counts
    rng = np.random.default_rng(2)
    a, b = _counts(rng, [0, 3, 8]), _counts(rng, [0, 8, 15])
    total = a + b
    # by hand: per-label IoU from the summed counts, mean over the labels the ground truths hold, 255 removed
    ious = [total[2, l] / (total[0, l] + total[1, l] - total[2, l]) for l in (0, 3, 8, 15)]
    assert E.dataset_miou(total) == float(np.mean(ious)) == mean_iou_from_counts(total)
    assert E.dataset_miou(total) != np.mean([mean_iou_from_counts(a), mean_iou_from_counts(b)])     # two conventions
    assert np.isnan(E.dataset_miou(np.zeros((3, 256), np.int64)))
    iou = E.label_ious(total)
    assert sorted(iou) == [0, 3, 8, 15] and iou[3] == ious[1]


def test_labelmap_csv_layout(tmp_path):
    from asr_amd import evaluation as E
    rng = np.random.default_rng(3)
    counts = _counts_per_key(rng, [0, 3, 8])
    rows = np.array([[0.5, 0.25, 0.125, 1.0], [0.25, 0.75, 0.375, 0.5]])
    path = str(tmp_path / "lm.csv")
    E.write_labelmap_csv(path, counts, rows)
    with open(path, newline="") as fh:
        got = list(csv.reader(fh))
    assert got[0] == ["Name", "standard_iou", "aug_iou", "max_iou", "mean_iou", "n"]
    assert [r[0] for r in got[1:]] == ["Label 0", "Label 3", "Label 8", "dataset_mIoU", "mean_image_mIoU"]
    for j in range(4):
        assert float(got[2][1 + j]) == E.label_ious(counts[j])[3]
        assert float(got[4][1 + j]) == E.dataset_miou(counts[j])
        assert float(got[5][1 + j]) == float(np.mean(rows[:, j]))
    assert int(got[2][5]) == int(counts[0][0, 3]) and got[5][5] == "2"


def test_labelmap_csv_marks_a_label_map_that_was_not_produced(tmp_path):
    """evaluate_labelmaps leaves all-zero counts and NaN rows for an SR type that was not asked for: its column is nan."""
    from asr_amd import evaluation as E
    rng = np.random.default_rng(4)
    counts = _counts_per_key(rng, [0, 3, 8])
    counts[0] = 0                                                                           # no standard label map
    counts[2] = 0                                                                           # no max label map
    rows = np.array([[np.nan, 0.25, np.nan, 1.0]])
    path = str(tmp_path / "lm.csv")
    E.write_labelmap_csv(path, counts, rows)
    with open(path, newline="") as fh:
        got = list(csv.reader(fh))
    assert [r[0] for r in got[1:]] == ["Label 0", "Label 3", "Label 8", "dataset_mIoU", "mean_image_mIoU"]
    for r in got[1:]:
        assert np.isnan(float(r[1])) and np.isnan(float(r[3])) and not np.isnan(float(r[2])) and not np.isnan(float(r[4]))
    assert int(got[2][5]) == int(counts[1][0, 3])


# ---- two gloo ranks gather what one rank computes ----------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _record(g):
    rng = np.random.default_rng(100 + g)
    counts = np.stack([_counts(rng, [0, 1 + g % 3, 8]) for _ in range(4)])
    miou = np.array([g + 0.25, g + 0.5, np.nan if g == 2 else g + 0.75, g + 1.0]) / 10.0
    return miou, counts


def _worker(rank, world, port, num_images, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import torch.distributed
    from asr_amd import distributed as D, evaluation as E
    if world > 1:
        D.init_from_env(backend="gloo")
    mine = D.shard_indices(num_images, rank, world)
    recs = [_record(g) for g in mine]
    fields = E.label_fields(E.LABELMAP_KEYS)
    rows, total = E.gather_labelmap_records(mine, fields, {fields[0]: ([r[0] for r in recs], [r[1] for r in recs])}, num_images)
    q.put((rank, rows, total))
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


def _run(world, num_images):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, num_images, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=180) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return res


def test_two_rank_gather_equals_one_rank():
    num_images = 5                                      # ragged: rank 0 owns 3 images, rank 1 owns 2
    two, one = _run(2, num_images), _run(1, num_images)
    exp_rows = np.stack([_record(g)[0] for g in range(num_images)])
    exp_total = sum(_record(g)[1] for g in range(num_images))
    for _rank, rows, total in two + one:
        np.testing.assert_array_equal(rows, exp_rows)                 # row for row, the NaN included
        assert total.dtype == np.int64 and np.array_equal(total, exp_total)
