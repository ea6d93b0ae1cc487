"""The label-map threshold sweep without a GPU: the numpy restatement of asr_fuse_labels_sweep_counts_f32 (used by the GPU tests
too) against a case worked out by hand in which a pixel goes from one class to another and then to 0 as the factor rises,
argument validation of the entry point, its workspace formula, the CSV writer of the curve, and a world-size-2 gloo run of the
record gathering with sweep records that equals the one-rank result."""
import csv
import ctypes as C
import os

import numpy as np
import pytest
import torch.multiprocessing as mp

from test_labelmap_host import _counts_per_key, _free_port, _ids, counts_numpy, fuse_numpy

F = np.float32
FACTORS_17 = [round(v, 2) for v in np.arange(0.1, 0.95, step=0.05)]             # threshold_tests.py's 0.10 ... 0.90


def sweep_numpy(scores, ids, truth, factors):
    """[T, 3, 256]: the counts of the fused label map of every factor, each factor rounded to f32 as the device array is."""
    return np.stack([counts_numpy(truth, fuse_numpy(scores, ids, F(f))) for f in factors])


# ---- known answer by hand ----------------------------------------------------------------------------------------------
def test_a_pixel_goes_from_class_a_to_class_b_to_zero_as_the_factor_rises():
    #             p0    p1    p2(max of A)  p3(max of B)
    s = np.array([[0.40, 0.05, 1.0, 0.0],           # class A = 4, maximum 1.0: threshold f
                  [0.30, 0.20, 0.0, 0.5]], F)       # class B = 9, maximum 0.5: threshold f / 2
    ids, truth = [4, 9], np.array([9, 9, 4, 0], np.int32)
    # f = 0.25: th 0.25 / 0.125.  p0: both pass, A's 0.40 > B's 0.30 -> 4.  p1: only B (0.20 > 0.125) -> 9.  p2 -> 4.  p3 -> 9
    # f = 0.5 : th 0.5  / 0.25.   p0: A fails (0.40 <= 0.5), B passes (0.30 > 0.25) -> 9.  p1: none -> 0.  p2 -> 4.  p3 -> 9
    # f = 0.75: th 0.75 / 0.375.  p0: none -> 0.  p1 -> 0.  p2 -> 4.  p3 (0.5 > 0.375) -> 9
    # f = 1.0 : nothing exceeds its own maximum -> all 0
    maps = [fuse_numpy(s, ids, F(f)).tolist() for f in (0.25, 0.5, 0.75, 1.0)]
    assert maps == [[4, 9, 4, 9], [9, 0, 4, 9], [0, 0, 4, 9], [0, 0, 0, 0]]
    got = sweep_numpy(s, ids, truth, [0.25, 0.5, 0.75, 1.0])
    assert got.shape == (4, 3, 256)
    for j in range(4):
        assert got[j, 0, 0] == 1 and got[j, 0, 4] == 1 and got[j, 0, 9] == 2 and got[j, 0].sum() == 4     # the truth, every row
    pred = lambda j: {l: int(got[j, 1, l]) for l in (0, 4, 9)}
    both = lambda j: {l: int(got[j, 2, l]) for l in (0, 4, 9)}
    assert pred(0) == {0: 0, 4: 2, 9: 2} and both(0) == {0: 0, 4: 1, 9: 1}
    assert pred(1) == {0: 1, 4: 1, 9: 2} and both(1) == {0: 0, 4: 1, 9: 1}
    assert pred(2) == {0: 2, 4: 1, 9: 1} and both(2) == {0: 0, 4: 1, 9: 0}
    assert pred(3) == {0: 4, 4: 0, 9: 0} and both(3) == {0: 1, 4: 0, 9: 0}
    # the order of the factors is the order of the rows, repeats included
    again = sweep_numpy(s, ids, truth, [1.0, 0.25, 0.25])
    assert np.array_equal(again, got[[3, 0, 0]])


# ---- argument validation needs no GPU ----------------------------------------------------------------------------------
def test_sweep_rejects_bad_arguments_before_any_launch(lib):
    fake = C.c_void_p(1 << 20)                                          # non-null, 8-byte aligned; never dereferenced on the host
    ws = lib.asr_fuse_labels_sweep_workspace_bytes(2, 17)
    fn = lib.asr_fuse_labels_sweep_counts_f32
    call = lambda scores=fake, truth=fake, factors=fake, work=fake, ws_bytes=ws, counts=fake, k=2, t=17, ids=_ids(1, 2): fn(
        scores, truth, factors, work, ws_bytes, counts, 64, k, t, ids, 21, None)
    assert call(t=0) == -1 and b"0 threshold factors (1..64)" in lib.asr_last_error()
    assert call(t=65, ws_bytes=1 << 20) == -1 and b"65 threshold factors (1..64)" in lib.asr_last_error()
    for name in ("scores", "truth", "factors", "work", "counts"):
        assert call(**{name: None}) == -1 and b"asr_fuse_labels_sweep_counts_f32: null pointer" in lib.asr_last_error(), name
    assert call(ids=None) == -1 and b"null class id array" in lib.asr_last_error()
    assert call(ws_bytes=ws - 1) == -4 and b"workspace of" in lib.asr_last_error()
    assert lib.asr_threshold_sweep_iou_counts_f32(fake, fake, fake, fake, 8, fake, 100, 1, 17, 1, 8, 0, None) == -4     # the same code
    assert call(ids=_ids(3, 5, 3), k=3) == -1 and b"given twice" in lib.asr_last_error()
    assert call(ids=_ids(3, 0)) == -1 and b"fallback label" in lib.asr_last_error()
    assert call(ids=_ids(3, 21)) == -1 and b"out of range" in lib.asr_last_error()
    assert call(ids=_ids(1), k=0) == -1 and b"0 class ids" in lib.asr_last_error()
    assert call(ids=_ids(*range(1, 34)), k=33) == -1 and b"33 class ids" in lib.asr_last_error()
    assert fn(fake, fake, fake, fake, ws, fake, 0, 2, 17, _ids(1, 2), 21, None) == -1 and b"bad shape" in lib.asr_last_error()


def test_sweep_workspace_bytes_is_the_formula_of_the_header(lib):
    fn = lib.asr_fuse_labels_sweep_workspace_bytes
    for k, t in [(1, 1), (3, 17), (32, 64)]:
        assert fn(k, t) == 8 * (t * 2 * (k + 1) + 256) + 8 * k, (k, t)
    assert fn(0, 17) == 0 and fn(-1, 17) == 0 and fn(3, 0) == 0 and fn(3, -2) == 0


def test_python_surface_names():
    from asr_amd import ops, utils
    assert ops.MAX_LABEL_SWEEP_FACTORS == 64
    assert callable(ops.fuse_labels_sweep_counts) and callable(utils.labelmap_threshold_sweep)
    assert callable(utils.labelmap_threshold_mIoU)


def test_run_image_labels_refuses_a_sweep_it_cannot_make():
    from asr_amd.pipeline import HotPath
    with pytest.raises(ValueError, match="gt_dev"):
        HotPath(None, None).run_image_labels(None, [], [], class_ids=[3], th_factors=[0.2])
    with pytest.raises(ValueError, match="plays no part"):
        HotPath(None, None, mode="slice_max").run_image_labels(None, [], [], class_ids=[3], gt_dev=object(), th_factors=[0.2])
    with pytest.raises(ValueError, match="65 threshold factors"):
        HotPath(None, None).run_image_labels(None, [], [], class_ids=[3], gt_dev=object(), th_factors=[0.2] * 65)


# ---- the CSV of the curve -----------------------------------------------------------------------------------------------
def test_threshold_csv_layout(tmp_path):
    from asr_amd import evaluation as E
    rng = np.random.default_rng(11)
    counts = _counts_per_key(rng, [0, 3, 8])
    rows = np.array([[0.5, 0.25, 0.125, 1.0], [0.25, 0.75, 0.375, 0.5]])
    factors = [0.1, 0.65, 0.3]
    sweep_counts = np.stack([np.stack([_counts_per_key(rng, [0, 3, 8])[0] for _ in factors]) for _ in range(3)])
    sweep_counts[:, 1] = counts[1:]                                     # factor 0.65 is the run's own: its counts are `counts`
    sweep_rows = rng.random((2, 3, 3))
    sweep_rows[:, :, 1] = rows[:, 1:]
    path, plain = str(tmp_path / "th.csv"), str(tmp_path / "lm.csv")
    E.write_labelmap_threshold_csv(path, factors, sweep_counts, sweep_rows, counts, rows)
    E.write_labelmap_csv(plain, counts, rows)
    with open(path, newline="") as fh:
        raw = fh.read()
    got = list(csv.reader(raw.splitlines()))
    assert got[0] == ["th_factor", "aug_dataset_mIoU", "aug_mean_image_mIoU", "max_dataset_mIoU", "max_mean_image_mIoU",
                      "mean_dataset_mIoU", "mean_mean_image_mIoU", "standard_dataset_mIoU", "standard_mean_image_mIoU"]
    assert raw.splitlines()[0].startswith('"th_factor","aug_dataset_mIoU"')                     # QUOTE_ALL
    assert len(got) == 1 + len(factors) and [r[0] for r in got[1:]] == ["0.1", "0.65", "0.3"]
    for j, r in enumerate(got[1:]):
        assert r[7] == repr(E.dataset_miou(counts[0])) and r[8] == repr(float(np.mean(rows[:, 0])))      # constant columns
        for i in range(3):
            assert r[1 + 2 * i] == repr(E.dataset_miou(sweep_counts[i, j]))
            assert r[2 + 2 * i] == repr(float(np.mean(sweep_rows[:, i, j])))
    with open(plain, newline="") as fh:
        lm = {r[0]: r for r in csv.reader(fh)}
    own = got[2]
    assert [own[1], own[3], own[5], own[7]] == [lm["dataset_mIoU"][k] for k in (2, 3, 4, 1)]           # the same digits
    assert [own[2], own[4], own[6], own[8]] == [lm["mean_image_mIoU"][k] for k in (2, 3, 4, 1)]
    best = E.best_threshold_factors(factors, sweep_counts)
    for i, key in enumerate(("aug", "max", "mean")):
        curve = [E.dataset_miou(c) for c in sweep_counts[i]]
        assert best[key] == (factors[int(np.argmax(curve))], max(curve))


def test_threshold_csv_marks_what_was_not_produced(tmp_path):
    from asr_amd import evaluation as E
    rng = np.random.default_rng(12)
    counts = _counts_per_key(rng, [0, 3, 8])
    counts[0] = 0                                                       # no standard label map
    sweep_counts = np.stack([np.stack([_counts_per_key(rng, [0, 3, 8])[0] for _ in range(2)]) for _ in range(3)])
    sweep_counts[1] = 0                                                 # no max label map
    path = str(tmp_path / "th.csv")
    E.write_labelmap_threshold_csv(path, [0.2, 0.4], sweep_counts, np.full((1, 3, 2), 0.5), counts, np.full((1, 4), 0.5))
    with open(path, newline="") as fh:
        got = list(csv.reader(fh))
    for r in got[1:]:
        assert [r[3], r[4], r[7], r[8]] == ["nan"] * 4 and "nan" not in (r[1], r[2], r[5], r[6])
    assert sorted(E.best_threshold_factors([0.2, 0.4], sweep_counts)) == ["aug", "mean"]


# ---- two gloo ranks gather what one rank computes ----------------------------------------------------------------------
T, B, L = 3, 2, 4


def _record(g):
    rng = np.random.default_rng(300 + g)
    return dict(miou=np.array([g + 0.25, g + 0.5, np.nan if g == 2 else g + 0.75, g + 1.0]) / 10.0,
                counts=rng.integers(0, 1000, (4, 3, 256)),
                band_miou=rng.random((4, B)), band_counts=rng.integers(0, 1000, (4, B, 3, 256)),
                confusion=rng.integers(0, 1000, (4, L + 1, L + 1)),
                sweep_miou=np.where(rng.random((3, T)) < 0.2, np.nan, rng.random((3, T))),
                sweep_counts=rng.integers(0, 1000, (3, T, 3, 256)))


def _gather(E, mine, recs, num_images, everything):
    col = lambda key: [r[key] for r in recs]
    fields = E.label_fields(E.LABELMAP_KEYS, n_bands=B if everything else 0, n_conf=L if everything else 0, n_factors=T)
    local = {"": (col("miou"), col("counts")), "band_": (col("band_miou"), col("band_counts")),
             "confusion": (None, col("confusion")), "sweep_": (col("sweep_miou"), col("sweep_counts"))}
    return E.gather_labelmap_records(mine, fields, {f: local[f.prefix] for f in fields}, num_images)


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
    q.put((rank, _gather(E, mine, recs, num_images, False), _gather(E, mine, recs, num_images, True)))
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


def test_two_rank_gather_of_sweep_records_equals_one_rank():
    num_images = 5                                      # ragged: rank 0 owns 3 images, rank 1 owns 2
    two, one = _run(2, num_images), _run(1, num_images)
    recs = [_record(g) for g in range(num_images)]
    stack = lambda key: np.stack([r[key] for r in recs])
    total = lambda key: sum(r[key] for r in recs)
    for _rank, plain, full in two + one:
        assert len(plain) == 4 and len(full) == 7
        # (rows, counts[, band_rows, band_counts][, confusion], sweep_rows, sweep_counts)
        for out in (plain, full):
            np.testing.assert_array_equal(out[0], stack("miou"))
            assert out[1].dtype == np.int64 and np.array_equal(out[1], total("counts"))
            assert out[-2].shape == (num_images, 3, T)
            np.testing.assert_array_equal(out[-2], stack("sweep_miou"))             # row for row, the NaNs included
            assert out[-1].dtype == np.int64 and out[-1].shape == (3, T, 3, 256)
            assert np.array_equal(out[-1], total("sweep_counts"))
        np.testing.assert_array_equal(full[2], stack("band_miou"))
        assert np.array_equal(full[3], total("band_counts"))
        assert full[4].shape == (4, L + 1, L + 1) and np.array_equal(full[4], total("confusion"))
