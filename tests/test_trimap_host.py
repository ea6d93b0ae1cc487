"""The trimap (label maps scored inside bands round the ground truth's label boundaries) without a GPU: the numpy restatement of
the definitions in include/asr_hip.h (used by the GPU tests too) against scipy's Euclidean distance transform and against
answers worked out by hand, the CSV writer, and the argument refusals that need no GPU.  Everything is integer: every
comparison is exact."""
import csv
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_labelmap_host import counts_numpy

NONE = 0xFFFF


def boundary_numpy(truth):
    """bool [H, W]: the pixel has a 4-neighbour inside the image with a different value (255 is a value like any other)."""
    t = np.asarray(truth)
    b = np.zeros(t.shape, bool)
    b[1:] |= t[1:] != t[:-1]
    b[:-1] |= t[:-1] != t[1:]
    b[:, 1:] |= t[:, 1:] != t[:, :-1]
    b[:, :-1] |= t[:, :-1] != t[:, 1:]
    return b


def dist2_numpy(truth, r_max):
    """uint16 [H, W]: the squared distance to the nearest boundary pixel where it is <= r_max^2, else 0xFFFF.  Two integer
    passes: each row's distance to the nearest boundary pixel of that row, then the minimum over the rows within r_max of
    dx^2 + dy^2 (a boundary pixel within r_max lies at most r_max rows away, so nothing within r_max is missed)."""
    b = boundary_numpy(truth)
    h, w = b.shape
    far = 1 << 20
    idx = np.arange(w, dtype=np.int64)[None, :]
    left = np.maximum.accumulate(np.where(b, idx, -far), axis=1)
    right = np.minimum.accumulate(np.where(b, idx, far)[:, ::-1], axis=1)[:, ::-1]
    dx = np.minimum(idx - left, right - idx)
    best = np.full((h, w), far * far, np.int64)
    for dy in range(-r_max, r_max + 1):
        lo, hi = max(0, -dy), min(h, h - dy)                      # rows y with y + dy inside the image
        if lo < hi:
            best[lo:hi] = np.minimum(best[lo:hi], dx[lo + dy:hi + dy] ** 2 + dy * dy)
    return np.where(best <= r_max * r_max, best, NONE).astype(np.uint16)


def dist2_scipy(truth, r_max):
    """The oracle: scipy's exact Euclidean distance transform of the boundary mask, squared, clipped like the entry point."""
    from scipy.ndimage import distance_transform_edt
    b = boundary_numpy(truth)
    if not b.any():
        return np.full(b.shape, NONE, np.uint16)
    sq = distance_transform_edt(~b) ** 2
    d2 = np.rint(sq)
    assert np.abs(sq - d2).max() < 1e-6                           # squared distances on the grid are integers
    return np.where(d2 <= r_max * r_max, d2, NONE).astype(np.uint16)


def band_counts_numpy(truth, pred, dist2, widths, ignore_label=255):
    """int64 [B, 3, 256]: counts_numpy over the pixels with dist2 <= width^2 whose truth is not ignore_label (-1: none)."""
    t, p, d = np.asarray(truth).reshape(-1), np.asarray(pred).reshape(-1), np.asarray(dist2).reshape(-1).astype(np.int64)
    out = np.zeros((len(widths), 3, 256), np.int64)
    for b, width in enumerate(widths):
        sel = (d <= int(width) ** 2) & (t != ignore_label)
        out[b] = counts_numpy(t[sel], p[sel])
    return out


def band_share(dist2, width):
    return float((np.asarray(dist2).astype(np.int64) <= int(width) ** 2).mean())


def assert_bands_say_something(truth, dist2, widths, ignore_label=255):
    """A band test proves nothing if its bands are empty or hold everything: the narrowest requested band holds at least 1 %
    and the widest at most 60 % of the pixels, and at least two labels besides void have counted pixels in the narrowest."""
    lo, hi = min(widths), max(widths)
    assert band_share(dist2, lo) >= 0.01, band_share(dist2, lo)
    assert band_share(dist2, hi) <= 0.60, band_share(dist2, hi)
    t = np.asarray(truth)
    sel = (np.asarray(dist2).astype(np.int64) <= lo * lo) & (t != ignore_label)
    held = [int(l) for l in np.unique(t[sel]) if l != 255]
    assert len(held) >= 2, held


def blob_map(seed, h, w, labels=(3, 8, 15, 12), ring=2):
    """A synthetic ground truth: background 0, one ellipse per label, each inside a ring of void (255) `ring` pixels wide."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    t = np.zeros((h, w), np.int32)
    for l in labels:
        cy, cx = rng.uniform(0.2, 0.8) * h, rng.uniform(0.2, 0.8) * w
        ry, rx = rng.uniform(0.08, 0.2) * h + ring + 1, rng.uniform(0.08, 0.2) * w + ring + 1
        outer = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
        inner = ((yy - cy) / (ry - ring)) ** 2 + ((xx - cx) / (rx - ring)) ** 2 <= 1.0
        t[outer] = 255
        t[inner] = l
    return t


def cat_gt():
    from PIL import Image
    return np.asarray(Image.open(os.path.join(GOLDEN, "test_cat_gt.png"))).astype(np.int32)


WIDTHS = [1, 2, 4, 8, 16, 32]


# ---- the restatement against scipy ---------------------------------------------------------------------------------------
def test_restatement_equals_scipy_on_the_cat():
    t = cat_gt()
    assert t.shape == (375, 500)
    for r in (1, 5, 32, 64):
        assert np.array_equal(dist2_numpy(t, r), dist2_scipy(t, r)), r
    d2 = dist2_numpy(t, 32)
    assert_bands_say_something(t, d2, WIDTHS)
    # the figures the design notes quote
    b = boundary_numpy(t)
    w1 = d2.astype(np.int64) <= 1
    assert int(w1.sum()) == 6906 and int((w1 & (t == 255)).sum()) == 3457
    assert int((w1 & (t == 0)).sum()) == 1740 and int((w1 & (t == 8)).sum()) == 1709
    assert round(band_share(d2, 1), 3) == 0.037 and round(band_share(d2, 32), 3) == 0.308
    assert b.sum() > 0 and (d2[b] == 0).all() and (d2[~b] != 0).all()


@pytest.mark.parametrize("seed,h,w", [(0, 96, 128), (1, 200, 75), (2, 64, 64), (3, 130, 257)])
def test_restatement_equals_scipy_on_blob_maps(seed, h, w):
    t = blob_map(seed, h, w)
    for r in (1, 7, 32, 64):
        assert np.array_equal(dist2_numpy(t, r), dist2_scipy(t, r)), r


def test_the_blob_maps_of_the_gpu_tests_have_bands_that_say_something():
    for seed, h, w in [(11, 512, 512), (12, 512, 512), (13, 512, 512), (14, 1024, 1024), (15, 375, 500)]:
        t = blob_map(seed, h, w)
        assert_bands_say_something(t, dist2_numpy(t, 32), WIDTHS)


# ---- known answers by hand -----------------------------------------------------------------------------------------------
def test_a_single_vertical_edge():
    t = np.zeros((9, 40), np.int32)
    t[:, 17:] = 4                                                  # columns 16 and 17 are the boundary pixels
    b = boundary_numpy(t)
    assert b[:, 16:18].all() and b.sum() == 2 * 9
    d2 = dist2_numpy(t, 64)
    col = np.arange(40)
    want = np.minimum(np.abs(col - 16), np.abs(col - 17)) ** 2     # d = column distance, whatever the row
    assert np.array_equal(d2, np.broadcast_to(want, (9, 40)))
    assert np.array_equal(dist2_numpy(t, 5), np.broadcast_to(np.where(want <= 25, want, NONE), (9, 40)))


def test_one_isolated_pixel():
    t = np.zeros((11, 11), np.int32)
    t[5, 5] = 9
    b = boundary_numpy(t)
    assert sorted(zip(*np.nonzero(b))) == [(4, 5), (5, 4), (5, 5), (5, 6), (6, 5)]     # itself and its four neighbours
    d2 = dist2_numpy(t, 64)
    assert d2[5, 5] == 0 and d2[4, 4] == 1 and d2[0, 0] == 4 * 4 + 5 * 5 and d2[5, 0] == 4 * 4 and d2[3, 4] == 2


def test_a_constant_map_has_empty_bands():
    t = np.full((20, 30), 7, np.int32)
    assert not boundary_numpy(t).any()                               # the image border makes no boundary
    d2 = dist2_numpy(t, 64)
    assert (d2 == NONE).all() and (dist2_scipy(t, 64) == NONE).all()
    assert band_counts_numpy(t, t, d2, [1, 64], -1).sum() == 0       # an empty band on purpose


def test_a_boundary_in_a_corner():
    t = np.zeros((6, 7), np.int32)
    t[0, 0] = 255                                                    # void makes boundaries like any value
    assert sorted(zip(*np.nonzero(boundary_numpy(t)))) == [(0, 0), (0, 1), (1, 0)]
    d2 = dist2_numpy(t, 3)
    assert d2[0, 0] == 0 and d2[1, 1] == 1 and d2[2, 2] == 5 and d2[0, 4] == 9 and d2[0, 5] == NONE and d2[3, 3] == NONE
    assert np.array_equal(d2, dist2_scipy(t, 3))
    t = np.zeros((6, 7), np.int32)
    t[5, 6] = 1
    assert np.array_equal(dist2_numpy(t, 64), dist2_scipy(t, 64)) and dist2_numpy(t, 64)[0, 0] == 5 * 5 + 5 * 5


# ---- bands --------------------------------------------------------------------------------------------------------------
def test_bands_are_nested_and_ignore_label_removes_pixels_but_not_boundaries():
    t = blob_map(5, 360, 480)
    p = blob_map(6, 360, 480, ring=0)
    d2 = dist2_numpy(t, 32)
    assert_bands_say_something(t, d2, WIDTHS)
    c = band_counts_numpy(t, p, d2, WIDTHS, 255)
    assert (np.diff(c, axis=0) >= 0).all() and (c[-1] > c[0]).any()          # nested: no bin ever shrinks with the width
    assert c[:, 0, 255].sum() == 0                                          # the ignored label is in no bin of the truth
    keep = band_counts_numpy(t, p, d2, WIDTHS, -1)
    assert (keep[:, 0, 255] > 0).all() and np.array_equal(keep[:, 0, :255], c[:, 0, :255])
    # ignored pixels still make boundaries: without the void ring the distance map is another one
    assert not np.array_equal(d2, dist2_numpy(np.where(t == 255, 0, t), 32))
    # order and repeats of the widths are the caller's
    mixed = band_counts_numpy(t, p, d2, [8, 1, 8, 32], 255)
    assert np.array_equal(mixed[0], c[3]) and np.array_equal(mixed[1], c[0]) and np.array_equal(mixed[2], c[3])


def test_a_covering_band_counts_what_class_counts_counts():
    rng = np.random.default_rng(7)
    t = rng.choice([0, 3, 8, 255, 300, -2], (40, 50)).astype(np.int32)       # noise: every pixel is near a boundary
    p = rng.choice([0, 3, 8, 12, 256], (40, 50)).astype(np.int32)
    d2 = dist2_numpy(t, 64)
    assert band_share(d2, 64) == 1.0                                         # a covering band on purpose
    assert np.array_equal(band_counts_numpy(t, p, d2, [64], -1)[0], counts_numpy(t, p))


# ---- the CSV ------------------------------------------------------------------------------------------------------------
def test_trimap_csv_layout(tmp_path):
    from asr_amd import evaluation as E
    rng = np.random.default_rng(8)
    t = rng.choice([0, 3, 8, 255], 4000)
    preds = [rng.choice([0, 3, 8], 4000) for _ in range(4)]
    nested = [np.arange(4000) < n for n in (500, 1500)]                      # two hand-made "bands"
    band = np.stack([[counts_numpy(t[s & (t != 255)], p[s & (t != 255)]) for s in nested] for p in preds])
    whole = np.stack([counts_numpy(t, p) for p in preds])
    band[2] = 0                                                              # no max label map
    rows = rng.random((3, 4, 2))
    path = str(tmp_path / "trimap.csv")
    E.write_trimap_csv(path, [2, 16], band, rows, counts=whole)
    with open(path, newline="") as fh:
        got = list(csv.reader(fh))
    assert got[0] == ["Name"] + [f"{k}_{c}" for k in ("standard", "aug", "max", "mean")
                                 for c in ("band_mIoU", "band_mean_image_mIoU")] + ["band_pixels", "band_share", "n"]
    assert [r[0] for r in got[1:]] == ["w=2", "w=16"]
    for b in range(2):
        r = got[1 + b]
        for j in (0, 1, 3):
            assert float(r[1 + 2 * j]) == E.dataset_miou(band[j, b])
            assert float(r[2 + 2 * j]) == float(np.mean(rows[:, j, b]))
        assert np.isnan(float(r[5])) and np.isnan(float(r[6]))               # the label map that was not produced
        pixels = int((nested[b] & (t != 255)).sum())
        assert int(r[9]) == pixels and float(r[10]) == pixels / int((t != 255).sum()) and r[11] == "3"
    E.write_trimap_csv(path, [2, 16], band, rows)                            # without whole-image counts: no share
    with open(path, newline="") as fh:
        assert all(np.isnan(float(r[10])) for r in list(csv.reader(fh))[1:])


# ---- refusals that need no GPU -------------------------------------------------------------------------------------------
def test_band_widths_are_checked_on_the_host():
    from asr_amd import ops, utils
    from asr_amd.pipeline import HotPath
    assert ops.check_band_widths((8, 1, 8, 64)) == [8, 1, 8, 64]
    for bad in ([0], [65], [1, -3], list(range(1, 18)), [], [1.5], 4):
        with pytest.raises(ValueError):
            ops.check_band_widths(bad)
        with pytest.raises(ValueError):
            utils.trimap_counts(np.zeros((4, 4), np.int32), np.zeros((4, 4), np.int32), bad)
        with pytest.raises(ValueError):
            HotPath(None, None).run_image_labels(None, [], [], class_ids=[3], band_widths=bad)
    with pytest.raises(ValueError):
        ops.check_band_widths([1, 9], r_max=8)
    with pytest.raises(ValueError, match="img_size"):
        utils.trimap_counts(np.zeros(16, np.int32), np.zeros(16, np.int32), [1])      # a flat map has no boundaries to measure


def _ints(*v):
    return (C.c_int * max(len(v), 1))(*v)


def test_entry_points_reject_bad_arguments_before_any_launch(lib):
    fake = C.c_void_p(1 << 20)                                          # non-null; never dereferenced on the host
    dist = lambda t, d, s, h, w, r: lib.asr_boundary_dist2_u16(t, d, s, h, w, r, None)
    assert dist(None, fake, 1, 8, 8, 4) == -1 and b"null pointer" in lib.asr_last_error()
    assert dist(fake, None, 1, 8, 8, 4) == -1 and b"null pointer" in lib.asr_last_error()
    assert dist(fake, fake, 1, 8, 8, 0) == -1 and b"r_max 0" in lib.asr_last_error()
    assert dist(fake, fake, 1, 8, 8, 65) == -1 and b"r_max 65" in lib.asr_last_error()
    assert dist(fake, fake, 0, 8, 8, 4) == -1 and b"bad shape" in lib.asr_last_error()
    assert dist(fake, fake, 1, 0, 8, 4) == -1 and b"bad shape" in lib.asr_last_error()
    band = lambda t, widths, p, b, r: lib.asr_band_class_counts_i32(t, fake, fake, widths, fake, 64, p, b, r, 255, None)
    assert band(None, _ints(1), 1, 1, 4) == -1 and b"null pointer" in lib.asr_last_error()
    assert band(fake, None, 1, 1, 4) == -1 and b"null width array" in lib.asr_last_error()
    assert band(fake, _ints(1), 9, 1, 4) == -1 and b"9 predictions" in lib.asr_last_error()
    assert band(fake, _ints(1), 0, 1, 4) == -1 and b"0 predictions" in lib.asr_last_error()
    assert band(fake, _ints(*([1] * 17)), 1, 17, 4) == -1 and b"17 widths" in lib.asr_last_error()
    assert band(fake, _ints(1), 1, 0, 4) == -1 and b"0 widths" in lib.asr_last_error()
    assert band(fake, _ints(2, 0), 1, 2, 4) == -1 and b"width 0 out of range" in lib.asr_last_error()
    assert band(fake, _ints(65), 1, 1, 64) == -1 and b"width 65 out of range" in lib.asr_last_error()
    assert band(fake, _ints(2, 5), 1, 2, 4) == -1 and b"width 5 > r_max 4" in lib.asr_last_error()
    assert band(fake, _ints(2), 1, 1, 65) == -1 and b"r_max 65" in lib.asr_last_error()


# ---- two gloo ranks gather the band records in the same all-gather ------------------------------------------------------
def _band_record(g, n_b=3):
    from test_labelmap_host import _record
    rng = np.random.default_rng(500 + g)
    miou, counts = _record(g)
    band = np.cumsum(rng.integers(0, 50, (4, n_b, 3, 256)), axis=1)          # nested by construction
    band_miou = rng.random((4, n_b))
    if g == 1:
        band_miou[2] = np.nan
    return miou, counts, band_miou, band


def _band_worker(rank, world, port, num_images, q):
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
    recs = [_band_record(g) for g in mine]
    whole, band = fields = E.label_fields(E.LABELMAP_KEYS, n_bands=3)
    out = E.gather_labelmap_records(mine, fields, {whole: ([r[0] for r in recs], [r[1] for r in recs]),
                                                   band: ([r[2] for r in recs], [r[3] for r in recs])}, num_images)
    q.put((rank,) + tuple(out))
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


def _gather(world, num_images):
    import torch.multiprocessing as mp
    from test_labelmap_host import _free_port
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_band_worker, args=(r, world, port, num_images, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=180) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return res


def test_two_rank_gather_carries_the_band_records():
    num_images = 5
    exp = [_band_record(g) for g in range(num_images)]
    for _rank, rows, total, band_rows, band_total in _gather(2, num_images) + _gather(1, num_images):
        np.testing.assert_array_equal(rows, np.stack([e[0] for e in exp]))
        assert np.array_equal(total, sum(e[1] for e in exp))
        np.testing.assert_array_equal(band_rows, np.stack([e[2] for e in exp]))          # [images, 4, B], the NaN included
        assert band_total.dtype == np.int64 and np.array_equal(band_total, sum(e[3] for e in exp))
