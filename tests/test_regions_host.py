"""The "regions" section of include/asr_hip.h without a GPU: the numpy restatement (tests/regions_ref.py) reproduces hand-drawn
cases whose answers are written out (tests/regions_cases.py) and agrees with scipy.ndimage.label where that imports; the record
layout, the option checks, the regions CSV and the library's argument checks behave as specified."""
import csv

import numpy as np
import pytest

import regions_ref as R
from regions_cases import CLEAN, LABEL


@pytest.mark.parametrize("case", CLEAN, ids=[c[0] for c in CLEAN])
def test_the_restatement_cleans_the_hand_drawn_cases(case):
    _, labels, c, min_area, want, stats = case
    out, got = R.clean_labels(labels, min_area, c)
    assert out.dtype == np.int32 and np.array_equal(out, want)
    assert got.dtype == np.int64 and got.tolist() == stats


@pytest.mark.parametrize("case", LABEL, ids=[c[0] for c in LABEL])
def test_the_restatement_labels_the_hand_drawn_cases(case):
    _, labels, c, root, area = case
    got_root, got_area = R.label_regions(labels, c)
    assert np.array_equal(got_root, root) and np.array_equal(got_area, area)


def test_every_value_makes_regions_and_the_border_connects_nothing():
    m = np.array([[-7, -7, 255, 2 ** 30], [0, -7, 255, 2 ** 30], [0, 0, -7, 255]], dtype=np.int32)
    root, area = R.label_regions(m, 4)
    assert root.tolist() == [[0, 0, 2, 3], [4, 0, 2, 3], [4, 4, 10, 11]]
    assert area.tolist() == [[3, 3, 2, 2], [3, 3, 2, 2], [3, 3, 1, 1]]
    root8, area8 = R.label_regions(m, 8)
    assert root8.tolist() == [[0, 0, 2, 3], [4, 0, 2, 3], [4, 4, 0, 2]]       # (2, 2) joins -7 and (2, 3) joins 255 by a diagonal
    assert area8.tolist() == [[4, 4, 3, 2], [3, 4, 3, 2], [3, 3, 4, 3]]
    # a one-row map: the first and the last pixel are not neighbours
    root, area = R.label_regions(np.array([[5, 1, 5]], dtype=np.int32), 8)
    assert root.tolist() == [[0, 1, 2]] and area.tolist() == [[1, 1, 1]]


def test_the_restatement_agrees_with_scipy_per_value():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(5)
    structures = {4: ndi.generate_binary_structure(2, 1), 8: ndi.generate_binary_structure(2, 2)}
    for shape, values, p in (((37, 41), (0, 1), (0.41, 0.59)), ((50, 33), (0, 3, 9), None), ((64, 70), (-2, 0, 1, 7, 255), None)):
        m = rng.choice(np.array(values, dtype=np.int32), size=shape, p=p)
        for c in (4, 8):
            root, area = R.label_regions(m, c)
            for v in values:
                lab, n = ndi.label(m == v, structure=structures[c])
                for k in range(1, n + 1):
                    members = np.flatnonzero(lab.ravel() == k)
                    assert np.all(root.ravel()[members] == members[0]) and np.all(area.ravel()[members] == members.size)


def test_the_restatement_is_quick_on_a_long_chain():
    """a one-pixel serpentine through a 160 x 160 map: the longest chain of the GPU tests' shapes, in well under a second or two"""
    import time
    m = np.zeros((160, 160), dtype=np.int32)
    m[::2] = 1
    m[1::4, -1] = 1
    m[3::4, 0] = 1
    t0 = time.perf_counter()
    root, area = R.label_regions(m, 4)
    assert time.perf_counter() - t0 < 2.0
    assert np.all(root[m == 1] == 0) and np.all(area[m == 1] == int(m.sum()))


def test_label_fields_with_regions_appends_two_fields():
    from asr_amd.label_record import Field, label_fields, label_layout
    keys = ("standard", "aug", "max", "mean")
    assert label_fields(keys, 2, 3, 0, 4) == label_fields(keys, 2, 3, 0, 4, 0) == label_fields(keys, 2, 3, 0, 4, n_regions=0)
    for before in ((0, 0, 0, 0), (2, 21, 0, 3)):
        plain = label_fields(keys, *before)
        fields = label_fields(keys, *before, n_regions=1)
        assert fields[:len(plain)] == plain
        assert fields[len(plain):] == (Field("raw_", keys, (3, 256), True), Field("regions", keys, (4,), False))
        spans0, end0 = label_layout(plain, with_miou=True)
        spans, end = label_layout(fields, with_miou=True)
        assert spans[:len(plain)] == spans0
        assert spans[-2] == (slice(end0, end0 + 4), slice(end0 + 4, end0 + 4 + 4 * 768))
        assert spans[-1] == (None, slice(end0 + 4 + 4 * 768, end0 + 4 + 4 * 768 + 16)) and end == end0 + 4 + 4 * 768 + 16
        spans, end = label_layout(fields, with_miou=False)
        assert spans[-2][0] is None and spans[-1] == (None, slice(end - 16, end)) and end == label_layout(plain, False)[1] + 4 * 768 + 16


def test_check_min_region():
    from asr_amd.ops import check_min_region
    assert check_min_region(5) == (5, 4) and check_min_region((7, 8)) == (7, 8) and check_min_region([1, 4]) == (1, 4)
    assert check_min_region(np.int64(3)) == (3, 4) and check_min_region(4.0) == (4, 4)
    for bad in (0, -3, 2.5, "5", None, True, (5,), (5, 8, 1), (5, 6), (5, 0), (0, 4), (2.5, 4), (5, "8"), (5, None)):
        with pytest.raises(ValueError):
            check_min_region(bad)


def test_label_options_with_min_region():
    from asr_amd.pipeline import HotPath
    path = HotPath(None, None, mode="argmax")
    off = path.label_options(None, True, band_widths=(1, 2))
    assert off.min_region is None and off.sizes == (2, 0, 0, 0, 0)
    on = path.label_options(None, False, min_region=9)                       # no ground truth needed: the maps are cleaned all the same
    assert on.min_region == (9, 4) and on.sizes == (0, 0, 0, 0, 1)
    assert path.label_options(None, True, confusion_labels=21, min_region=(3, 8)).min_region == (3, 8)
    with pytest.raises(ValueError, match="th_factors with min_region"):
        path.label_options(None, True, th_factors=[0.1, 0.2], min_region=4)
    for bad in (0, (4, 5), 1.5):
        with pytest.raises(ValueError):
            path.label_options(None, True, min_region=bad)


def test_labelmap_scores_name_the_new_entries():
    from asr_amd import evaluation as E
    fields = E.label_fields(E.LABELMAP_KEYS, n_conf=2, n_regions=1)
    n, rng = 3, np.random.default_rng(2)
    local = {}
    for f in fields:
        counts = rng.integers(0, 1000, size=(n, len(f.keys)) + f.shape)
        local[f] = (rng.random((n, len(f.keys)) + f.shape[:-2]) if f.scored else None, counts)
    out = E.gather_labelmap_records(list(range(n)), fields, local, n)
    assert len(out) == 6 and out.raw_rows is out[3] and out.raw_counts is out[4] and out.regions is out[5]
    assert out.rows is out[0] and out.counts is out[1] and out.confusion is out[2] and out.band_rows is None
    assert out.raw_rows.shape == (n, 4) and out.raw_counts.shape == (4, 3, 256) and out.regions.shape == (4, 4)
    assert out.regions.dtype == np.int64 and np.array_equal(out.regions, local[fields[-1]][1].sum(axis=0))
    assert np.array_equal(out.raw_counts, local[fields[-2]][1].sum(axis=0)) and np.array_equal(out.raw_rows, local[fields[-2]][0])


def test_write_regions_csv(tmp_path):
    from asr_amd import evaluation as E
    counts, raw = np.zeros((4, 3, 256), np.int64), np.zeros((4, 3, 256), np.int64)
    # two labels; the map "aug" (column 1): raw IoUs 2/4 and 5/8, cleaned 3/4 and 6/7; "standard": unchanged 1/2, 1/1; max, mean: not produced
    raw[1, :, 0], raw[1, :, 1] = (3, 3, 2), (6, 7, 5)
    counts[1, :, 0], counts[1, :, 1] = (3, 4, 3), (6, 7, 6)
    raw[0, :, 0], raw[0, :, 1] = counts[0, :, 0], counts[0, :, 1] = (3, 1, 1), (6, 6, 6)
    regions = np.array([[5, 0, 0, 0], [40, 31, 77, 60], [0, 0, 0, 0], [0, 0, 0, 0]], np.int64)
    nan = float("nan")
    raw_rows = np.array([[0.5, 0.25, nan, nan], [0.75, 0.5, nan, nan]])
    rows = np.array([[0.5, 0.5, nan, nan], [0.75, 0.875, nan, nan]])
    path = str(tmp_path / "regions.csv")
    E.write_regions_csv(path, regions, raw, raw_rows, counts, rows)
    text = open(path).read()
    assert text.splitlines()[0] == ",".join(f'"{c}"' for c in E.REGIONS_CSV_COLUMNS)        # every cell quoted, as write_labelmap_csv
    with open(path, newline="") as fh:
        got = list(csv.reader(fh))
    assert got[0] == ["key", "regions", "small_regions", "small_region_pixels", "pixels_changed", "raw_dataset_mIoU",
                      "raw_mean_image_mIoU", "dataset_mIoU", "mean_image_mIoU"]
    assert got[1] == ["standard", "5", "0", "0", "0", repr((1 / 3 + 1.0) / 2), repr(0.625), repr((1 / 3 + 1.0) / 2), repr(0.625)]
    assert got[2] == ["aug", "40", "31", "77", "60", repr((2 / 4 + 5 / 8) / 2), repr(0.375), repr((3 / 4 + 6 / 7) / 2), repr(0.6875)]
    assert got[3] == ["max"] + ["nan"] * 8 and got[4] == ["mean"] + ["nan"] * 8 and len(got) == 5


def test_the_library_refuses_bad_arguments_before_any_launch(lib):
    from asr_amd import _lib
    assert (_lib.REGIONS_TILE_W, _lib.REGIONS_TILE_H) == (32, 32)
    header = open(__import__("os").path.join(__import__("conftest").ROOT, "include", "asr_hip.h")).read()
    assert "#define ASR_REGIONS_TILE_W 32\n" in header and "#define ASR_REGIONS_TILE_H 32\n" in header
    fake, big = 1 << 20, 1 << 40                               # non-null, aligned; never dereferenced on the host
    INVALID, WORKSPACE = -1, -4

    def label(labels=fake, root=fake, area=fake, ws=fake, ws_bytes=big, maps=1, h=8, w=8, c=4):
        return lib.asr_label_regions_i32(labels, root, area, ws, ws_bytes, maps, h, w, c, None)

    def clean(labels=fake, root=fake, area=fake, out=fake, stats=None, ws=fake, ws_bytes=big, maps=1, h=8, w=8, c=4, min_area=2):
        return lib.asr_clean_labels_i32(labels, root, area, out, stats, ws, ws_bytes, maps, h, w, c, min_area, None)

    for fn, pointers in ((label, ("labels", "root", "area", "ws")), (clean, ("labels", "root", "area", "out", "ws"))):
        for name in pointers:
            assert fn(**{name: None}) == INVALID and b"null pointer" in lib.asr_last_error()
        for c in (0, 1, 6, -4, 12):
            assert fn(c=c) == INVALID and b"connectivity" in lib.asr_last_error()
        for kw in (dict(h=0), dict(w=0), dict(h=-1), dict(w=-5)):
            assert fn(**kw) == INVALID and b"bad shape" in lib.asr_last_error()
        assert fn(h=1 << 16, w=1 << 15) == INVALID and b"2^31 - 1" in lib.asr_last_error()          # h*w = 2^31
        assert fn(h=46341, w=46341) == INVALID                                                       # just above
        for maps in (0, -1, 65536):
            assert fn(maps=maps) == INVALID and b"maps" in lib.asr_last_error()
    for bad in (0, -1):
        assert clean(min_area=bad) == INVALID and b"min_area" in lib.asr_last_error()
    need = lib.asr_label_regions_workspace_bytes(2, 8, 9)
    assert need >= 4 * 2 * 8 * 9
    assert label(maps=2, h=8, w=9, ws_bytes=need - 1) == WORKSPACE and b"workspace" in lib.asr_last_error()
    need = lib.asr_clean_labels_workspace_bytes(2, 8, 9)
    assert need >= 8 * 2 * 8 * 9
    assert clean(maps=2, h=8, w=9, ws_bytes=need - 1) == WORKSPACE and b"workspace" in lib.asr_last_error()


def test_the_workspace_sizes_are_host_arithmetic(lib):
    for fn in (lib.asr_label_regions_workspace_bytes, lib.asr_clean_labels_workspace_bytes):
        for bad in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (1, -4, 4), (1, 4, -4)):
            assert fn(*bad) == 0
        assert fn(3, 200, 199) >= 4 * 3 * 200 * 199 and fn(65535, 1, 1) > 0
        assert fn(4, 46340, 46340) >= 4 * 4 * 46340 * 46340            # beyond 2^32 bytes: size_t arithmetic


def test_the_product_refuses_cpu_tensors(lib):
    import torch
    from asr_amd import _lib, ops
    m = torch.zeros((4, 4), dtype=torch.int32)
    with pytest.raises(_lib.AsrError):
        ops.label_regions(m)
    with pytest.raises(_lib.AsrError):
        ops.clean_labels(m, 2, regions=(m, m))
