"""asr_boundary_dist2_u16 and asr_band_class_counts_i32 on the MI355X against the numpy restatement of tests/test_trimap_host.py
(itself pinned against scipy's distance transform there; where scipy imports here it is asked directly too).  Every element,
every bin: the definitions are integer."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_labelmap_host import counts_numpy
from test_trimap_host import (NONE, WIDTHS, assert_bands_say_something, band_counts_numpy, band_share, blob_map, cat_gt,
                              dist2_numpy, dist2_scipy)

pytestmark = pytest.mark.gpu


def _dev_i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def _dist2(t, r_max, dev, segments=1):
    from asr_amd import ops
    out = ops.boundary_dist2(_dev_i32(t, dev), r_max, segments=segments)
    assert out.dtype == torch.uint16 and tuple(out.shape) == tuple(np.shape(t))
    return out.cpu().numpy()


def _oracle(t, r_max):
    want = dist2_numpy(t, r_max)
    try:
        import scipy.ndimage  # noqa: F401
    except ImportError:
        return want
    assert np.array_equal(want, dist2_scipy(t, r_max))
    return want


def _edge_map(h, w):
    """Boundaries on the first and last row and column, labels including 255 and values outside 0..255."""
    rng = np.random.default_rng(h * 1000 + w)
    t = np.zeros((h, w), np.int32)
    t[0, : max(1, w // 3)] = 255
    t[-1, w // 2:] = 300
    t[: max(1, h // 2), 0] = -7
    t[h // 3:, -1] = 12
    for _ in range(3):
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        t[y:y + 3, x:x + 5] = int(rng.choice([3, 255, 1000]))
    return t


SHAPES = [(1, 1), (1, 300), (7, 513), (375, 500), (512, 512), (1024, 1024)]


@pytest.mark.parametrize("h,w", SHAPES)
@pytest.mark.parametrize("r_max", [1, 5, 32, 64])
def test_distance_equals_the_clipped_oracle(dev, h, w, r_max):
    maps = [_edge_map(h, w)]
    if (h, w) == (375, 500):
        maps.append(cat_gt())
    elif h >= 375:
        maps.append(blob_map(11 if h == 512 else 14, h, w))
    for t in maps:
        got = _dist2(t, r_max, dev)
        want = _oracle(t, r_max)
        assert np.array_equal(got, want), (int((got != want).sum()), np.argwhere(got != want)[:4].tolist())
    if h >= 375:
        assert 0.0 < float((want != NONE).mean()) < 1.0          # neither empty nor everything at this r_max


def test_distance_of_a_map_without_a_boundary_is_all_none(dev):
    for h, w in [(1, 1), (33, 70), (512, 512)]:
        assert (_dist2(np.full((h, w), 255, np.int32), 64, dev) == NONE).all()       # an empty band on purpose


def test_distance_of_three_segments_with_different_maps(dev):
    stack = np.stack([blob_map(15, 375, 500), cat_gt(), _edge_map(375, 500)])
    for r_max in (5, 64):
        got = _dist2(stack, r_max, dev, segments=3)
        for s in range(3):
            assert np.array_equal(got[s], _oracle(stack[s], r_max)), (r_max, s)


def _preds(t, num, seed):
    """Predictions with structure: the truth shifted, other blob maps, and labels outside 0..255."""
    rng = np.random.default_rng(seed)
    out = []
    for j in range(num):
        p = np.roll(t, (int(rng.integers(-6, 7)), int(rng.integers(-6, 7))), axis=(0, 1)).copy()
        p[p == 255] = 0
        y, x = int(rng.integers(0, t.shape[0] - 8)), int(rng.integers(0, t.shape[1] - 8))
        p[y:y + 8, x:x + 8] = [256, -1, 999, 255][j % 4]
        out.append(p)
    return np.stack(out)


def _band(t, preds, d2, widths, r_max, ignore, dev):
    from asr_amd import ops
    got = ops.band_class_counts(_dev_i32(t, dev), _dev_i32(preds, dev), torch.from_numpy(d2).to(dev), widths, r_max, ignore)
    assert got.dtype == torch.int64 and tuple(got.shape) == (len(preds), len(widths), 3, 256)
    return got.cpu().numpy()


WIDTH_SETS = {1: [4], 6: [8, 1, 32, 2, 8, 16], 16: [5, 1, 32, 2, 2, 9, 16, 3, 4, 32, 7, 6, 1, 12, 24, 8]}


@pytest.mark.parametrize("num_preds", [1, 4, 8])
@pytest.mark.parametrize("num_widths", [1, 6, 16])
@pytest.mark.parametrize("ignore", [-1, 255])
def test_band_counts_equal_the_restatement(dev, num_preds, num_widths, ignore):
    widths = WIDTH_SETS[num_widths]
    t = cat_gt() if num_preds == 4 else blob_map({1: 12, 8: 13}[num_preds], 512, 512)
    t = t.copy()
    t[5:9, 5:30] = 700                                             # a truth label outside 0..255 (makes boundaries, is never counted)
    d2 = _dist2(t, 32, dev)
    assert np.array_equal(d2, dist2_numpy(t, 32))
    assert_bands_say_something(t, d2, widths)
    preds = _preds(t, num_preds, 100 + num_preds)
    got = _band(t, preds, d2, widths, 32, ignore, dev)
    for p in range(num_preds):
        want = band_counts_numpy(t, preds[p], d2, widths, ignore)
        assert np.array_equal(got[p], want), (p, np.argwhere(got[p] != want)[:4].tolist())
    assert got[0, 0, 2].sum() > 0 and (got[:, :, 0, 255] == 0).all() == (ignore == 255)


def test_a_covering_band_counts_what_class_counts_counts(dev):
    from asr_amd import ops
    rng = np.random.default_rng(7)
    t = rng.choice([0, 3, 8, 255, 300, -2], (130, 200)).astype(np.int32)     # noise: every pixel is near a boundary
    preds = rng.choice([0, 3, 8, 12, 256], (4, 130, 200)).astype(np.int32)
    d2 = _dist2(t, 64, dev)
    assert band_share(d2, 64) == 1.0                                         # a covering band on purpose
    got = _band(t, preds, d2, [64, 64], 64, -1, dev)
    for p in range(4):
        cc = ops.class_counts(_dev_i32(t, dev), _dev_i32(preds[p], dev))[0].cpu().numpy()
        assert np.array_equal(got[p, 0], cc) and np.array_equal(got[p, 1], cc) and np.array_equal(cc, counts_numpy(t, preds[p]))


def test_refusals_launch_nothing(dev, lib):
    t = _dev_i32(blob_map(11, 64, 64), dev)
    d2 = torch.zeros((64, 64), dtype=torch.uint16, device=dev)
    counts = torch.full((9 * 17 * 768,), -5, dtype=torch.int64, device=dev)
    preds = t.repeat(9, 1, 1).contiguous()
    ints = lambda *v: (C.c_int * len(v))(*v)
    call = lambda widths, p, b, r: lib.asr_band_class_counts_i32(t.data_ptr(), preds.data_ptr(), d2.data_ptr(), widths,
                                                                 counts.data_ptr(), 64 * 64, p, b, r, 255, None)
    assert call(ints(4, 9), 1, 2, 8) == -1 and b"width 9 > r_max 8" in lib.asr_last_error()
    assert call(ints(4), 9, 1, 8) == -1 and b"9 predictions" in lib.asr_last_error()
    assert call(ints(*([4] * 17)), 1, 17, 8) == -1 and b"17 widths" in lib.asr_last_error()
    torch.cuda.synchronize()
    assert bool((counts == -5).all())                                        # not even the zeroing ran
