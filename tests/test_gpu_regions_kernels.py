"""asr_label_regions_i32 and asr_clean_labels_i32 against the numpy restatement (tests/regions_ref.py), bit for bit: root, area,
the cleaned map and the statistics, on shapes built from the exported tile size (one pixel, one row, one column, every
combination of one pixel less than, exactly and one pixel more than a tile, 2 x 2 tiles and a bit, and 6 x 6 ragged tiles with
three different maps in one call) and on contents that cross every tile border many times."""
import numpy as np
import pytest
import torch

import regions_ref as R
from regions_cases import CLEAN, LABEL

pytestmark = pytest.mark.gpu

from asr_amd._lib import REGIONS_TILE_H as TH, REGIONS_TILE_W as TW  # noqa: E402

SHAPES = [(1, 1), (1, TW + 1), (TH + 1, 1)] + [(TH + a, TW + b) for a in (-1, 0, 1) for b in (-1, 0, 1)] + [(2 * TH + 3, 2 * TW + 5)]
BIG = (5 * TH + 3, 5 * TW + 7)                              # 6 x 6 ragged tiles, 163 x 167 at 32 x 32
assert BIG[0] <= 200 and BIG[1] <= 200
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def all_equal(h, w, rng):
    return np.full((h, w), 7, np.int32)


def checkerboard(h, w, rng):
    y, x = np.mgrid[:h, :w]
    return (1 + ((y + x) & 1)).astype(np.int32)


def serpentine(h, w, rng):
    m = np.zeros((h, w), np.int32)
    m[::2] = 1
    m[1::4, -1] = 1
    m[3::4, 0] = 1
    return m


def spiral(h, w, rng):
    """a one-pixel-wide line that winds inwards, one pixel of 0 between its turns"""
    m = np.zeros((h, w), np.int32)
    m[0, 0] = 1
    y = x = d = turns = 0
    inside = lambda a, b: 0 <= a < h and 0 <= b < w
    while turns < 2:
        dy, dx = ((0, 1), (1, 0), (0, -1), (-1, 0))[d]
        if inside(y + dy, x + dx) and m[y + dy, x + dx] == 0 and not (inside(y + 2 * dy, x + 2 * dx) and m[y + 2 * dy, x + 2 * dx]):
            y, x, turns = y + dy, x + dx, 0
            m[y, x] = 1
        else:
            d, turns = (d + 1) % 4, turns + 1
    return m


def comb_h(h, w, rng):
    m = np.zeros((h, w), np.int32)
    m[:, 0] = 3
    m[::2] = 3
    return m


def comb_v(h, w, rng):
    return np.ascontiguousarray(comb_h(w, h, rng).T)


def random_of(values, p=None):
    def make(h, w, rng):
        return rng.choice(np.array(values, dtype=np.int32), size=(h, w), p=p)
    return make


def blocks(h, w, rng):
    """blobs of 3 x 2 pixels over the values that could trip a sentinel or an index: negatives, 255, 2^30, both ends of int32"""
    coarse = rng.choice(np.array([INT_MIN, -5, 0, 255, 2 ** 30, INT_MAX], dtype=np.int32), size=((h + 2) // 3, (w + 1) // 2))
    return np.ascontiguousarray(np.kron(coarse, np.ones((3, 2), np.int32))[:h, :w])


CONTENTS = [all_equal, checkerboard, serpentine, spiral, comb_h, comb_v, random_of((0, 1), (0.41, 0.59)), random_of((0, 1, 2)),
            random_of((0, 3, 8, 12, 255)), blocks]


def _check(dev, maps, c):
    """maps: a list of [h, w] int32 arrays, labelled and cleaned in ONE call each."""
    from asr_amd import ops
    h, w = maps[0].shape
    n = h * w
    host = np.stack(maps)
    labels = torch.as_tensor(host).to(dev)
    root, area = ops.label_regions(labels, c)
    again = ops.label_regions(labels.clone(), c)
    assert torch.equal(root, again[0]) and torch.equal(area, again[1])                   # two calls, the same bits
    assert root.dtype == torch.int32 and area.dtype == torch.int32 and root.shape == labels.shape == area.shape
    root_h, area_h = root.cpu().numpy(), area.cpu().numpy()
    assert not (root_h == -1).any()
    refs = [R.label_regions(m, c) for m in maps]
    for j, (want_root, want_area) in enumerate(refs):
        assert np.array_equal(root_h[j], want_root), (j, "root")
        assert np.array_equal(area_h[j], want_area), (j, "area")
        flat = root_h[j].ravel()
        assert np.array_equal(flat[flat], flat)                                           # root[root[p]] == root[p]
    if len(maps) == 1:                                                                    # [H, W] in, [H, W] out
        r2, a2 = ops.label_regions(labels[0], c)
        assert r2.shape == (h, w) and torch.equal(r2, root[0]) and torch.equal(a2, area[0])
    for min_area in (1, 2, 5, 17, n + 1):
        out, stats = ops.clean_labels(labels, min_area, c, regions=(root, area), want_stats=True)
        assert out.dtype == torch.int32 and stats.dtype == torch.int64 and stats.shape == (len(maps), 4)
        out_h, stats_h = out.cpu().numpy(), stats.cpu().numpy()
        for j, m in enumerate(maps):
            want, want_stats = R.clean_labels(m, min_area, c, regions=refs[j])
            assert np.array_equal(out_h[j], want), (j, min_area, "out")
            assert np.array_equal(stats_h[j], want_stats), (j, min_area, "stats")
            small = area_h[j] < min_area
            assert stats_h[j, 0] == np.count_nonzero(root_h[j].ravel() == np.arange(n))   # regions = pixels that are their own root
            assert stats_h[j, 2] == area_h[j].ravel()[(root_h[j].ravel() == np.arange(n)) & small.ravel()].sum()
        if min_area == 1:
            assert torch.equal(out, labels) and not stats_h[:, 1:].any()
        if min_area == n + 1:
            assert not out_h.any()
        # without given regions, without statistics, and in place: the same map
        assert torch.equal(ops.clean_labels(labels, min_area, c), out)
        alias = labels.clone()
        got = ops.clean_labels(alias, min_area, c, regions=(root, area), out=alias)
        assert got.data_ptr() == alias.data_ptr() and torch.equal(alias, out)
    assert torch.equal(labels.cpu(), torch.as_tensor(host))                              # the input is only read


@pytest.mark.parametrize("c", (4, 8))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_content_at_every_tile_edge_shape(dev, shape, c):
    rng = np.random.default_rng(1000 * shape[0] + shape[1])
    _check(dev, [make(*shape, rng) for make in CONTENTS], c)


@pytest.mark.parametrize("c", (4, 8))
@pytest.mark.parametrize("picks", ((serpentine, spiral, CONTENTS[6]), (comb_v, blocks, all_equal)), ids=("chains", "mixed"))
def test_three_different_maps_of_six_by_six_ragged_tiles(dev, picks, c):
    rng = np.random.default_rng(77)
    _check(dev, [make(*BIG, rng) for make in picks], c)


def test_one_map_alone_and_a_batch_give_the_same(dev):
    from asr_amd import ops
    rng = np.random.default_rng(3)
    maps = [make(2 * TH + 3, 2 * TW + 5, rng) for make in (CONTENTS[6], spiral, blocks)]
    _check(dev, maps[:1], 8)
    batch = ops.label_regions(torch.as_tensor(np.stack(maps)).to(dev), 4)
    for j, m in enumerate(maps):
        one = ops.label_regions(torch.as_tensor(m).to(dev), 4)
        assert torch.equal(one[0], batch[0][j]) and torch.equal(one[1], batch[1][j])


@pytest.mark.parametrize("case", CLEAN, ids=[k[0] for k in CLEAN])
def test_the_hand_drawn_cases_clean(dev, case):
    from asr_amd import ops, utils
    _, labels, c, min_area, want, stats = case
    out, got = ops.clean_labels(torch.as_tensor(labels).to(dev), min_area, c, want_stats=True)
    assert np.array_equal(out.cpu().numpy(), want) and got.shape == (4,) and got.cpu().tolist() == stats
    # the numpy-in, numpy-out helpers
    assert np.array_equal(utils.remove_small_regions(labels, min_area, c), want)
    assert utils.region_stats(labels, min_area, c).tolist() == stats


@pytest.mark.parametrize("case", LABEL, ids=[k[0] for k in LABEL])
def test_the_hand_drawn_cases_label(dev, case):
    from asr_amd import ops
    _, labels, c, root, area = case
    got_root, got_area = ops.label_regions(torch.as_tensor(labels).to(dev), c)
    assert np.array_equal(got_root.cpu().numpy(), root) and np.array_equal(got_area.cpu().numpy(), area)


def test_bad_arguments_raise(dev):
    from asr_amd import _lib, ops
    m = torch.zeros((5, 6), dtype=torch.int32, device=dev)
    with pytest.raises(_lib.AsrError):
        ops.label_regions(m, 6)
    with pytest.raises(_lib.AsrError):
        ops.label_regions(m.to(torch.int64))
    with pytest.raises(_lib.AsrError):
        ops.label_regions(m.view(-1))
    with pytest.raises(ValueError):
        ops.clean_labels(m, 0)
    with pytest.raises(ValueError):
        ops.clean_labels(m, 3, 5)
    with pytest.raises(_lib.AsrError):
        ops.clean_labels(m, 3, regions=(m[:4], m))
