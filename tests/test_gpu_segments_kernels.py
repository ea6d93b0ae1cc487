"""asr_segment_match_i32 against the numpy restatement (tests/segments_ref.py), bit for bit: the counts and both planes, on
shapes built from the exported tile size (one pixel, one row, one column, every combination of one pixel less than, exactly and
one pixel more than a tile, 2 x 2 tiles and a bit, and 6 x 6 ragged tiles with three different predictions in one call) and on
contents that fill a tile's pair table (1024 distinct pairs) or spread one pair over every tile."""
import numpy as np
import pytest
import torch

import regions_ref as R
import segments_ref as S
from segments_cases import CASES, expected
from test_gpu_regions_kernels import BIG, SHAPES, all_equal, blocks, random_of, serpentine, spiral

pytestmark = pytest.mark.gpu

VALUES = (0, 3, 8, 12, 255)


def checkerboard(h, w, rng):
    """7 and 2 in turn: 7 is all_equal's value, so against it every other pixel is a one-pixel segment of the truth's value"""
    y, x = np.mgrid[:h, :w]
    return np.where((y + x) & 1, 7, 2).astype(np.int32)


def big_blocks(h, w, rng):
    """blobs of 40 x 24 pixels over 0, 1, 1, 3: wider than a tile one way, narrower the other"""
    coarse = rng.choice(np.array([0, 1, 1, 3], dtype=np.int32), size=((h + 39) // 40, (w + 23) // 24))
    return np.ascontiguousarray(np.kron(coarse, np.ones((40, 24), np.int32))[:h, :w])


def striped(h, w, rng):
    """random over VALUES with a void stripe down the middle column and along the middle row"""
    m = random_of(VALUES)(h, w, rng)
    m[:, w // 2] = 255
    m[h // 2, : max(1, w // 3)] = 255
    return m


def shifted(m):
    """the map moved one pixel down and right, the first row and column repeated"""
    out = m.copy()
    out[1:, 1:] = m[:-1, :-1]
    return out


def groups(h, w, rng):
    """[(truth, [predictions], [(L, include_zero), ...])]: each truth is matched in ONE call per parameter pair"""
    a, eq, ch, sp, se, ext = (f(h, w, rng) for f in (striped, all_equal, checkerboard, spiral, serpentine, blocks))
    bb = big_blocks(h, w, rng)
    return [
        (a, [a, shifted(a), striped(h, w, rng), ext], [(21, False), (64, True)]),
        (eq, [ch, eq, bb], [(21, False)]),                        # all-equal truth, checkerboard: the LDS table at its fullest
        (ch, [eq, ch, shifted(ch)], [(64, False)]),               # ... and the reverse
        (se, [bb, sp, se], [(21, False), (1, True)]),             # one pair's count adds up across tiles
        (sp, [bb, se], [(21, True)]),
        (ext, [ext, shifted(ext), a], [(64, True), (1, False)]),  # the int32 extremes
    ]


class Labelled:
    """regions_ref.label_regions, once per map and connectivity"""

    def __init__(self):
        self.seen = {}

    def __call__(self, m, c):
        key = (m.shape, m.tobytes(), c)
        if key not in self.seen:
            self.seen[key] = R.label_regions(m, c)
        return self.seen[key]


def _check(dev, truth, preds, L, c, zero, labelled, extras=True):
    """truth [h, w] and a list of predictions, matched in ONE call."""
    from asr_amd import ops
    h, w = truth.shape
    n = h * w
    host = np.stack(preds)
    t_dev, p_dev = torch.as_tensor(truth).to(dev), torch.as_tensor(host).to(dev)
    counts, pm, tm = ops.segment_match(t_dev, p_dev, L, c, zero, want_planes=True)
    again = ops.segment_match(t_dev.clone(), p_dev.clone(), L, c, zero, want_planes=True)
    assert all(torch.equal(x, y) for x, y in zip((counts, pm, tm), again))              # two calls, the same bits
    assert counts.dtype == torch.int64 and counts.shape == (len(preds), L, 4)
    assert pm.dtype == tm.dtype == torch.int32 and pm.shape == tm.shape == p_dev.shape
    counts_h, pm_h, tm_h = counts.cpu().numpy(), pm.cpu().numpy(), tm.cpu().numpy()
    t_reg = labelled(truth, c)
    v0 = 0 if zero else 1
    for j, p in enumerate(preds):
        p_reg = labelled(p, c)
        want, want_pm, want_tm = S.segment_match(truth, p, L, c, zero, truth_regions=t_reg, pred_regions=p_reg)
        assert np.array_equal(counts_h[j], want), (j, "counts", counts_h[j][want != counts_h[j]], want[want != counts_h[j]])
        assert np.array_equal(pm_h[j], want_pm), (j, "pred_match")
        assert np.array_equal(tm_h[j], want_tm), (j, "truth_match")
        # TP + FN = the truth segments, TP + FP = the predicted segments that are not dropped, counted from the roots
        idx = np.arange(n)
        t_is_root, p_is_root = t_reg[0].ravel() == idx, p_reg[0].ravel() == idx
        for v in range(L):
            n_t = np.count_nonzero(t_is_root & (truth.ravel() == v)) if v >= v0 else 0
            n_p = np.count_nonzero(p_is_root & (p.ravel() == v) & (pm_h[j].ravel() != -2)) if v >= v0 else 0
            assert counts_h[j, v, 0] + counts_h[j, v, 2] == n_t and counts_h[j, v, 0] + counts_h[j, v, 1] == n_p, (j, v)
        assert not counts_h[j, :v0].any()
    assert torch.equal(t_dev.cpu(), torch.as_tensor(truth)) and torch.equal(p_dev.cpu(), torch.as_tensor(host))   # only read
    if extras:
        # a map alone ([H, W] in, [L, 4] out) equals its row of the batch; regions given or not, planes or not, out given or not
        one = ops.segment_match(t_dev, p_dev[0], L, c, zero, want_planes=True)
        assert one[0].shape == (L, 4) and one[1].shape == (h, w)
        assert torch.equal(one[0], counts[0]) and torch.equal(one[1], pm[0]) and torch.equal(one[2], tm[0])
        regions = (ops.label_regions(t_dev, c), ops.label_regions(p_dev, c))
        out = torch.full((len(preds), L, 4), -7, dtype=torch.int64, device=dev)
        got = ops.segment_match(t_dev, p_dev, L, c, zero, truth_regions=regions[0], pred_regions=regions[1], out=out)
        assert got.data_ptr() == out.data_ptr() and torch.equal(out, counts)
    return counts_h


@pytest.mark.parametrize("c", (4, 8))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_content_at_every_tile_edge_shape(dev, shape, c):
    rng = np.random.default_rng(1000 * shape[0] + shape[1])
    labelled = Labelled()
    for k, (truth, preds, params) in enumerate(groups(*shape, rng)):
        for L, zero in params:
            _check(dev, truth, preds, L, c, zero, labelled, extras=k in (0, 3))


@pytest.mark.parametrize("c", (4, 8))
def test_three_different_predictions_of_six_by_six_ragged_tiles(dev, c):
    rng = np.random.default_rng(77)
    truth = serpentine(*BIG, rng)
    counts = _check(dev, truth, [big_blocks(*BIG, rng), spiral(*BIG, rng), shifted(truth)], 21, c, False, Labelled())
    assert counts[:, :, :3].sum() > 0


def test_a_full_tile_table_against_one_region(dev):
    """all-equal truth against a 4-connected checkerboard on 2 x 2 tiles: every tile holds 1024 distinct pairs"""
    from asr_amd._lib import REGIONS_TILE_H as TH, REGIONS_TILE_W as TW
    rng = np.random.default_rng(5)
    eq, ch = all_equal(2 * TH, 2 * TW, rng), checkerboard(2 * TH, 2 * TW, rng)
    counts = _check(dev, eq, [ch], 21, 4, False, Labelled())
    assert counts[0, 7].tolist() == [0, 2 * TH * TW, 1, 0] and counts[0, 2].tolist() == [0, 2 * TH * TW, 0, 0]
    counts = _check(dev, ch, [eq], 21, 4, False, Labelled())
    assert counts[0, 7].tolist() == [0, 1, 2 * TH * TW, 0] and counts[0, 2].tolist() == [0, 0, 2 * TH * TW, 0]


@pytest.mark.parametrize("case", CASES, ids=[k[0] for k in CASES])
def test_the_hand_drawn_cases(dev, case):
    from asr_amd import ops, utils
    _, truth, pred, L, c, zero, _ = case
    got = ops.segment_match(torch.as_tensor(truth).to(dev), torch.as_tensor(pred).to(dev), L, c, zero)
    assert np.array_equal(got.cpu().numpy(), expected(case))
    counts = utils.segment_counts(truth, pred, L, c, zero)                               # numpy in, numpy out
    assert counts.dtype == np.int64 and np.array_equal(counts, expected(case))
    assert np.array_equal(utils.segment_counts(truth[..., None], np.stack([pred, pred]), L, c, zero), np.stack([expected(case)] * 2))


def test_bad_arguments_raise_and_nothing_is_written(dev):
    from asr_amd import _lib, ops
    t = torch.zeros((5, 6), dtype=torch.int32, device=dev)
    p = torch.ones((2, 5, 6), dtype=torch.int32, device=dev)
    out = torch.full((2, 21, 4), -7, dtype=torch.int64, device=dev)
    for bad in ((0, 8), (65, 8), (21, 6), (21.5, 8), (21, 8, 2)):
        with pytest.raises(ValueError):
            ops.segment_match(t, p, *bad, out=out)
    with pytest.raises(_lib.AsrError):
        ops.segment_match(t, p.to(torch.int64), out=out)
    with pytest.raises(_lib.AsrError):
        ops.segment_match(t[:4], p, out=out)
    with pytest.raises(_lib.AsrError):
        ops.segment_match(t, p, truth_regions=(t, t[:4]), out=out)
    with pytest.raises(_lib.AsrError):
        ops.segment_match(t, p, out=out[:1])
    # the library's own refusals, past the Python checks: nothing is launched, nothing written
    lib = _lib.load()
    root = torch.zeros_like(p)
    ws = torch.full((4096,), -7, dtype=torch.int64, device=dev)
    nbytes = lib.asr_segment_match_workspace_bytes(2, 5, 6)
    assert 0 < nbytes <= ws.numel() * 8 and lib.asr_segment_match_workspace_bytes(2, 0, 6) == 0
    args = lambda **kw: [kw.get("truth", t.data_ptr()), t.data_ptr(), t.data_ptr(), p.data_ptr(), root.data_ptr(), out.data_ptr(),
                         None, None, ws.data_ptr(), kw.get("nbytes", nbytes), kw.get("maps", 2), kw.get("h", 5), 6, kw.get("L", 21),
                         0, None]
    for kw in ({"truth": None}, {"L": 0}, {"L": 65}, {"h": 0}, {"maps": 0}, {"maps": 65536}):
        assert lib.asr_segment_match_i32(*args(**kw)) != 0, kw
    assert lib.asr_segment_match_i32(*args(nbytes=nbytes - 1)) != 0
    torch.cuda.synchronize()
    assert bool((out == -7).all()) and bool((ws == -7).all())
