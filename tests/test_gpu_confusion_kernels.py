"""asr_confusion_counts_i32 on the MI355X against the numpy restatement of tests/test_confusion_host.py (np.add.at over the
binned pairs), every cell, bit for bit: the definitions are integer.  Pixel counts round the wave and the workgroup, and sizes
at which the grid-stride loop makes a second and a third, ragged trip (from the launcher's constants); contents that take
label_hist_add down its popcount path, its one-by-one path and both at once."""
import numpy as np
import pytest
import torch

from test_confusion_host import confusion_numpy

pytestmark = pytest.mark.gpu

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
LABELS = [1, 2, 21, 64]
PREDS = [1, 4, 8]


def _sizes():
    from asr_amd import _lib
    span, grid = _lib.CONFUSION_SPAN, _lib.CONFUSION_GRID
    # span * grid pixels are one trip of every workgroup: 5 more give workgroup 0 a second trip of 5 pixels, and
    # 2 * span * grid + span + 300 a third trip in which workgroup 0 is full, workgroup 1 ragged and the others idle
    return [1, 63, 64, 65, 255, 256, 257, span * grid + 5, 2 * span * grid + span + 300]


SMALL = [1, 63, 64, 65, 255, 256, 257]


def _dev_i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def _others(L):
    """Values that all fall into the other bin."""
    return np.array([-1, I32_MIN, L, 255, I32_MAX], np.int64)


def _run(truth, preds, L, dev):
    """The matrices through ops.confusion_counts into a buffer full of garbage, checked against numpy and the identities."""
    from asr_amd import ops
    P, n = preds.shape
    t, q = _dev_i32(truth, dev), _dev_i32(preds, dev)
    out = torch.full((P * (L + 1) * (L + 1),), -0x5A5A5A5A5A5A, dtype=torch.int64, device=dev)       # zeroed by the call
    got = ops.confusion_counts(t, q, L, out=out)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (P, L + 1, L + 1) and got.dtype == torch.int64
    got = got.cpu().numpy()
    for p in range(P):
        want = confusion_numpy(truth, preds[p], L)
        assert np.array_equal(got[p], want), (n, L, p, np.argwhere(got[p] != want)[:4])
        assert int(got[p].sum()) == n
    return got, t, q


def _pairs(n, L, rng):
    """n (truth, prediction) values drawn over all (L + 1)^2 bins, the other bin through its several spellings."""
    other = _others(L)
    def draw():
        b = rng.integers(0, L + 1, n)
        return np.where(b == L, other[rng.integers(0, len(other), n)], b)
    return draw(), draw()


@pytest.mark.parametrize("P", PREDS)
@pytest.mark.parametrize("L", LABELS)
def test_random_maps_every_size(dev, L, P):
    from asr_amd import ops
    for n in _sizes():
        rng = np.random.default_rng(n * 131 + L * 7 + P)
        truth, _ = _pairs(n, L, rng)
        # mostly background on background, as label maps are, over a uniform draw of every bin
        preds = np.stack([np.where(rng.random(n) < 0.6, truth, _pairs(n, L, rng)[1]) for _ in range(P)])
        got, t, q = _run(truth, preds, L, dev)
        # rows, columns and diagonal are asr_class_counts_i32's
        for p in (0, P - 1):
            cc = ops.class_counts(t, q[p].contiguous())[0].cpu().numpy()
            assert np.array_equal(got[p].sum(axis=1)[:L], cc[0, :L]) and np.array_equal(got[p].sum(axis=0)[:L], cc[1, :L])
            assert np.array_equal(np.diagonal(got[p])[:L], cc[2, :L])


@pytest.mark.parametrize("L", LABELS)
def test_one_pair_everywhere_is_one_cell(dev, L):
    """Every lane holds lane 0's key: the ballot and popcount path alone."""
    sizes = _sizes()
    for n in (SMALL + sizes[-2:-1]):
        for tv, pv in ((0, 0), (L - 1, 0), (0, L - 1), (255, L - 1), (L - 1, -1), (I32_MIN, I32_MAX)):
            truth = np.full(n, tv, np.int64)
            preds = np.stack([np.full(n, pv, np.int64), np.full(n, tv, np.int64)])
            got, _, _ = _run(truth, preds, L, dev)
            assert np.count_nonzero(got[0]) == 1 and np.count_nonzero(got[1]) == 1


@pytest.mark.parametrize("L", LABELS)
def test_every_lane_another_pair(dev, L):
    """Neighbouring pixels walk through all (L + 1)^2 cells: with L >= 8 no two lanes of a wave share a key (one-by-one path)."""
    side = L + 1
    for n in SMALL + _sizes()[-2:-1]:
        k = np.arange(n) % (side * side)
        spell = lambda b, alt: np.where(b == L, alt, b)
        truth = spell(k // side, 255)
        preds = np.stack([spell(k % side, -1), spell((k + 1) % side, I32_MAX), spell((k * 5 + 3) % side, L)])
        _run(truth, preds, L, dev)
    if L >= 8:
        assert len(set((np.arange(64) % (side * side)).tolist())) == 64


@pytest.mark.parametrize("L", LABELS)
def test_lane_zero_holds_a_rare_pair(dev, L):
    """Lane 0 alone adds by popcount, the 63 other lanes, which share one key, one by one -- and the reverse, a wave whose last
    lane alone differs."""
    for n in SMALL + _sizes()[-2:-1]:
        i = np.arange(n)
        truth = np.where(i % 64 == 0, L - 1, 0)
        preds = np.stack([np.where(i % 64 == 0, 255, 0), np.where(i % 64 == 63, L - 1, 0), np.zeros(n, np.int64),
                          np.where(i % 64 == 0, L - 1, I32_MIN)])
        _run(truth, preds, L, dev)


@pytest.mark.parametrize("L", LABELS)
def test_everything_outside_the_labels_is_other(dev, L):
    other = _others(L)
    n = 257
    truth = other[np.arange(n) % len(other)]
    preds = np.stack([other[(np.arange(n) // 5) % len(other)], np.zeros(n, np.int64)])
    got, _, _ = _run(truth, preds, L, dev)
    assert got[0, L, L] == n and got[1, L, 0] == n


def test_refusals_launch_nothing(dev, lib):
    t = _dev_i32(np.zeros(256), dev)
    preds = t.repeat(9, 1).contiguous()
    counts = torch.full((9 * 66 * 66,), -5, dtype=torch.int64, device=dev)
    call = lambda tp, pp, cp, pixels, p, labels: lib.asr_confusion_counts_i32(tp, pp, cp, pixels, p, labels, None)
    good = (t.data_ptr(), preds.data_ptr(), counts.data_ptr())
    assert call(None, good[1], good[2], 256, 1, 21) == -1 and b"null pointer" in lib.asr_last_error()
    assert call(good[0], None, good[2], 256, 1, 21) == -1 and b"null pointer" in lib.asr_last_error()
    assert call(good[0], good[1], None, 256, 1, 21) == -1 and b"null pointer" in lib.asr_last_error()
    assert call(*good, 0, 1, 21) == -1 and b"pixels=0" in lib.asr_last_error()
    assert call(*good, -1, 1, 21) == -1 and b"pixels=-1" in lib.asr_last_error()
    assert call(*good, 256, 0, 21) == -1 and b"0 predictions" in lib.asr_last_error()
    assert call(*good, 256, 9, 21) == -1 and b"9 predictions" in lib.asr_last_error()
    assert call(*good, 256, 1, 0) == -1 and b"0 labels" in lib.asr_last_error()
    assert call(*good, 256, 1, 65) == -1 and b"65 labels" in lib.asr_last_error()
    torch.cuda.synchronize()
    assert bool((counts == -5).all())                                        # not even the zeroing ran
    assert call(*good, 256, 8, 64) == 0                                      # and the largest good call next to them
    torch.cuda.synchronize()
    got = counts[:8 * 65 * 65].view(8, 65, 65).cpu().numpy()
    assert all(got[p, 0, 0] == 256 and got[p].sum() == 256 for p in range(8)) and bool((counts[8 * 65 * 65:] == -5).all())
