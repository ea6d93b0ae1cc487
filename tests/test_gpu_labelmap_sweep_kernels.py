"""asr_fuse_labels_sweep_counts_f32 on the GPU, bit for bit: against the numpy restatement (tests/test_labelmap_sweep_host.py) and
against one call of ops.fuse_labels per factor.  The planes of a case have different maxima, so that the winner of a pixel
changes from one non-zero label to another along the curve: each case asserts that, with numpy alone, before it runs."""
import numpy as np
import pytest
import torch

from test_labelmap_host import fuse_numpy
from test_labelmap_sweep_host import FACTORS_17, sweep_numpy

pytestmark = pytest.mark.gpu

F = np.float32
TRUTH_EXTRA = [0, 0, 255, 300, -1]                   # void and labels that are counted nowhere, as the fusion test draws them


def make_case(k, pixels, seed):
    """Uniform [0, 1) planes, each scaled by its own factor from [0.5, 2); class k a candidate on a random min(1, 2.5 / K) share
    of the pixels and 0.0 elsewhere; the plane's maximum at pixel 0; distinct, unordered ids from 1..32."""
    rng = np.random.default_rng(seed)
    scale = rng.uniform(0.5, 2.0, k).astype(F)
    s = (rng.random((k, pixels)).astype(F) * scale[:, None]).astype(F)
    s[rng.random((k, pixels)) >= min(1.0, 2.5 / k)] = F(0.0)
    s[:, 0] = scale                                                         # uniform < 1: nothing exceeds the scale itself
    assert np.array_equal(s.max(axis=1), scale)
    ids = [int(c) for c in rng.permutation(np.arange(1, 33))[:k]]
    truth = rng.choice(np.array(ids + TRUTH_EXTRA, np.int32), pixels).astype(np.int32)
    return s, ids, truth


def passing(s, f):
    return s > (s.max(axis=1) * F(f)).astype(F)[:, None]


def switches(maps):
    """Pixels that hold two different non-zero labels somewhere along the curve."""
    m = np.stack(maps)
    first = np.where(m != 0, m, np.iinfo(np.int32).max).min(axis=0)
    last = m.max(axis=0)
    return int(((last != 0) & (first != last)).sum())


def assert_worth_running(s, ids, factors=FACTORS_17):
    k = len(ids)
    lo, hi = passing(s, min(factors)).sum(axis=0), passing(s, max(factors)).sum(axis=0)
    if k >= 2:
        assert float((lo >= 2).mean()) >= 0.05
    assert float((hi == 0).mean()) >= 0.05
    maps = [fuse_numpy(s, ids, F(f)) for f in factors]
    assert all(not np.array_equal(a, b) for a, b in zip(maps, maps[1:]))
    if k >= 2:
        assert switches(maps) >= 20


def run_both(dev, s, ids, truth, factors, classes=33):
    """(sweep counts, the counts of one ops.fuse_labels call per factor), host int64 [T, 3, 256] each."""
    from asr_amd import ops
    sd, td = ops.to_device(s, device=dev), ops.to_device(truth, torch.int32, device=dev)
    got = ops.fuse_labels_sweep_counts(sd, ids, td, factors, classes=classes)
    assert got.shape == (len(factors), 3, 256) and got.dtype == torch.int64 and got.is_cuda
    each = torch.stack([ops.fuse_labels(sd, ids, th_factor=f, truth=td, classes=classes)[1] for f in factors])
    return got.cpu().numpy(), each.cpu().numpy()


@pytest.mark.parametrize("k", [1, 2, 3, 21, 32])
@pytest.mark.parametrize("pixels", [50 * 73, 256 * 9 + 1, 255])
def test_sweep_equals_the_rule_and_one_fusion_per_factor(dev, k, pixels):
    s, ids, truth = make_case(k, pixels, seed=1000 * k + pixels)
    assert_worth_running(s, ids)
    got, each = run_both(dev, s, ids, truth, FACTORS_17)
    assert np.array_equal(got, sweep_numpy(s, ids, truth, FACTORS_17))
    assert np.array_equal(got, each)
    assert (got[:, 0] == got[0, 0]).all() and got[0, 0].sum() == (truth >= 0).sum() - (truth == 300).sum()
    assert (got[:, 1].sum(axis=1) == pixels).all()                          # every pixel predicted once: ids < 256 here


@pytest.mark.parametrize("t", [1, 17, 64])
def test_factor_lists_unsorted_and_repeated(dev, t):
    s, ids, truth = make_case(3, 256 * 9 + 1, seed=5)
    rng = np.random.default_rng(t)
    factors = [float(f) for f in rng.uniform(-0.2, 1.1, t).astype(F)]
    if t > 1:
        factors[t // 2] = factors[0]                                        # a repeat, away from its twin
        assert sorted(factors) != factors
    got, each = run_both(dev, s, ids, truth, factors)
    assert np.array_equal(got, sweep_numpy(s, ids, truth, factors))
    assert np.array_equal(got, each)
    if t > 1:
        assert np.array_equal(got[t // 2], got[0])


def test_the_largest_class_set_with_the_longest_factor_list(dev):
    """K = 32 and T = 64 together: the largest threshold table and slot histogram a workgroup holds, over more than one trip
    of a workgroup's loop (more pixels than 512 workgroups of 256 cover in one)."""
    pixels = 512 * 256 + 256 * 3 + 5
    s, ids, truth = make_case(32, pixels, seed=64)
    factors = [float(f) for f in np.linspace(0.05, 0.95, 64, dtype=F)]
    assert_worth_running(s, ids, factors[::4])
    from asr_amd import ops
    sd, td = ops.to_device(s, device=dev), ops.to_device(truth, torch.int32, device=dev)
    got = ops.fuse_labels_sweep_counts(sd, ids, td, factors, classes=33).cpu().numpy()
    assert (got[:, 0] == got[0, 0]).all() and (got[:, 1].sum(axis=1) == pixels).all()
    for j in (0, 21, 42, 63):
        want = ops.fuse_labels(sd, ids, th_factor=factors[j], truth=td, classes=33)[1].cpu().numpy()
        assert np.array_equal(got[j], want), j
    assert np.array_equal(got[::21], sweep_numpy(s, ids, truth, factors[::21]))


def test_ties_are_decided_by_the_strict_comparison_and_the_lowest_k(dev):
    k, pixels = 3, 256 * 3 + 7
    s, ids, truth = make_case(k, pixels, seed=9)
    factors = FACTORS_17 + [-0.1]                                           # a negative factor lets the zeros pass
    mx = s.max(axis=1)
    p = 1
    planted = []
    for c in range(k):
        for f in FACTORS_17:
            th = F(mx[c] * F(f))
            for v in (th, np.nextafter(th, F(np.inf)), np.nextafter(th, F(-np.inf))):
                s[:, p] = F(0.0)
                s[c, p] = v
                planted.append((c, f, p, v > th))
                p += 1
    # equal scores in two planes, small enough to pass both thresholds at the low factors: the lowest k keeps the pixel
    v = F(0.5) * mx.min()
    tie = list(range(p, p + 8))
    s[:, tie] = F(0.0)
    s[1, tie] = s[2, tie] = v
    zeros = list(range(p + 8, p + 16))                                      # -0.0 against +0.0: equal, the lowest k again
    s[:, zeros] = F(0.0)
    s[0, zeros] = F(-0.0)
    assert p + 16 < pixels and np.array_equal(s.max(axis=1), mx)
    for c, f, q, above in planted:                                          # exactly the pixel one ulp above passes
        assert bool(passing(s, f)[c, q]) == bool(above)
    assert (fuse_numpy(s, ids, F(0.1))[tie] == ids[1]).all() and (fuse_numpy(s, ids, F(-0.1))[zeros] == ids[0]).all()
    got, each = run_both(dev, s, ids, truth, factors)
    assert np.array_equal(got, sweep_numpy(s, ids, truth, factors))
    assert np.array_equal(got, each)


def test_special_maxima(dev):
    """An all-equal plane, a plane whose maximum is negative (its thresholds run against the factor order), a plane whose
    maximum is 0, an all-zero plane, and an ordinary one; the factors extended by 0.0, -0.5 and 1.5."""
    pixels = 256 * 5 + 3
    rng = np.random.default_rng(21)
    s = np.stack([np.full(pixels, 0.25, F),
                  rng.uniform(-2.0, -0.5, pixels).astype(F),
                  -rng.random(pixels).astype(F),
                  np.zeros(pixels, F),
                  rng.random(pixels).astype(F)])
    s[2, 0] = F(0.0)
    assert s[1].max() < 0 and s[2].max() == 0
    ids = [6, 31, 2, 17, 11]
    truth = rng.choice(np.array(ids + TRUTH_EXTRA, np.int32), pixels).astype(np.int32)
    factors = FACTORS_17 + [0.0, -0.5, 1.5]
    maps = {f: fuse_numpy(s, ids, F(f)) for f in (0.1, 0.9, -0.5, 1.5)}
    assert (maps[1.5] == 31).any() and not (maps[0.1] == 31).any()          # the negative plane passes only above factor 1
    assert not any(np.isin(m, [2, 17]).any() for m in maps.values())        # zero maxima: thresholds of +-0.0, passed by no 0
    assert (maps[1.5] == 0).any() and (maps[0.9] == 6).any() and (maps[-0.5] == 11).any()
    got, each = run_both(dev, s, ids, truth, factors)
    assert np.array_equal(got, sweep_numpy(s, ids, truth, factors))
    assert np.array_equal(got, each)


def test_an_id_beyond_255_is_predicted_and_counted_nowhere(dev):
    s, _, _ = make_case(3, 50 * 73, seed=33)
    ids = [300, 7, 260]
    rng = np.random.default_rng(34)
    truth = rng.choice(np.array([7, 0, 0, 255, 300, 260, -1], np.int32), s.shape[1]).astype(np.int32)
    got, each = run_both(dev, s, ids, truth, FACTORS_17, classes=0)
    assert np.array_equal(got, sweep_numpy(s, ids, truth, FACTORS_17))
    assert np.array_equal(got, each)
    big = np.isin(fuse_numpy(s, ids, F(0.1)), [300, 260]).sum()
    assert big > 0 and got[0, 1].sum() == s.shape[1] - big                  # those pixels are in no bin


def test_refusals_from_ops(dev):
    from asr_amd import _lib, ops
    s = torch.zeros((2, 10), device=dev)
    truth = torch.zeros(10, dtype=torch.int32, device=dev)
    with pytest.raises(_lib.AsrError, match="65 threshold factors"):
        ops.fuse_labels_sweep_counts(s, [1, 2], truth, np.zeros(65))
    with pytest.raises(_lib.AsrError, match="truth has 7 pixels"):
        ops.fuse_labels_sweep_counts(s, [1, 2], truth[:7], [0.5])
    with pytest.raises(_lib.AsrError, match="one plane per class"):
        ops.fuse_labels_sweep_counts(s, [1, 2, 3], truth, [0.5])
    with pytest.raises(_lib.AsrError, match="fallback label"):
        ops.fuse_labels_sweep_counts(s, [1, 0], truth, [0.5])
    torch.cuda.synchronize()


def test_utils_surface(dev):
    from asr_amd import utils
    from asr_amd.utils import mean_iou_from_counts
    s, ids, truth = make_case(3, 50 * 73, seed=41)
    want = sweep_numpy(s, ids, truth, FACTORS_17)
    got = utils.labelmap_threshold_sweep(s.reshape(3, 50, 73), ids, truth.reshape(50, 73), FACTORS_17)
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and np.array_equal(got, want)
    miou = utils.labelmap_threshold_mIoU(s, ids, truth, FACTORS_17)
    assert miou.dtype == np.float64 and miou.shape == (17,)
    np.testing.assert_array_equal(miou, np.array([mean_iou_from_counts(c) for c in want]))
