"""asr_fuse_labels_f32 and asr_standard_labels_i32 on the GPU, bit for bit: the fusion against the numpy restatement of the
rule (tests/test_labelmap_host.py) and against the composition of the class-set entry points it replaces, the standard label
map against the sum of the standard masks."""
import numpy as np
import pytest
import torch

from test_labelmap_host import counts_numpy, fuse_numpy, masks_numpy

pytestmark = pytest.mark.gpu

F = np.float32
TH = 0.4


def _ids(k, rng):
    return [int(c) for c in rng.permutation(np.arange(1, 33))[:k]]          # distinct, unordered, in [1, 33)


GRID = np.array([-0.0, 0.0, 0.5, 1.0], F)


def _planes(kind, k, pixels, rng):
    """kind "ties": values from a set of 4 floats with both zeros; "random": uniform scores, a quarter of them snapped to the
    same 4 floats so that exact ties between classes exist there too."""
    if kind == "ties":
        return GRID[rng.integers(0, 4, (k, pixels))]
    x = rng.random((k, pixels)).astype(F)
    snap = rng.random((k, pixels)) < 0.25
    x[snap] = GRID[rng.integers(0, 4, int(snap.sum()))]
    return x


def _case(kind, k, pixels, with_max, seed):
    """Planes, max planes, th_factor, ids.  Untouched planes pass at about half of the pixels per class, which leaves no pixel
    without a class once K is large; so each class is a candidate only on a random share of the pixels -- chosen so that it
    passes on min(0.3, 1 - 0.3^(1/K)) of them: about 30 % of the pixels keep no class and many keep several -- and holds a
    zero (of either sign) that fails elsewhere."""
    rng = np.random.default_rng(seed)
    s = _planes(kind, k, pixels, rng)
    m = _planes(kind, k, pixels, rng) if with_max else None
    s[:, 0] = F(1.0)                                                        # every plane's maximum, exactly
    base = float((s >= m).mean()) if with_max else float((s > F(TH)).mean())
    share = min(0.3, 1.0 - 0.3 ** (1.0 / k)) / base
    out = rng.random((k, pixels)) >= share
    out[:, 0] = False
    s[out] = GRID[rng.integers(0, 2, int(out.sum()))]
    if with_max:
        m[out] = F(1.0)
    return s, m, TH, _ids(k, rng)


def _assert_worth_running(s, ids, th, m):
    n_pass = (masks_numpy(s, ids, th, m) != 0).sum(axis=0)
    several, none = float((n_pass >= 2).mean()), float((n_pass == 0).mean())
    if len(ids) > 1:
        assert several >= 0.05, several
    assert none >= 0.05, none


@pytest.mark.parametrize("k", [1, 2, 3, 21, 32])
@pytest.mark.parametrize("with_max", [False, True])
@pytest.mark.parametrize("kind,pixels", [("random", 50 * 73), ("ties", 256 * 9 + 1), ("random", 255)])
def test_fusion_equals_the_rule(dev, k, with_max, kind, pixels):
    from asr_amd import ops
    s, m, th, ids = _case(kind, k, pixels, with_max, seed=1000 * k + pixels + int(with_max))
    _assert_worth_running(s, ids, th, m)
    sd = ops.to_device(s, device=dev)
    md = ops.to_device(m, device=dev) if m is not None else None
    got, counts = ops.fuse_labels(sd, ids, th_factor=th, max_scores=md, classes=33)
    assert counts is None
    ref = fuse_numpy(s, ids, th, m)
    assert torch.equal(got.cpu(), torch.from_numpy(ref))
    if kind == "ties":                                  # exact ties between passing classes did decide pixels
        on = masks_numpy(s, ids, th, m) != 0
        rank = s if m is None else (s - m).astype(F)
        top = np.where(on, rank, -np.inf).max(axis=0)
        tied = ((np.where(on, rank, -np.inf) == top) & on).sum(axis=0) >= 2
        assert k == 1 or tied.mean() > 0.01


@pytest.mark.parametrize("k", [1, 3, 21])
@pytest.mark.parametrize("with_max", [False, True])
def test_fusion_against_the_entry_points_it_replaces(dev, k, with_max):
    """The masks of asr_threshold_classes_f32 on the same planes: a label c != 0 lies inside c's mask, 0 exactly where no mask
    is set, K = 1 is the mask itself; and the counts of the same pass are asr_class_counts_i32 on the written label map."""
    from asr_amd import ops
    pixels = 97 * 61
    s, m, th, ids = _case("random", k, pixels, with_max, seed=77 + k)
    _assert_worth_running(s, ids, th, m)
    rng = np.random.default_rng(5)
    truth = rng.choice(np.array(ids + [0, 0, 255, 300, -1], np.int32), pixels).astype(np.int32)     # void and uncounted labels
    sd = ops.to_device(s.reshape(k, 97, 61), device=dev)
    md = ops.to_device(m.reshape(k, 97, 61), device=dev) if m is not None else None
    td = ops.to_device(truth.reshape(97, 61), torch.int32, device=dev)
    lab, counts = ops.fuse_labels(sd, ids, th_factor=th, max_scores=md, truth=td, classes=33)
    assert lab.shape == (97, 61) and counts.shape == (3, 256)
    masks = ops.threshold_classes(sd, ids, th_mask=md) if md is not None else ops.threshold_classes(sd, ids, th_factor=th)
    for j, c in enumerate(ids):
        assert bool((masks[j][lab == c] == c).all()), c
    assert torch.equal(lab == 0, (masks == 0).all(dim=0))
    if k == 1:
        assert torch.equal(lab, masks[0])
    assert torch.equal(counts, ops.class_counts(td, lab)[0])
    assert np.array_equal(counts.cpu().numpy(), counts_numpy(truth, lab.cpu().numpy()))
    plain, none = ops.fuse_labels(sd, ids, th_factor=th, max_scores=md, classes=33)               # the pass without a truth
    assert none is None and torch.equal(plain, lab)


def test_fusion_of_all_zero_planes_is_the_zero_map(dev):
    from asr_amd import ops
    z = torch.zeros((3, 40, 40), dtype=torch.float32, device=dev)
    lab, _ = ops.fuse_labels(z, [4, 9, 2], th_factor=0.2)
    assert int(lab.abs().sum()) == 0
    lab, _ = ops.fuse_labels(z, [4, 9, 2], max_scores=-z)                   # 0 >= -0: every class passes, all margins tie
    assert bool((lab == 4).all())


@pytest.mark.parametrize("ids", [[8], [3, 8, 15], list(range(1, 21)), [20, 1, 7]])
def test_standard_labels_is_the_sum_of_the_standard_masks(dev, ids):
    """Logits drawn from a few values and constant over 4 x 4 blocks of source pixels: inside a block the four taps of every
    class are equal, the interpolation returns them exactly, and the classes that share the block's top value tie (the first
    maximum wins in both kernels).  Two rows of ordinary random logits keep the general case in."""
    from asr_amd import ops
    rng = np.random.default_rng(len(ids))
    blocks = rng.choice(np.array([-1.0, 0.0, 0.5, 2.0], F), (4, 4, 21)).astype(F)
    top2 = np.sort(blocks, axis=-1)[..., -2:]
    assert float((top2[..., 0] == top2[..., 1]).mean()) > 0.5               # the top logit is shared in most blocks
    logits = np.ascontiguousarray(np.repeat(np.repeat(blocks, 4, axis=0), 4, axis=1))
    logits[:2] = rng.standard_normal((2, 16, 21)).astype(F)
    ld = ops.to_device(logits, device=dev)
    got = ops.standard_labels(ld, (61, 67), ids)
    masks = ops.standard_mask_classes(ld, (61, 67), ids)
    assert torch.equal(got, masks.sum(dim=0).to(torch.int32))
    assert bool((got == 0).any()) and (len(ids) < 3 or bool((got != 0).any()))
