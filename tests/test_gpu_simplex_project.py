"""GPU: sr_simplex_project_kernel (ops.simplex_project, asr_simplex_project_f32) against the restatement tests/sr_ml_ref.py,
bit for bit: every group size, pixel counts round the workgroup's 256 and the wave's 64, one and several groups, and planted
columns at the rule's edges.  No tolerance: reduce.hip is built without contraction and the restatement rounds every operation."""
import numpy as np
import pytest
import torch

import sr_ml_ref as M

pytestmark = pytest.mark.gpu

GROUPS = (1, 2, 3, 5, 21, 32)
PIXELS = (1, 63, 64, 65, 257, 4099)


def _planted(G):
    """Columns [G, 8] at the rule's edges: all equal (0.25 each, 1.0 each), an exact sum of 1, all negative, -0.0, one value
    1e6, two equal maxima, and an exact sum of 1 spread over the group."""
    cols = np.zeros((G, 8), np.float32)
    cols[:, 0] = 0.25
    cols[:, 1] = 1.0
    cols[0, 2] = 1.0                                              # exact sum of 1: feasible, returned as it is
    cols[:, 3] = -np.abs(np.linspace(0.1, 2.0, G, dtype=np.float32))
    cols[:, 4] = -0.0
    cols[:, 5] = np.linspace(0.0, 0.5, G, dtype=np.float32)
    cols[G // 2, 5] = 1e6
    cols[:, 6] = np.linspace(-0.2, 0.4, G, dtype=np.float32)
    cols[0, 6] = cols[G - 1, 6] = 0.9                             # two equal maxima (one value when G = 1)
    cols[:, 7] = np.float32(1.0 / 2 ** max(int(np.ceil(np.log2(G))), 0))    # G powers of two: the sum is exact, at or below 1
    return cols


def _input(G, pixels, groups, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(0.3, 0.6, (groups, G, pixels)).astype(np.float32)
    planted = _planted(G)
    k = min(pixels, planted.shape[1])
    # the planted columns go to the END of the pixel range (the partial wave / workgroup) of every group, rotated per group
    for g in range(groups):
        x[g, :, pixels - k:] = np.roll(planted, g, axis=1)[:, :k]
    return x.reshape(groups * G, pixels)


@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("G", GROUPS)
def test_the_kernel_is_the_restatement_bit_for_bit(dev, G, groups):
    from asr_amd import ops
    for pixels in PIXELS:
        x = _input(G, pixels, groups, 1000 * G + pixels)
        want = M.project_groups(x, G)
        xd = ops.to_device(x)
        out = ops.simplex_project(xd, G)
        assert out is xd
        got = xd.cpu().numpy()
        bad = int((got != want).sum())
        print(f"G={G} groups={groups} pixels={pixels}: {bad} of {got.size} values differ, max |diff| "
              f"{float(np.abs(got.astype(np.float64) - want).max()):.3e}")
        assert np.array_equal(got, want), (G, groups, pixels)
        assert not np.signbit(got).any()                          # -0 and negatives become +0
        assert float(got.min()) >= 0.0


def test_planted_columns_mean_what_they_say(dev):
    """The planted columns through the kernel, read for what the rule promises rather than against the restatement."""
    from asr_amd import ops
    G = 5
    got = ops.simplex_project(ops.to_device(_planted(G)), G).cpu().numpy()
    f = np.float32
    assert np.array_equal(got[:, 0], np.full(G, f(0.25) - f(0.25) / f(5)))    # 5 x 0.25 -> theta (1.25 - 1) / 5
    assert np.array_equal(got[:, 1], np.full(G, f(1) - f(4) / f(5)))          # 5 x 1.0 -> theta (5 - 1) / 5
    assert np.array_equal(got[:, 2], _planted(G)[:, 2])                       # sum exactly 1: untouched
    assert not got[:, 3].any() and not got[:, 4].any()
    assert got[G // 2, 5] == 1.0 and got[:, 5].sum() == 1.0                   # 1e6 takes everything
    assert got[0, 6] == got[G - 1, 6] == 0.5 and got[1:G - 1, 6].sum() == 0   # two equal maxima share the unit
    # a higher-dimensional x is its planes
    x = np.random.default_rng(3).normal(0.3, 0.6, (6, 7, 9)).astype(np.float32)
    got = ops.simplex_project(ops.to_device(x), 3).cpu().numpy()
    assert np.array_equal(got, M.project_groups(x, 3))


def test_the_c_refusals_leave_x_untouched(dev, lib):
    from asr_amd import _lib, ops
    x = np.random.default_rng(4).normal(0.3, 0.6, (6, 50)).astype(np.float32)
    xd = ops.to_device(x)
    p = xd.data_ptr()
    s = _lib.stream_ptr()
    for args, what in (((None, 2, 3, 50), b"null pointer"), ((p, 2, 0, 50), b"group"), ((p, 2, 33, 50), b"group"),
                       ((p, 2, -1, 50), b"group"), ((p, 0, 3, 50), b"bad shape"), ((p, 2, 3, 0), b"bad shape")):
        rc = lib.asr_simplex_project_f32(*args, s)
        assert rc == -1 and what in lib.asr_last_error(), (args, lib.asr_last_error())
    torch.cuda.synchronize()
    assert np.array_equal(xd.cpu().numpy(), x)
    with pytest.raises(_lib.AsrError):
        ops.simplex_project(xd, 4)                                            # 6 planes are no multiple of 4
    with pytest.raises(_lib.AsrError):
        ops.simplex_project(xd, 0)
    assert np.array_equal(xd.cpu().numpy(), x)
