"""The kernels of csrc/warp.hip on the GPU beyond the one convenient shape: warp_affine (bilinear and nearest) with 1 / 2 / 3 / 4 /
21 channels, the four shared / batched combinations of source and transforms, output sizes other than the input's (1 x 1 and a
300-wide one among them), proj == 0 and proj < 0, coordinates beyond the int range and in (-1, 0), nearest rounding at exact
halves and at w - 0.5, the grid-stride trip; augment_copies wider than one workgroup (blockIdx.x > 0), its out-of-frame branch,
its refusals and its writes into a slice of a larger buffer.

Cases, data, the numpy restatement and the checks: tests/base_kernel_cases.py (tests/test_base_kernel_cases_host.py shows that
the restatement equals oracle.tf_ops and that subtly wrong kernels fail these checks).  The reference here is oracle.tf_ops:
bilinear within atol 1e-6 (images in [0, 1), the bound of test_warp_affine_matches_oracle), with the reference's exact zeros,
identity copies and integer shifts bit for bit; nearest exact.  Each test prints its largest difference ("MAXDIFF"; expected 0)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))      # tests/base_kernel_cases.py, whatever pytest's import mode
import base_kernel_cases as bk  # noqa: E402
from oracle import tf_ops  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


def _up(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _oracle(data, nearest):
    src, tf, n, out_hw = data
    img = src if src.ndim == 4 else np.broadcast_to(src, (n,) + src.shape).copy()
    return tf_ops.projective_transform(torch.from_numpy(np.ascontiguousarray(img)), np.ascontiguousarray(tf).reshape(-1, 8),
                                       output_shape=out_hw, interpolation="nearest" if nearest else "bilinear").numpy()


def _run_warp(dev, entry, tf_name):
    from asr_amd import ops
    worst = 0.0
    for case in bk.CASES[entry]:
        if case.tf_name != tf_name:
            continue
        data = bk.build_warp(case)
        src, tf, n, out_hw = data
        got = ops.warp_affine(_up(dev, src), _up(dev, tf), out_hw=out_hw, n=n,
                              interpolation="nearest" if case.nearest else "bilinear").cpu().numpy()
        worst = max(worst, bk.check_warp(case, data, got, ref=_oracle(data, case.nearest)))
        if case.combo == "bs":                          # shared transforms, batched source: every image got the same warp
            for b in range(n):
                one = ops.warp_affine(_up(dev, src[b]), _up(dev, tf), out_hw=out_hw, n=1,
                                      interpolation="nearest" if case.nearest else "bilinear").cpu().numpy()[0]
                assert bk.same_bits(got[b], one), (case.id, "image", b)
    print(f"MAXDIFF {entry} {tf_name} {worst:.3e}")


@pytest.mark.parametrize("tf_name", list(bk.WARP_TRANSFORMS) + ["stride"])
def test_warp_affine_bilinear(dev, tf_name):
    _run_warp(dev, "warp", tf_name)


@pytest.mark.parametrize("tf_name", list(bk.NEAREST_TRANSFORMS))
def test_warp_affine_nearest(dev, tf_name):
    _run_warp(dev, "nearest", tf_name)


@pytest.mark.parametrize("id", bk.ids("augment"))
def test_augment_copies(dev, id):
    from asr_amd import ops
    case = bk.case_by_id("augment", id)
    data = bk.build_augment(case)
    image, rot, trans, angles, shifts = data
    n = case.shape[0]
    got = ops.augment_copies(_up(dev, image), _up(dev, rot), _up(dev, trans)).cpu().numpy()
    tiled = torch.from_numpy(np.broadcast_to(image, (n,) + image.shape).copy())
    ref = tf_ops.translate(tf_ops.rotate(tiled, angles), shifts).numpy()
    print(f"MAXDIFF augment {id} {bk.check_augment(case, data, got, ref=ref):.3e}")


@pytest.mark.parametrize("name", list(bk.AUGMENT_REFUSALS))
def test_augment_copies_refusals_leave_out_untouched(dev, name):
    from asr_amd import ops
    from asr_amd._lib import AsrError
    n, h, w, c = bk.AUGMENT_REFUSALS[name]
    image = torch.zeros((h, w, c), device=dev)
    tf = _up(dev, np.tile(bk.shift_tf(0, 0), (n, 1)))
    out = torch.full((n, h, w, c), SENTINEL, device=dev)
    with pytest.raises(AsrError, match="channels must be 1 or 3" if name.startswith("c") else "must not exceed 65535"):
        ops.augment_copies(image, tf, tf, out=out)
    torch.cuda.synchronize()
    assert (out == SENTINEL).all(), name


@pytest.mark.parametrize("shape", [(5, 300, 3), (3, 257, 1)])
def test_augment_one_copy_into_a_slice_writes_only_its_rows(dev, shape):
    from asr_amd import ops
    h, w, c = shape
    image = bk.warp_image(shape, 5)
    buf = torch.full((3, h, w, c), SENTINEL, device=dev)
    rot, trans = bk.rotation_tf(0.4, h, w)[None], bk.shift_tf(1.25, -0.75)[None]
    ops.augment_copies(_up(dev, image), _up(dev, rot), _up(dev, trans), out=buf[1:2])
    got = buf.cpu().numpy()
    assert (got[0] == SENTINEL).all() and (got[2] == SENTINEL).all() and not (got[1] == SENTINEL).any()
    np.testing.assert_allclose(got[1:2], bk.augment_np(image, rot, trans), rtol=0, atol=bk.WARP_ATOL)
