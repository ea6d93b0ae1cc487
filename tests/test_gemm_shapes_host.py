"""Host-only companion of tests/test_gpu_gemm_shapes.py: the bound those tests hold the split-f16 GEMM kernels to
(4e-6 * (sum |a||w| + |bias| + |residual|)) only proves something if a correct kernel passes it and a subtly wrong one does
not -- at the very shapes and data the GPU tests use (tests/gemm_shapes.py, shared by both files).

For every case, in numpy float64:
  * the split arithmetic the kernels implement (hi * whi + hi * wlo + lo * whi, products exact, float64 sum) lies within the
    bound of the float64 product: the reference alone passes;
  * each defect a kernel of this family can plausibly have -- the lo * whi term dropped, the last K chunk dropped, the
    residual read one row late, the bias read one column late, the residual added before the activation, ReLU6 without its
    clamp at 6 -- exceeds the bound on at least one output."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))      # tests/gemm_shapes.py, whatever pytest's import mode
import gemm_shapes as gs  # noqa: E402

_ids = [f"{c.kernel}-{c.id}" for c in gs.HOST_CASES]


def test_case_table_reaches_every_path():
    """The properties the GPU file's docstring table claims for its cases, derived from the table itself."""
    ids = [(c.kernel, c.id) for c in gs.HOST_CASES]
    assert len(set(ids)) == len(ids)
    phase = gs.RING_PHASE
    assert {c.kt for c in phase} == {1, 2, 3, 4, 5, 6, 7, 10}
    for res in (False, True):                                  # every ring phase, with and without a residual
        assert {c.kt % gs.RING for c in phase if c.res == res} == {0, 1, 2, 3, 4}
    for relu in (0, 1, 2):                                     # every activation mode meets a residual at least twice
        assert sum(1 for c in phase if c.res and c.relu == relu) >= 2
    assert {c.bias for c in phase if c.res} == {False, True} == {c.bias for c in phase if not c.res}
    assert any(c.k % 32 for c in phase if c.res)               # zero padding inside the last chunk
    # column tiles with real columns in the right half of the last N-tile -> the K-loop instantiation (CTV = 8 / 6 / 4 / 2)
    def ctv(n):
        valid = min(8, max(0, (n - ((n - 1) // 256 * 256 + 128) + 15) >> 4))
        return 8 if valid > 6 else 6 if valid > 4 else 4 if valid > 2 else 2
    assert {ctv(c.n) for c in gs.RING_N_TILES} == {2, 4, 6, 8}
    assert [ctv(n) for n in (132, 392, 440, 472, 512, 728)] == [2, 2, 4, 6, 8, 6]
    assert any(c.n % 4 and c.res for c in gs.RING_N_TILES)
    for c in gs.RING_CASES:                                    # one tile per workgroup: the grid stays below any CU count
        assert -(-c.m // 256) * -(-c.n // 256) <= 8 and -(-c.n // 128) * 128 % 256 == 0
    assert -(-gs.WALK.m // 256) * -(-gs.WALK.n // 256) > 256 and gs.WALK.kt >= 4     # the walk: more tiles than CUs
    assert any(c.m % 256 and c.m > 256 and c.res for c in gs.RING_CASES)
    assert {c.m for c in gs.RING_M_EDGES} == {1, 15, 16, 37, 255, 256, 257} and all(c.res for c in gs.RING_M_EDGES)
    assert all(c.n <= 64 for c in gs.SPLIT_TILE64) and all(c.n > 64 for c in gs.SPLIT_TILE128)
    for group in (gs.SPLIT_RELU6, gs.SPLIT_LDX, gs.SPLIT_SUB):     # both tiles
        assert any(c.n <= 64 for c in group) and any(c.n > 64 for c in group)
    assert {(c.n <= 64, c.res) for c in gs.SPLIT_RELU6} == {(a, b) for a in (False, True) for b in (False, True)}


@pytest.fixture(scope="module", params=gs.HOST_CASES, ids=_ids)
def data(request):
    return gs.build(request.param)


def _excess(d, out):
    return float((np.abs(out - d.ref) / d.bound).max())


def test_split_arithmetic_lies_within_the_bound(data):
    d = data
    assert d.ref.shape == (d.case.m, d.case.n) and np.isfinite(d.ref).all() and (d.bound > 0).all()
    worst = _excess(d, gs.emulate(d))
    print(f"[gemm_shapes_host] {d.case.id}: split arithmetic at {worst * gs.TOL:.2e} of the magnitude (bound {gs.TOL:.0e})")
    assert worst <= 1.0, worst * gs.TOL
    if d.case.relu == 2:
        assert min(gs.relu6_spread(d)) >= 0.10, gs.relu6_spread(d)


@pytest.mark.parametrize("mutation", gs.MUTATIONS)
def test_a_subtly_wrong_kernel_exceeds_the_bound(data, mutation):
    d = data
    if not gs.applies(d.case, mutation):
        assert mutation not in ("drop_lo_whi", "drop_last_chunk")      # these two apply to every case
        return                                                         # the case has no residual / bias / activation / clamp
    worst = _excess(d, gs.emulate(d, mutation))
    print(f"[gemm_shapes_host] {d.case.id}: {mutation} reaches {worst:.1f} x the bound")
    assert worst > 1.0, (mutation, worst)


@pytest.mark.parametrize("case", gs.CONV, ids=[c.id for c in gs.CONV])
def test_im2col_reference_is_conv2d(case):
    """The GPU test's reference for the implicit GEMM is F.conv2d in float64; the host emulation's is im2col @ w.  The same."""
    d = gs.build(case)
    b, h, w, cin, cout, stride, pad, dil = case.conv
    ho, wo = gs.conv_out_hw(case.conv)
    kern = torch.from_numpy(d.w.reshape(3, 3, cin, cout)).permute(3, 2, 0, 1).double()
    ref = F.conv2d(torch.from_numpy(d.x).permute(0, 3, 1, 2).double(), kern, torch.from_numpy(d.bias).double(), stride=stride,
                   padding=pad, dilation=dil).permute(0, 2, 3, 1).numpy()
    assert ref.shape == (b, ho, wo, cout)
    np.testing.assert_allclose(d.pre.reshape(b, ho, wo, cout), ref, rtol=0, atol=1e-12)


def test_ring_lines_layout():
    rng = np.random.default_rng(1)
    hi, lo = gs.split16(gs._rand(rng, 5, 40))
    lines = gs.ring_lines(hi, lo, 3)
    assert lines.shape == (5, 3, 2, 32) and lines.dtype == np.float16
    assert np.array_equal(lines[:, 1, 0, :8], hi[:, 32:]) and np.array_equal(lines[:, 0, 1], lo[:, :32])
    assert (lines[:, 1, :, 8:] == 0).all() and np.isnan(lines[:, 2]).all()
