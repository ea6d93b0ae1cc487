"""GPU parity of the split-f16 pointwise GEMMs (csrc/gemm.hip, csrc/gemm_common.h) away from the workload's own, mostly
tile-aligned shapes: every K-step count and ring phase, ragged M with a staged residual, the padded last N-tile, both
epilogues of the ring kernel, strided and offset operands, both tiles of the in-kernel-split kernel, ReLU6, the
sub-sampled gather and the implicit 3x3 GEMM at general geometry -- each against the float64 product of the SAME operands.

Conventions (cases and data: tests/gemm_shapes.py, shared with the host-only tests/test_gemm_shapes_host.py, which shows
that the split arithmetic passes this bound on this data and that subtly wrong kernels do not):
  * bound: every output within 4e-6 * (sum_k |a||w| + |bias| + |residual|) of the float64 product, activation applied in
    float64 (test_gpu_layers.py::test_pwconv_split_f16_is_f32_grade); the largest deviation is printed before it is asserted;
  * ring-kernel A operands are built on the host (hi = f16(a), lo = f16(a - hi), chunks of 32, zero padding up to ceil32(K));
    the reference is computed from hi + lo: no depthwise kernel is involved;
  * outputs are prefilled with -7: every column outside the written slice and the spare rows behind M must still hold it;
  * memory a kernel must not read into the result is NaN (columns k..ldx of x, chunks beyond ceil(K / 32), the pixels a
    sub_stride gather skips, residual columns n..ldres, the floats in front of an advanced pointer): outputs must be finite;
  * the residual / bias buffers carry one spare row / element behind the operand.

Case group                       kernel (tile)        path reached
-------------------------------  -------------------  ------------------------------------------------------------------------
test_ring_every_phase            ring, one tile       KT = 1..7, 10: KT mod 5 = 1 2 3 4 0 1 2 0 with and without a residual
                                                      (KT = 1: the vmcnt(0) prologue; KT = 2, 7: the slot_b - 1 < 0 wrap);
                                                      row tile 0 fast epilogue, row tile 1 (37 rows) slow epilogue WITH barriers
                                                      when a residual is staged; CTV = 8; K = 40: zeros inside the last chunk
test_ring_m_edges_with_residual  ring, one tile       m = 1, 15, 16, 37: every wave slow epilogue with barriers; m = 255: three
                                                      row blocks fast, one slow, in one workgroup; 256: all fast; 257: 2nd tile
test_ring_padded_n_tiles         ring, one tile       CTV = 2 (N 132, 392), 4 (440), 6 (472, 728), 8 (512) in the last N-tile's
                                                      right half, fast epilogue + slow with barriers (ragged M);
                                                      N = 250: N % 4 != 0, slow epilogue without barriers, scalar residual
test_ring_fast_and_slow_..agree  ring, one tile       fast epilogue contiguous and strided (ldy, ldres > N: the ASPP concat
                                                      layout); slow epilogue by each of its five triggers (y, bias, residual
                                                      misaligned; ldy, ldres % 4 != 0), with / without residual, bias = None
test_ring_spare_chunks           ring, one tile       ldx_chunks > chunks (through ops.pwconv_presplit's ldx_chunks)
test_walk_into_a_concat_slice    ring, WALK           persistent walk, KT mod 5 = 0: fast epilogue strided; ep_fast == false
(+ two parameter sets of test_gpu_layers.py::test_presplit_gemm_persistent_walk_...: KT mod 5 = 0, 1; CTV = 4 on the walk)
test_split_tile64                in-kernel, 128 x 64  N <= 64 ("pw16s"): decoder slice, exact tile, scalar stores + residual
                                                      + K tail of 4, one row / K = 4
test_split_tile128               in-kernel, 128 x 128 N = 65, 100, 130, 128: second N-tile of 1, 2 columns, K = 4, 36, 728,
                                                      ldres > n (vector and scalar residual)
test_split_relu6                 both tiles           relu == 2 with / without a residual
test_split_ldx                   both tiles           ldx > k
test_split_sub_stride            both tiles           sub_stride = 2 gather on an odd map, slice output / residual
test_conv3x3_geometries          implicit 3x3, both   stride 2, pad 0 / 2, dilation 2, ragged maps, cout 21 / 48 / 64 / 160
test_*_refusals                  host wrappers        unsupported / invalid arguments: AsrError, nothing written"""
import os
import sys
from dataclasses import replace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))      # tests/gemm_shapes.py, whatever pytest's import mode
import gemm_shapes as gs  # noqa: E402

pytestmark = pytest.mark.gpu

SPARE_ROWS = 2                    # rows allocated behind M in every output buffer


def _ids(cases):
    return [c.id for c in cases]


class _Out:
    """Sentinel-filled flat output buffer: row i of the result at floats lead + i * ldy .. + n."""

    def __init__(self, dev, m, n, ldy, lead):
        self.m, self.n, self.ldy, self.lead = m, n, ldy, lead
        self.buf = torch.full((lead + (m + SPARE_ROWS) * ldy,), gs.SENTINEL, device=dev)

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * self.lead

    def result(self):
        """the [m, n] result; asserts that every other float of the buffer still holds the sentinel"""
        flat = self.buf.cpu().numpy()
        idx = self.lead + np.arange(self.m)[:, None] * self.ldy + np.arange(self.n)[None, :]
        outside = np.ones(flat.size, bool)
        outside[idx.ravel()] = False
        assert (flat[outside] == gs.SENTINEL).all(), f"{int((flat[outside] != gs.SENTINEL).sum())} floats outside the slice were written"
        return flat[idx]

    def untouched(self):
        return bool((self.buf == gs.SENTINEL).all())


def _in_buf(dev, rows2d, ld, lead):
    """NaN-filled flat input buffer with rows2d [r, c] at floats lead + i * ld .. + c; -> (tensor, pointer of row 0)"""
    r, c = rows2d.shape
    flat = np.full(lead + r * ld, np.nan, np.float32)
    flat[lead + np.arange(r)[:, None] * ld + np.arange(c)[None, :]] = rows2d
    t = torch.from_numpy(flat).to(dev)
    return t, t.data_ptr() + 4 * lead


def _epilogue_operands(dev, d, c):
    bias_t, bias_p = _in_buf(dev, d.bias_full[None, :], c.n + 1, c.bias_lead) if c.bias else (None, None)
    ldres = (c.ldres or c.n) if c.res else 0
    res_t, res_p = _in_buf(dev, d.res_full, ldres, c.res_lead) if c.res else (None, None)
    return bias_t, bias_p, res_t, res_p, ldres


def _check(d, got, what=""):
    """finite, and within the f32-grade bound of the float64 reference"""
    assert got.shape == d.ref.shape
    assert np.isfinite(got).all(), f"{d.case.id} {what}: {int((~np.isfinite(got)).sum())} non-finite outputs (poisoned input read)"
    worst = float((np.abs(got - d.ref) / d.bound).max())
    print(f"[gemm_shapes] {d.case.kernel} {d.case.id} {what}: max error {worst * gs.TOL:.3e} of the magnitude (bound {gs.TOL:.0e})")
    assert worst <= 1.0, (d.case.id, what, worst * gs.TOL)
    if d.case.relu == 2:
        assert min(gs.relu6_spread(d)) >= 0.10, gs.relu6_spread(d)
    return got


def _launch_ring(dev, d, **layout):
    """asr_pwconv_mfma_f16x3_presplit on the case's data in the case's layout (overridden by `layout`) -> _Out, not yet checked.
    Through ops.pwconv_presplit where no pointer is advanced, else through the C ABI with offset pointers."""
    from asr_amd import ops, _lib
    c = replace(d.case, **layout)
    chunks = c.kt
    lines = gs.ring_lines(*d.x, c.ldx)
    xs = torch.from_numpy(lines.reshape(c.m, -1)).to(dev).view(torch.float32).reshape(c.m, lines.shape[1], 32)
    w16 = ops.pack_pw_weights_f16x3(ops.to_device(d.w))
    bias_t, bias_p, res_t, res_p, ldres = _epilogue_operands(dev, d, c)
    out = _Out(dev, c.m, c.n, c.ldy or c.n, c.y_lead)
    if c.y_lead == 0 and c.bias_lead == 0 and c.res_lead == 0:
        ops.pwconv_presplit(xs, w16, bias_t, c.k, c.n, chunks, out=out.buf, residual=res_t, relu=c.relu,
                            ldx_chunks=lines.shape[1], ldy=out.ldy, ldres=ldres, m=c.m)
    else:
        _lib.call("asr_pwconv_mfma_f16x3_presplit", xs.data_ptr(), w16.data_ptr(), bias_p, res_p, out.ptr, c.m, c.k, c.n,
                  lines.shape[1], out.ldy, ldres, c.relu, _lib.stream_ptr())
    torch.cuda.synchronize()
    return out


def _launch_split(dev, d):
    """asr_pwconv_mfma_f16x3 on the case's data and layout -> _Out"""
    from asr_amd import ops, _lib
    c = d.case
    if c.sub:
        b, h, w = c.sub
        xin = np.full((b, h, w, c.k), np.nan, np.float32)
        xin[:, ::2, ::2] = d.x[:, ::2, ::2]                    # the pixels the gather skips stay NaN
        ldx, sub, h_in, w_in = c.k, 2, h, w
    else:
        ldx, sub, h_in, w_in = c.ldx or c.k, 1, 0, 0
        xin = np.full((c.m, ldx), np.nan, np.float32)
        xin[:, :c.k] = d.a
    x = ops.to_device(xin)
    wp = ops.pack_pw_weights_f16x3(ops.to_device(d.w))
    bias_t, bias_p, res_t, res_p, ldres = _epilogue_operands(dev, d, c)
    out = _Out(dev, c.m, c.n, c.ldy or c.n, c.y_lead)
    if c.y_lead == 0 and c.bias_lead == 0 and c.res_lead == 0:
        ops.pwconv(x, wp, bias_t, c.k, c.n, out=out.buf, residual=res_t, relu=c.relu, ldx=ldx, ldy=out.ldy, ldres=ldres, m=c.m,
                   sub_stride=sub, h_in=h_in, w_in=w_in, f16x3=True)
    else:
        _lib.call("asr_pwconv_mfma_f16x3", x.data_ptr(), wp.data_ptr(), bias_p, res_p, out.ptr, c.m, c.k, c.n, ldx, out.ldy,
                  ldres, c.relu, sub, h_in, w_in, _lib.stream_ptr())
    torch.cuda.synchronize()
    return out


# ---- ring kernel, one tile per workgroup ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", gs.RING_PHASE, ids=_ids(gs.RING_PHASE))
def test_ring_every_phase(dev, case):
    d = gs.build(case)
    _check(d, _launch_ring(dev, d).result(), f"KT={case.kt} (mod 5 = {case.kt % gs.RING})")


@pytest.mark.parametrize("case", gs.RING_M_EDGES, ids=_ids(gs.RING_M_EDGES))
def test_ring_m_edges_with_residual(dev, case):
    d = gs.build(case)
    _check(d, _launch_ring(dev, d).result())


@pytest.mark.parametrize("case", gs.RING_N_TILES, ids=_ids(gs.RING_N_TILES))
def test_ring_padded_n_tiles(dev, case):
    d = gs.build(case)
    _check(d, _launch_ring(dev, d).result())


def test_ring_fast_and_slow_epilogue_agree(dev):
    """One data set through the 16-byte epilogue (contiguous; strided into a slice of a wider buffer) and through the
    element-by-element one, reached by each of its triggers in turn.  Both epilogues perform the same float32 operations in
    the same order on the same accumulators (add bias, max, min, add residual: no multiply, nothing to contract), so every
    layout must reproduce the contiguous launch BIT FOR BIT, besides sitting within the float64 bound on its own."""
    layouts = dict(gs.RING_LAYOUTS)
    for case, names in ((gs.RING_LAYOUT_DATA, [n for n, _ in gs.RING_LAYOUTS]), (gs.RING_LAYOUT_DATA_NORES, gs.RING_LAYOUTS_NORES),
                        (gs.RING_LAYOUT_DATA_NOBIAS, gs.RING_LAYOUTS_NOBIAS)):
        d = gs.build(case)
        assert names[0] == "contiguous"
        first = None
        for name in names:
            lay = {k: v for k, v in layouts[name].items() if (case.res or k not in ("ldres", "res_lead")) and (case.bias or k != "bias_lead")}
            got = _check(d, _launch_ring(dev, d, **lay).result(), name)
            if first is None:
                first = got
            diff = got.view(np.uint32) != first.view(np.uint32)
            assert not diff.any(), f"{case.id} {name}: {int(diff.sum())} outputs differ from the contiguous launch"


@pytest.mark.parametrize("case", gs.RING_LDX, ids=_ids(gs.RING_LDX))
def test_ring_spare_chunks(dev, case):
    d = gs.build(case)
    _check(d, _launch_ring(dev, d).result(), f"ldx_chunks={case.ldx}")


# ---- persistent walk --------------------------------------------------------------------------------------------------------
def test_walk_into_a_concat_slice(dev):
    """More tiles than CUs, no residual: the persistent walk.  The whole launch into columns [260, 516) of a 520-wide buffer
    (the 16-byte epilogue, strided) and once more with the bias pointer advanced by one float (ep_fast == false: the walk
    stages no bias row, every tile takes the element-by-element epilogue) must equal the contiguous launch bit for bit, the
    rest of the buffer untouched."""
    from asr_amd import ops, _lib
    c = gs.WALK
    d = gs.build(c)
    lines = gs.ring_lines(*d.x)
    xs = torch.from_numpy(lines.reshape(c.m, -1)).to(dev).view(torch.float32).reshape(c.m, c.kt, 32)
    w16 = ops.pack_pw_weights_f16x3(ops.to_device(d.w))
    whole = ops.pwconv_presplit(xs, w16, ops.to_device(d.bias), c.k, c.n, c.kt, relu=c.relu)
    _check(d, whole.cpu().numpy(), "contiguous walk")
    ld, off = 520, 260
    for lead in (0, 1):
        bias_t, bias_p = _in_buf(dev, d.bias_full[None, :], c.n + 1, lead)
        wide = torch.full((c.m + SPARE_ROWS, ld), gs.SENTINEL, device=dev)
        _lib.call("asr_pwconv_mfma_f16x3_presplit", xs.data_ptr(), w16.data_ptr(), bias_p, None, wide.data_ptr() + 4 * off,
                  c.m, c.k, c.n, c.kt, ld, 0, c.relu, _lib.stream_ptr())
        torch.cuda.synchronize()
        differ = int((wide[:c.m, off:off + c.n].contiguous().view(torch.int32) != whole.view(torch.int32)).sum())
        assert differ == 0, f"bias pointer + {lead}: {differ} outputs differ from the contiguous launch"
        assert bool((wide[:, :off] == gs.SENTINEL).all()) and bool((wide[:, off + c.n:] == gs.SENTINEL).all()) \
            and bool((wide[c.m:] == gs.SENTINEL).all()), f"bias pointer + {lead}: floats outside the slice were written"
        del wide


# ---- in-kernel-split kernel ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", gs.SPLIT_TILE64, ids=_ids(gs.SPLIT_TILE64))
def test_split_tile64(dev, case):
    d = gs.build(case)
    _check(d, _launch_split(dev, d).result())


@pytest.mark.parametrize("case", gs.SPLIT_TILE128, ids=_ids(gs.SPLIT_TILE128))
def test_split_tile128(dev, case):
    d = gs.build(case)
    _check(d, _launch_split(dev, d).result())


@pytest.mark.parametrize("case", gs.SPLIT_RELU6, ids=_ids(gs.SPLIT_RELU6))
def test_split_relu6(dev, case):
    d = gs.build(case)
    _check(d, _launch_split(dev, d).result())


@pytest.mark.parametrize("case", gs.SPLIT_LDX, ids=_ids(gs.SPLIT_LDX))
def test_split_ldx(dev, case):
    d = gs.build(case)
    _check(d, _launch_split(dev, d).result())


@pytest.mark.parametrize("case", gs.SPLIT_SUB, ids=_ids(gs.SPLIT_SUB))
def test_split_sub_stride(dev, case):
    d = gs.build(case)
    b, h, w = case.sub
    assert np.array_equal(d.a, d.x[:, ::2, ::2].reshape(-1, case.k)) and case.m == b * ((h + 1) // 2) * ((w + 1) // 2)
    _check(d, _launch_split(dev, d).result())


@pytest.mark.parametrize("case", gs.CONV, ids=_ids(gs.CONV))
def test_conv3x3_geometries(dev, case):
    """asr_conv3x3_mfma_f16x3 beyond stride 1 / pad 1 / dilation 1, against F.conv2d in float64; the bound is 4e-6 of the
    magnitude convolution, as in test_gpu_layers.py::test_conv3x3_mfma_matches_conv2d."""
    from asr_amd import ops
    d = gs.build(case)
    b, h, w, cin, cout, stride, pad, dil = case.conv
    kern = d.w.reshape(3, 3, cin, cout)
    xt = torch.from_numpy(d.x).permute(0, 3, 1, 2).double()
    ref = F.conv2d(xt, torch.from_numpy(kern).permute(3, 2, 0, 1).double(), torch.from_numpy(d.bias).double(), stride=stride,
                   padding=pad, dilation=dil).permute(0, 2, 3, 1).numpy()
    ref = gs.activation(ref, case.relu)
    mag = F.conv2d(xt.abs(), torch.from_numpy(np.abs(kern)).permute(3, 2, 0, 1).double(), stride=stride, padding=pad,
                   dilation=dil).permute(0, 2, 3, 1).numpy()
    got = ops.conv3x3_mfma(ops.to_device(d.x), ops.pack_pw_weights_f16x3(ops.to_device(d.w)), ops.to_device(d.bias), cout,
                           stride=stride, pad=pad, dil=dil, relu=case.relu, f16x3=True).cpu().numpy()
    assert got.shape == ref.shape == (b,) + gs.conv_out_hw(case.conv) + (cout,)
    assert np.isfinite(got).all()
    worst = float(np.max(np.abs(got - ref) / (mag + 1e-30)))
    print(f"[gemm_shapes] conv {case.id}: max error {worst:.3e} of the magnitude convolution (bound {gs.TOL:.0e})")
    assert worst <= gs.TOL
    if case.relu == 2:
        assert min(gs.relu6_spread(d)) >= 0.10, gs.relu6_spread(d)


# ---- refusals: AsrError before anything is written ----------------------------------------------------------------------------
def _refused(call, out, what):
    from asr_amd._lib import AsrError
    with pytest.raises(AsrError):
        call()
    torch.cuda.synchronize()
    assert out.untouched(), f"{what}: refused, but the output was written"


def test_presplit_refusals(dev):
    from asr_amd import ops, _lib
    rng = np.random.default_rng(3)
    m, k, chunks = 40, 96, 3
    hi, lo = gs.split16(gs._rand(rng, m, k))
    xs = torch.from_numpy(gs.ring_lines(hi, lo, chunks + 1).reshape(m, -1)).to(dev).view(torch.float32)   # one spare chunk per row
    res = ops.to_device(gs._rand(rng, m, 300))

    def launch(n, out, x_ptr=None, ldx_chunks=chunks + 1, ldy=None, ldres=0, residual=None):
        w16 = ops.pack_pw_weights_f16x3(ops.to_device(gs._rand(rng, k, n)))
        bias = ops.to_device(gs._rand(rng, n))
        _lib.call("asr_pwconv_mfma_f16x3_presplit", x_ptr or xs.data_ptr(), w16.data_ptr(), bias.data_ptr(), residual, out.ptr,
                  m, k, n, ldx_chunks, ldy or n, ldres, 0, _lib.stream_ptr())

    for n in (128, 300):                                       # ceil128(n) not a multiple of 256
        out = _Out(dev, m, n, n, 0)
        _refused(lambda: launch(n, out), out, f"n={n}")
    n = 256
    out = _Out(dev, m, n, n, 0)
    _refused(lambda: launch(n, out, x_ptr=xs.data_ptr() + 64), out, "x_split + 64 bytes")
    _refused(lambda: launch(n, out, ldx_chunks=chunks - 1), out, "ldx_chunks = chunks - 1")
    _refused(lambda: launch(n, out, ldy=n - 1), out, "ldy = n - 1")
    _refused(lambda: launch(n, out, ldres=n - 1, residual=res.data_ptr()), out, "ldres = n - 1")
    launch(n, out)                                             # the same launcher, accepted: the refusals above were not its own fault
    torch.cuda.synchronize()
    assert not out.untouched()


def test_split_refusals(dev):
    from asr_amd import ops, _lib
    rng = np.random.default_rng(4)
    n = 48
    x = ops.to_device(gs._rand(rng, 2 * 11 * 9 + 1, 64))
    bias = ops.to_device(gs._rand(rng, n))

    def launch(out, m, k, ldx=None, x_ptr=None, sub=1, h=0, w=0):
        wp = ops.pack_pw_weights_f16x3(ops.to_device(gs._rand(rng, k, n)))
        _lib.call("asr_pwconv_mfma_f16x3", x_ptr or x.data_ptr(), wp.data_ptr(), bias.data_ptr(), None, out.ptr, m, k, n,
                  ldx or k, n, 0, 0, sub, h, w, _lib.stream_ptr())

    out = _Out(dev, 60, n, n, 0)
    _refused(lambda: launch(out, 60, 30), out, "k = 30")
    _refused(lambda: launch(out, 60, 32, ldx=34), out, "ldx = k + 2")
    _refused(lambda: launch(out, 60, 32, x_ptr=x.data_ptr() + 4), out, "x + 4 bytes")
    _refused(lambda: launch(out, 59, 64, sub=2, h=11, w=9), out, "sub_stride = 2, m not a whole number of maps")
    launch(out, 60, 64, sub=2, h=11, w=9)
    torch.cuda.synchronize()
    assert not out.untouched()
