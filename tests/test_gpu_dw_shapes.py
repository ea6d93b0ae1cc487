"""Every depthwise kernel instantiation of csrc/dwconv.hip (33 behind three C entry points) on the GPU, bit for bit against
the fma chain they all compute: acc = bias; for (ky, kx) row-major: acc = fma(x, w, acc) -- tests/f32_exact.py::dwconv_exact.

Conventions (cases, data and checks: tests/dw_shapes.py, shared with the host-only tests/test_dw_shapes_host.py, which shows
that the oracle agrees with a float64 torch convolution, that nine subtly wrong kernels fail these checks on this data, and
that the table reaches all 33 instantiations of the built library):
  * float32 outputs EQUAL dwconv_exact (-0 equals +0); the message gives the count and the first differing index;
  * every output is also within 10 * 2^-24 * (sum |x||w| + |bias|) of the float64 sum: the bound of a ten-term chain with one
    rounding per step (the split entries through the float32 entry run at the same geometry);
  * split outputs: the hi and lo halves, read as uint16, equal split_f16_exact(dwconv_exact(...)) below c; every padding channel,
    and for asr_dwconv3x3_nhwc_split_f16 every chunk up to ldy_chunks, is 0x0000 -- the buffer is prefilled with 0xFF bytes, so
    a zero was written by the kernel; they also equal the numpy split of what the float32 entry returned (one operand, two
    producers: DESIGN.md 4.2);
  * everything a kernel must not write still holds its prefill (float32: NaN): ldy gaps, the channel offset, spare chunks of
    the fused ASPP, one pixel row behind the output;
  * x gap columns (ldx > c) are NaN: outputs must be finite.

Family                       instantiations reached
---------------------------  ---------------------------------------------------------------------------------------------
test_full_strips_16_rows     dw_stream_full_kernel<R,S,16,4,SPLIT,ACT>: 3 geometries x f32 / split x ACT 1, ACT 2 and the four
                             activation pairs behind ACT 0 (none, both, ReLU6, pre + ReLU6); h_out = 32: two strips, one seam
test_full_strips_32_rows     dw_stream_full_kernel<R,S,32,1,SPLIT,0>: h_out = 96, three strips
test_ragged_strips           dw_stream_kernel<R,S,16 | 32>: h_out = 20, 70; the split entry refuses them
test_stride_2                pad 1 on an even and an odd input, TF-SAME (pad 0) on an even one: full strip (f32, split), ragged, direct
test_leading_dimensions      ldx = 80, ldy = 88 at channel offset 8; split: ldx = 80, ldy_chunks = 4 (the fourth chunk zero)
test_narrow_and_tiny_maps    w_out = 3, 16; h_in = 1; c = 4, 8
test_direct_kernel           rates 6, 12, 18, 3 on a 16 x 20 map
test_direct_kernel_second_grid_stride_pass   2.16 M channel quads on a grid capped at 2.10 M threads
test_fused_aspp              aspp_dw3_phase_kernel<SPLIT>: ragged planes, ldx / ldy > c, pre-ReLU, ReLU6, nxg = 2, a spare chunk"""
import os
import sys
from dataclasses import replace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))      # tests/dw_shapes.py, whatever pytest's import mode
import dw_shapes as ds  # noqa: E402

pytestmark = pytest.mark.gpu

ASR_ERR_UNSUPPORTED = -2


def _ids(cases):
    return [c.id for c in cases]


def _launch(dev, case, d):
    """The case's entry point on d's operands, into prefilled buffers -> the buffers as numpy arrays (one per branch)"""
    from asr_amd import _lib
    c = case
    x = torch.from_numpy(d.xbuf).to(dev)
    w = torch.from_numpy(np.ascontiguousarray(d.w)).to(dev)
    bias = torch.from_numpy(np.ascontiguousarray(d.bias)).to(dev)
    host = [ds.out_buffer(c) for _ in ds.branches(c)]
    outs = [torch.from_numpy(h.view(np.int16) if c.split else h).to(dev) for h in host]
    ptrs = [o.data_ptr() + 4 * c.y_lead for o in outs]
    if c.aspp:
        _lib.call("asr_aspp_dwconv3_nhwc_split_f16" if c.split else "asr_aspp_dwconv3_nhwc_f32", x.data_ptr(), w.data_ptr(), bias.data_ptr(),
                  *ptrs, c.b, c.h_in, c.w_in, c.c, *c.rate, c.ld_in, c.ld_out, c.pre, c.post, _lib.stream_ptr())
    else:
        args = (x.data_ptr(), w.data_ptr(), bias.data_ptr(), ptrs[0], c.b, c.h_in, c.w_in, c.c, c.stride, c.rate, c.pad_top, c.pad_left,
                c.h_out, c.w_out, c.ld_in, c.ld_out, c.pre, c.post)
        if c.split:
            _lib.call("asr_dwconv3x3_nhwc_split_f16", *args, _lib.stream_ptr())
        else:
            _lib.call("asr_dwconv3x3_nhwc_f32", *args, c.mode, _lib.stream_ptr())
    torch.cuda.synchronize()
    return [o.cpu().numpy().view(np.uint16) if c.split else o.cpu().numpy() for o in outs]


def _check_case(dev, case):
    """One launch of the case, every check of the module docstring; a split case also runs the float32 entry on the same data"""
    assert ds.kernel_of(case) in ds.ALL_KERNELS
    d = ds.build(case)
    bufs = _launch(dev, case, d)
    ds.check_buffers(d, bufs)
    if case.post == 2:
        assert min(ds.relu6_reach(d)) >= 1
    if case.split:
        twin = replace(case, entry="aspp_f32" if case.aspp else "f32", ldy=0)
        assert ds.kernel_of(twin)[:4] == ds.kernel_of(case)[:4] or case.aspp
        for i, (buf, fbuf) in enumerate(zip(bufs, _launch(dev, twin, d))):
            y = ds.read_f32(twin, fbuf)
            ds.check_f32(d, y, i)
            ds.check_same_operand(case, *ds.read_split(case, buf), y, i)


@pytest.mark.parametrize("case", ds.FULL16, ids=_ids(ds.FULL16))
def test_full_strips_16_rows(dev, case):
    assert ds.kernel_of(case)[:5] == ("full", case.rate, case.stride, 16, 4) and case.h_out == 2 * 16
    _check_case(dev, case)


@pytest.mark.parametrize("case", ds.FULL32, ids=_ids(ds.FULL32))
def test_full_strips_32_rows(dev, case):
    assert ds.kernel_of(case)[:5] == ("full", case.rate, case.stride, 32, 1) and case.h_out == 3 * 32
    _check_case(dev, case)


@pytest.mark.parametrize("case", ds.RAGGED, ids=_ids(ds.RAGGED))
def test_ragged_strips(dev, case):
    assert ds.kernel_of(case) == ("stream", case.rate, case.stride, 16 if case.h_out == 20 else 32)
    _check_case(dev, case)


def test_split_entry_refuses_ragged_strips_and_writes_nothing(dev):
    """h_out = 20 is no multiple of the strip height: asr_dwconv3x3_nhwc_split_f16 returns ASR_ERR_UNSUPPORTED before any launch"""
    from asr_amd import _lib
    c = ds.SPLIT_RAGGED_REFUSED
    assert ds.kernel_of(c) == ds.UNSUPPORTED and c.h_out == 20
    d = ds.build(c)
    x, w, bias = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (d.xbuf, d.w, d.bias))
    out = torch.from_numpy(ds.out_buffer(c).view(np.int16)).to(dev)
    rc = _lib.load().asr_dwconv3x3_nhwc_split_f16(x.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(), c.b, c.h_in, c.w_in, c.c,
                                                  c.stride, c.rate, c.pad_top, c.pad_left, c.h_out, c.w_out, c.ld_in, c.ld_out, c.pre, c.post,
                                                  _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == ASR_ERR_UNSUPPORTED
    assert b"multiple of the strip height" in _lib.load().asr_last_error()
    assert (out.cpu().numpy().view(np.uint16) == ds.PREFILL16).all()
    full = replace(c, id="r1s1-h32-split-accepted", h_in=32, h_out=32, unsupported=False)    # the same arguments at 32 rows are accepted
    d = ds.build(full)
    ds.check_buffers(d, _launch(dev, full, d))


@pytest.mark.parametrize("case", ds.STRIDE2, ids=_ids(ds.STRIDE2))
def test_stride_2(dev, case):
    assert case.stride == 2 and ds.kernel_of(case)[0] == ("direct" if case.mode == 1 else "full" if case.h_out == 32 else "stream")
    _check_case(dev, case)


@pytest.mark.parametrize("case", ds.LEADING, ids=_ids(ds.LEADING))
def test_leading_dimensions(dev, case):
    assert case.ldx == 80 and (case.ldy == 4 if case.split else (case.ldy == 88 and case.y_lead == 8))
    _check_case(dev, case)


@pytest.mark.parametrize("case", ds.NARROW, ids=_ids(ds.NARROW))
def test_narrow_and_tiny_maps(dev, case):
    _check_case(dev, case)


@pytest.mark.parametrize("case", ds.DIRECT, ids=_ids(ds.DIRECT))
def test_direct_kernel(dev, case):
    assert ds.kernel_of(case) == ("direct",)
    _check_case(dev, case)


def test_direct_kernel_second_grid_stride_pass(dev):
    """b = 1, 64 x 66 x 2048 at rate 6: 2 162 688 channel quads on a grid capped at 8192 x 256 = 2 097 152 threads, so the last
    128 pixels are written by the second pass of the grid-stride loop.  The fma chain is held on the first and the last four
    output rows, the float64 bound and the guard row on everything."""
    case = ds.DIRECT_TWO_PASSES
    assert case.b * case.h_out * case.w_out * (case.c // 4) > ds.DIRECT_GRID and ds.kernel_of(case) == ("direct",)
    _check_case(dev, case)


@pytest.mark.parametrize("case", ds.ASPP, ids=_ids(ds.ASPP))
def test_fused_aspp(dev, case):
    from asr_amd import _lib
    assert _lib.load().asr_aspp_dwconv3_supported(case.h_out, case.w_out, *case.rate) == 1
    if case.id.endswith("nxg2"):
        assert ds.aspp_geometry(case.h_out, case.w_out, case.rate) == (6, 2)
    _check_case(dev, case)
