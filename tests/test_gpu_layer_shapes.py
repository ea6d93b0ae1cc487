"""The kernels of csrc/layers.hip and csrc/sepconv.hip on the GPU beyond one tile per workgroup: the persistent tile walk of the
fused entry stem, the run walk and cross-tile prefetch of the fused sepconv, the second pass of the convolution kernels' capped
grid, maps smaller than a tile, ldx / ldy wider than the channels, ReLU6, GAP and both resize kernels at their edges, and the
wrappers' rejections.

Cases, oracles, bounds and checks: tests/layer_shapes.py, shared with the host-only tests/test_layer_shapes_host.py, which shows
that the oracles agree with torch in float64, that the table reaches the paths named below for several CU counts, and that
subtly wrong kernels fail these checks on this data.  Shapes that depend on the CU count are built for the device's
multi_processor_count.  Conventions:
  * every output buffer is NaN-prefilled, wider than the output where ldy > cout (the output at a 16-byte aligned channel
    offset) and one pixel row longer: everything outside the written slice must still be NaN, every output finite (the gap
    columns of x, where ldx > c, are NaN);
  * GAP equals the float32 replay of its add sequence; the VALU convolutions stay within 28 * 2^-24 * (sum |x||w| + |bias|) of
    the float64 convolution; the split-f16 kernels within 4e-6 of the same sum (the fused stem: layer 1's bound carried through
    |w2|); the resizes within the derived bound of layer_shapes.resize_f64;
  * the fused sepconv also equals asr_dwconv3x3_nhwc_f32 + asr_pwconv_mfma_f16x3 bit for bit, and that depthwise output equals
    f32_exact.dwconv_exact, the operand of its float64 reference;
  * the fused stem also agrees with the two-kernel path under the same carried bound;
  * the x4 resize kernel equals the generic kernel's expressions bit for bit: its pure column lerps (h_out = h_in) equal the
    generic kernel's row lerps of the transposed image, and its output at any height equals the generic kernel's vertical
    resize of those column lerps.
Each test prints its case's largest error as a fraction of the bound ("RATIO <id> <fraction>")."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))      # tests/layer_shapes.py, whatever pytest's import mode
import layer_shapes as ls  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cus(dev):
    n = torch.cuda.get_device_properties(dev).multi_processor_count
    print(f"CUS {n}")
    return n


def _up(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _weights(dev, d):
    """the weight tensors of a case in the order of its entry point's pointer arguments"""
    from asr_amd import ops
    c = d.case
    if c.family == "stem":
        return [_up(dev, d.k1), _up(dev, d.b1), ops.pack_pw_weights_f16x3(_up(dev, d.k2.reshape(288, 64))), _up(dev, d.b2)]
    if c.family == "sepconv":
        return [_up(dev, d.wd), _up(dev, d.bd), ops.pack_pw_weights_f16x3(_up(dev, d.wk)), _up(dev, d.bk)]
    if c.family == "conv":
        return [_up(dev, d.k), _up(dev, d.bias)]
    return []


def _launch(dev, d, weights):
    """the case's entry point on d's operands into a prefilled buffer -> the buffer as a numpy array"""
    from asr_amd import _lib
    c = d.case
    x = _up(dev, d.xbuf)
    out = _up(dev, ls.out_buffer(c))
    _lib.call(ls.entry_of(c), *ls.call_args(c, x.data_ptr(), [w.data_ptr() for w in weights], out.data_ptr() + 4 * c.lead), _lib.stream_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _report(case, ratio):
    print(f"RATIO {case.id} {ratio:.3f}")


@pytest.mark.parametrize("id", ls.ids("stem"))
def test_fused_entry_stem(dev, cus, id):
    """walk: 80 x 112 inputs, 3 x 4 tiles per image with a ragged last row and column, more than 2 * CUs tiles -- workgroups of two
    and of three tiles, the LDS image reused between them; small: maps below one tile; ldx = 4 (NaN fourth channel); ldy = 96"""
    from asr_amd import ops
    case = ls.case_by_id("stem", id, cus)
    if case.path == "walk":
        wk = ls.stem_walk(case.b, case.h, case.w, cus)
        assert wk.grid == cus and {len(t) for t in wk.of} == {2, 3}
    d = ls.build(case)
    weights = _weights(dev, d)
    got = ls.read_out(case, _launch(dev, d, weights))
    ratio = ls.check(d, got, "fused")
    xd = _up(dev, d.x)
    mid = ops.conv3x3_direct(xd, weights[0], weights[1], 2, 0, 0, (case.h_out, case.w_out), relu=True, f16x3=True)
    two = ops.conv3x3_mfma(mid, weights[2], weights[3], 64, relu=True, f16x3=True).cpu().numpy()
    _report(case, max(ratio, ls.check(d, two, "two kernels")))
    apart = np.abs(got.astype(np.float64) - two) / d.bound
    print(f"RATIO {case.id}-fused-vs-two-kernels {apart.max():.3f}")
    assert apart.max() <= 1.0


@pytest.mark.parametrize("id", ls.ids("sepconv"))
def test_fused_sepconv(dev, cus, id):
    """walk3 / walk2: 12 x 61 maps (2 x 5 tiles, last row 4, last column 5) with per_wg = 3 / 2 -- the cross-tile prefetch, runs
    across tile-row and image ends, a shorter last run, idle workgroups; small: maps below one tile; every activation pattern;
    ldx = cin + 8 (NaN gap); ldy = 160 at channel 32"""
    from asr_amd import ops
    case = ls.case_by_id("sepconv", id, cus)
    if case.path.startswith("walk"):
        wk = ls.sepconv_walk(case.b, case.h, case.w, case.cin, cus)
        assert wk.per_wg == int(case.path[-1]) and ls.sepconv_run_properties(wk)["idle_workgroup"]
    d = ls.build(case)
    weights = _weights(dev, d)
    got = ls.read_out(case, _launch(dev, d, weights))
    _report(case, ls.check(d, got))
    pre, dw, out = case.act
    xd = _up(dev, d.x)
    ref_dw = ops.dwconv3x3(xd, weights[0], weights[1], stride=1, rate=1, out_hw=(case.h, case.w), pre_relu=pre, post_relu=dw)
    assert np.array_equal(ref_dw.cpu().numpy(), d.a), "asr_dwconv3x3_nhwc_f32 differs from the fma chain"
    m = case.b * case.h * case.w
    two = ops.pwconv(ref_dw.reshape(m, case.cin), weights[2], weights[3], case.cin, case.cout, relu=bool(out), f16x3=True).cpu().numpy()
    diff = got.reshape(m, case.cout).view(np.uint32) != two.view(np.uint32)
    assert not diff.any(), f"{case.id}: {int(diff.sum())} outputs differ from the two-kernel form, first at (pixel, channel) = {tuple(np.argwhere(diff)[0])}"


@pytest.mark.parametrize("id", ls.ids("conv"))
def test_stem_and_direct_conv(dev, cus, id):
    """conv3x3_stem_kernel (VALU), conv3x3_stem_mfma_kernel and conv3x3_direct_kernel: ragged widths, the three paddings, ReLU and
    ReLU6, ldx = 4, ldy = 48, and the second pass of the grid capped at 8192 workgroups (VALU: a last wave with masked groups)"""
    case = ls.case_by_id("conv", id, cus)
    wk = ls.conv_work(case.kernel, case.b, case.h_out, case.w_out, case.cout)
    assert wk.passes == (2 if case.path == "second_pass" else 1)
    d = ls.build(case)
    _report(case, ls.check_buffer(d, _launch(dev, d, _weights(dev, d))))
    if case.relu == 2 and case.path != "second_pass":
        assert min(ls.relu6_reach(d)) >= 1


@pytest.mark.parametrize("id", ls.ids("gap"))
def test_gap(dev, cus, id):
    case = ls.case_by_id("gap", id, cus)
    d = ls.build(case)
    _report(case, ls.check_buffer(d, _launch(dev, d, [])))


@pytest.mark.parametrize("id", ls.ids("resize"))
def test_resize(dev, cus, id):
    from asr_amd import ops
    case = ls.case_by_id("resize", id, cus)
    assert ls.resize_kernel(case.w, case.w_out) == case.kernel
    d = ls.build(case)
    got = ls.read_out(case, _launch(dev, d, []))
    _report(case, ls.check(d, got))
    if case.kernel == "x4":
        xd = _up(dev, d.x)
        cols = ops.resize_bilinear(xd, (case.h, case.w_out))                       # x4 kernel, ty = 0: the column lerps alone
        assert ls.resize_kernel(case.h, case.h) == "generic" and ls.resize_kernel(case.w_out, case.w_out) == "generic"
        rows_t = ops.resize_bilinear(xd.permute(0, 2, 1, 3).contiguous(), (case.w_out, case.h))      # generic kernel, tx = 0, on the transpose
        assert torch.equal(cols.view(torch.int32), rows_t.permute(0, 2, 1, 3).contiguous().view(torch.int32)), \
            "the x4 kernel's column lerp differs from the generic kernel's lerp"
        tall = ops.resize_bilinear(cols, (case.h_out, case.w_out))                 # generic kernel, tx = 0: the row lerp of those
        assert np.array_equal(tall.cpu().numpy().view(np.uint32), got.view(np.uint32)), "x4 differs from generic rows of x4 columns"


@pytest.mark.parametrize("r", ls.REJECTS, ids=[r.id for r in ls.REJECTS])
def test_rejections_return_their_status_and_write_nothing(dev, r):
    """arguments the wrappers refuse before any launch (tests/test_layer_shapes_host.py: each message stands in front of the launch)"""
    from asr_amd import _lib
    lib = _lib.load()
    ptrs = [torch.zeros(1 << 16, device=dev) for _ in range(r.nptr - 1)]
    out = torch.full((1 << 16,), float("nan"), device=dev)
    addr = [p.data_ptr() for p in ptrs] + [out.data_ptr()]
    if r.misalign >= 0:
        addr[r.misalign] += 4
    rc = getattr(lib, r.entry)(*addr, *r.ints, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == r.rc, (rc, lib.asr_last_error())
    assert r.message.encode() in lib.asr_last_error(), lib.asr_last_error()
    assert bool(torch.isnan(out).all())
