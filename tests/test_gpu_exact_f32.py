"""The exact-f32 path (precision="f32", and the range guard's fallback) is exact f32, bit for bit.

1. Bit-exact GEMMs.  v_mfma_f32_32x32x2_f32 is a k-ordered chain of single-rounding f32 fmas, so every output of
   asr_pwconv_mfma_f32 / asr_conv3x3_mfma_f32 is a fixed sequence of f32 roundings that tests/f32_exact.py replays on the
   CPU.  The outputs are compared with np.array_equal on full-mantissa operands spread over 2^-30 .. 2^30, in every tile
   configuration, with tails, padding, the epilogue's options and both store paths.  The order probe
   (test_mfma_chain_order_probe) established the chain order: inside a BK = 32 tile 0,4,1,5,2,6,3,7, 8,12,..., i.e. k0
   (lanes 0-31) before k1 (lanes 32-63) in each MFMA, as the guide to FP32-input MFMA on gfx950 states.  The split-f16
   kernels on the same data are NOT bit-equal to the emulation, so these tests can see the split arithmetic.
2. 2^k equivariance.  Rounding commutes with scaling by s = 2^k while nothing overflows or becomes subnormal, and ReLU,
   zero padding, max, mean, bilinear weights and BN folding are positively homogeneous.  Every exact-f32 entry point (and
   the precision="f32" model) run on (s*x, s*bias-like parameters) must return exactly s * its output at s = 1, for
   s in {2^-40, 2^-9, 2^11, 2^40}.  Margin: the data are O(1) normal deviates (|x| >= 2^-24 in practice) times weights of
   O(0.1-1), so at s = 2^-40 the smallest products sit near 2^-80, 2^46 above f32's smallest normal 2^-126, and at s = 2^40
   the largest sums stay below 2^60, far under 2^128.  ReLU6 is not homogeneous: it is excluded (relu = 2, MobileNetV2).
   The split-f16 counterparts fail the same check at 2^+-40 (f16 saturates at 65504; lo and hi go subnormal).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))      # tests/f32_exact.py, whatever pytest's import mode
import f32_exact as fx  # noqa: E402

pytestmark = pytest.mark.gpu

SCALES = (2.0 ** -40, 2.0 ** -9, 2.0 ** 11, 2.0 ** 40)


def _bits_equal(got, ref):
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    return got.shape == ref.shape and np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def _assert_bits_equal(got, ref):
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    diff = got.view(np.uint32) != ref.view(np.uint32)
    if diff.any():
        i = np.argwhere(diff)[0]
        raise AssertionError(f"{int(diff.sum())} of {diff.size} outputs differ from the fmaf chain; first at {tuple(i)}: "
                             f"got {got[tuple(i)]!r} expected {ref[tuple(i)]!r}")


def _operands(rng, m, k, n):
    """Full-mantissa A [m,k] and W [k,n]: elements over 2^-4 .. 2^4 times per-row scales 2^-30 .. 2^30 (A) and per-column
    scales 2^-8 .. 2^8 (W); products between 2^-46 and 2^46, no subnormal, no overflow."""
    x = fx.wide_range(rng, (m, k), -4, 4) * np.ldexp(np.float32(1), rng.integers(-30, 31, (m, 1))).astype(np.float32)
    w = fx.wide_range(rng, (k, n), -4, 4) * np.ldexp(np.float32(1), rng.integers(-8, 9, (1, n))).astype(np.float32)
    return x.astype(np.float32), w.astype(np.float32)


def _pw(x, w, bias=None, relu=0, res=None, f16x3=False, **kw):
    from asr_amd import ops
    wd = ops.to_device(w)
    wp = ops.pack_pw_weights_f16x3(wd) if f16x3 else ops.pack_pw_weights(wd)
    k, n = w.shape
    return ops.pwconv(ops.to_device(x), wp, None if bias is None else ops.to_device(bias), k, n, relu=relu,
                      residual=None if res is None else ops.to_device(res), f16x3=f16x3, **kw).cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# 1. bit-exact GEMMs
# ---------------------------------------------------------------------------------------------------------------------
def test_mfma_chain_order_probe(dev):
    """K = 8 (padded to 32) with cancelling products.  Row 0: a*b = 1, -1, 2^-30, 2^-30 at k = 0, 1, 4, 5: the k0-first chain
    (0,4,1,5,..) gives 2^-30, the natural order 2^-29, the k1-first chain (4,0,5,1,..) 0.  The other rows are random
    wide-range products on which the three orders disagree too.  Observed: the k0-first chain, bit for bit."""
    rng = np.random.default_rng(100)
    m, k, n = 64, 8, 32
    x = fx.wide_range(rng, (m, k), -30, 0)
    w = fx.wide_range(rng, (k, n), -8, 0)
    x[0] = [1, -1, 0, 0, 2.0 ** -30, 2.0 ** -30, 0, 0]
    w[:, 0] = 1
    candidates = {f: fx.gemm_chain(x, w, fx.kernel_k_order(k, f)) for f in ("k0", "k1", "natural")}
    assert candidates["k0"][0, 0] == 2.0 ** -30 and candidates["natural"][0, 0] == 2.0 ** -29 and candidates["k1"][0, 0] == 0
    # the probe discriminates: the orders give different bits on many outputs (about 30 %)
    assert np.mean(candidates["k0"] != candidates["k1"]) > 0.1 and np.mean(candidates["k0"] != candidates["natural"]) > 0.1
    got = _pw(x, w)
    _assert_bits_equal(got, candidates["k0"])


@pytest.mark.parametrize("m,k,n,bias,relu,res", [
    (200, 64, 21, True, 0, False),        # <4,1,1,1> (N <= 32), M tail, N % 4 != 0: the scalar store path
    (300, 100, 32, False, 1, True),       # K = 3 tiles + 4 (zero-padded k), no bias, residual
    (130, 36, 48, True, 2, False),        # <2,2,2,1> (N <= 64), ReLU6, K = 36
    (257, 256, 64, True, 1, True),        # <2,2,2,1>, M tail of one row, residual
    (190, 520, 200, True, 0, True),       # <2,2,2,2>, N tail inside the 128-wide tile, K % 32 = 8
    (129, 1024, 130, False, 1, False),    # <2,2,2,2>, two N tiles, N % 4 != 0, K = 1024
])
def test_pwconv_f32_is_the_fmaf_chain(dev, m, k, n, bias, relu, res):
    rng = np.random.default_rng(m * 7 + k + n)
    x, w = _operands(rng, m, k, n)
    b = fx.wide_range(rng, n, 0, 40) if bias else None
    r = fx.wide_range(rng, (m, n), 0, 40) if res else None
    ref = fx.pwconv_exact(x, w, b, relu, r)
    _assert_bits_equal(_pw(x, w, b, relu, r), ref)


@pytest.mark.parametrize("n,off,total_c", [(40, 16, 72), (21, 3, 30)])
def test_pwconv_f32_strided_rows_into_a_channel_slice_is_the_fmaf_chain(dev, n, off, total_c):
    """sub_stride = 2 with h_in / w_in (odd sizes), written into columns [off, off + n) of a wider row: vector stores
    (n = 40 at a 16-byte aligned offset) and the scalar path (n = 21 at offset 3); the other columns stay untouched."""
    from asr_amd import ops, _lib
    rng = np.random.default_rng(11 + n)
    b, h, w_, k = 2, 13, 10, 64
    ho, wo = 7, 5
    x4, wt = _operands(rng, b * h * w_, k, n)
    x4 = x4.reshape(b, h, w_, k)
    bias = fx.wide_range(rng, n, 0, 40)
    ref = fx.pwconv_exact(x4[:, ::2, ::2].reshape(-1, k), wt, bias, relu=1)
    out = torch.full((b * ho * wo, total_c), -7.0, device=dev)
    xd, wp, bd = ops.to_device(x4), ops.pack_pw_weights(ops.to_device(wt)), ops.to_device(bias)
    _lib.call("asr_pwconv_mfma_f32", xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), None, out.data_ptr() + 4 * off,
              b * ho * wo, k, n, k, total_c, 0, 1, 2, h, w_, _lib.stream_ptr())
    got = out.cpu().numpy()
    _assert_bits_equal(got[:, off:off + n], ref)
    assert np.all(got[:, :off] == -7.0) and np.all(got[:, off + n:] == -7.0)


@pytest.mark.parametrize("b,h,w_,cin,cout,stride,pad,dil,relu", [
    (2, 11, 13, 32, 21, 1, 1, 1, 1),      # CONV <4,1,1,1>, ragged map
    (2, 12, 9, 64, 48, 2, 1, 1, 0),       # CONV <2,2,2,1>, stride 2
    (1, 15, 14, 32, 64, 1, 2, 2, 1),      # CONV <2,2,2,1>, dilation 2
    (2, 9, 10, 32, 160, 2, 3, 3, 0),      # CONV <2,2,2,2>, two N tiles, stride 2, dilation 3
])
def test_conv3x3_mfma_f32_is_the_fmaf_chain(dev, b, h, w_, cin, cout, stride, pad, dil, relu):
    from asr_amd import ops
    rng = np.random.default_rng(b * 1000 + h * 10 + cout)
    pix = np.ldexp(np.float32(1), rng.integers(-30, 31, (b, h, w_, 1))).astype(np.float32)   # per-pixel scales 2^+-30
    x = (fx.wide_range(rng, (b, h, w_, cin), -4, 4) * pix).astype(np.float32)
    wk = _operands(rng, 1, 9 * cin, cout)[1]
    bias = fx.wide_range(rng, cout, 0, 40)
    ref = fx.conv3x3_exact(x, wk.reshape(3, 3, cin, cout), bias, stride, pad, dil, relu)
    got = ops.conv3x3_mfma(ops.to_device(x), ops.pack_pw_weights(ops.to_device(wk)), ops.to_device(bias), cout, stride=stride,
                           pad=pad, dil=dil, relu=relu).cpu().numpy()
    _assert_bits_equal(got, ref)


def test_identity_probes_return_the_other_operand_bit_for_bit(dev):
    """A = I returns W and W = I returns A, on full-mantissa values over 2^-60 .. 2^60 (one nonzero product per chain);
    for the implicit GEMM a centre-tap identity kernel returns x, and one-hot pixels return every tap of W."""
    from asr_amd import ops
    rng = np.random.default_rng(5)
    k, n = 160, 136
    w = fx.wide_range(rng, (k, n), -60, 60)
    assert _bits_equal(_pw(np.eye(k, dtype=np.float32), w), w)
    x = fx.wide_range(rng, (300, 96), -60, 60)
    assert _bits_equal(_pw(x, np.eye(96, dtype=np.float32)), x)
    cin = 32
    xi = fx.wide_range(rng, (2, 7, 9, cin), -60, 60)
    eye9 = np.zeros((3, 3, cin, cin), np.float32)
    eye9[1, 1] = np.eye(cin)
    got = ops.conv3x3_mfma(ops.to_device(xi), ops.pack_pw_weights(ops.to_device(eye9.reshape(9 * cin, cin))), None, cin)
    assert _bits_equal(got.cpu().numpy(), xi)
    w9 = fx.wide_range(rng, (3, 3, cin, 64), -60, 60)
    onehot = np.zeros((cin, 3, 3, cin), np.float32)
    onehot[np.arange(cin), 1, 1, np.arange(cin)] = 1
    got = ops.conv3x3_mfma(ops.to_device(onehot), ops.pack_pw_weights(ops.to_device(w9.reshape(9 * cin, 64))), None, 64).cpu().numpy()
    # out[b, oy, ox] = w9[2 - oy, 2 - ox, b]
    assert _bits_equal(got[:, ::-1, ::-1].transpose(1, 2, 0, 3), w9)


def test_split_f16_kernels_are_not_the_fmaf_chain(dev):
    """Non-vacuity: on the same wide-range data the split-f16 GEMMs (direct and pre-split operand) differ from the exact
    chain -- the bit-exact tests above would see a kernel that quietly ran the split arithmetic."""
    from asr_amd import ops
    rng = np.random.default_rng(6)
    m, k, n = 256, 256, 256
    x, w = _operands(rng, m, k, n)
    ref = fx.pwconv_exact(x, w)
    assert _bits_equal(_pw(x, w), ref)
    assert not _bits_equal(_pw(x, w, f16x3=True), ref)
    # pre-split operand: the depthwise kernel's split output against the same depthwise output in f32
    xs = (fx.wide_range(rng, (1, 16, 32, 64), -4, 4) * np.float32(2.0 ** 12)).astype(np.float32)
    wd = ops.to_device((rng.standard_normal((3, 3, 64)) * 0.3).astype(np.float32))
    bd = ops.to_device(np.zeros(64, np.float32))
    xsd = ops.to_device(xs)
    dw = ops.dwconv3x3(xsd, wd, bd).cpu().numpy().reshape(-1, 64)
    split, _shape, chunks = ops.dwconv3x3_split(xsd, wd, bd)
    w2 = _operands(rng, 1, 64, 256)[1]
    got = ops.pwconv_presplit(split, ops.pack_pw_weights_f16x3(ops.to_device(w2)), None, 64, 256, chunks).cpu().numpy()
    ref2 = fx.pwconv_exact(dw, w2)
    assert _bits_equal(_pw(dw, w2), ref2)
    assert not _bits_equal(got, ref2)


# ---------------------------------------------------------------------------------------------------------------------
# 2. 2^k equivariance
# ---------------------------------------------------------------------------------------------------------------------
def _outputs(r):
    return list(r) if isinstance(r, (tuple, list)) else [r]


def _equivariant_at(fn, s, base=None):
    """fn(s) -> tensor(s) computed on s-scaled inputs; True if every output is exactly s * fn(1)."""
    base = base if base is not None else _outputs(fn(1.0))
    got = _outputs(fn(s))
    return all(torch.equal(g, b * s) for g, b in zip(got, base))


def _assert_equivariant(fn, scales=SCALES):
    base = _outputs(fn(1.0))
    for b in base:
        assert torch.count_nonzero(b) > b.numel() // 4, "vacuous: the output is mostly zeros"
    for s in scales:
        got = _outputs(fn(s))
        for i, (g, b) in enumerate(zip(got, base)):
            if not torch.equal(g, b * s):
                d = (g != b * s)
                raise AssertionError(f"output {i} at s = 2^{int(np.log2(s))}: {int(d.sum())} of {d.numel()} values are not "
                                     f"s * out(1)")


def _rn(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


@pytest.mark.parametrize("relu,res", [(0, True), (1, False)])
@pytest.mark.parametrize("n", [24, 48, 200])
def test_pwconv_f32_is_power_of_two_equivariant(dev, n, relu, res):
    from asr_amd import ops
    rng = np.random.default_rng(n + relu)
    m, k = 333, 100
    x, w, b, r = _rn(rng, m, k), _rn(rng, k, n, scale=0.1), _rn(rng, n), _rn(rng, m, n)
    xd, bd, rd = ops.to_device(x), ops.to_device(b), ops.to_device(r)
    wp = ops.pack_pw_weights(ops.to_device(w))
    _assert_equivariant(lambda s: ops.pwconv(xd * s, wp, bd * s, k, n, relu=relu, residual=rd * s if res else None))


@pytest.mark.parametrize("cout,stride,dil", [(21, 1, 1), (64, 2, 1), (160, 1, 2)])
def test_conv3x3_mfma_f32_is_power_of_two_equivariant(dev, cout, stride, dil):
    from asr_amd import ops
    rng = np.random.default_rng(cout)
    x, w, b = _rn(rng, 2, 13, 11, 32), _rn(rng, 9 * 32, cout, scale=0.1), _rn(rng, cout)
    xd, bd, wp = ops.to_device(x), ops.to_device(b), ops.pack_pw_weights(ops.to_device(w))
    _assert_equivariant(lambda s: ops.conv3x3_mfma(xd * s, wp, bd * s, cout, stride=stride, pad=dil, dil=dil, relu=True))


@pytest.mark.parametrize("stride,pad", [(2, 0), (1, 1)])
def test_conv3x3_direct_f32_is_power_of_two_equivariant(dev, stride, pad):
    """entry_flow_conv1_1: TF-SAME stride 2 on an even input (pad bottom/right only), and stride 1."""
    from asr_amd import ops
    rng = np.random.default_rng(13 + stride)
    h, w_ = 32, 46
    x, k, b = _rn(rng, 2, h, w_, 3), _rn(rng, 3, 3, 3, 32, scale=0.3), _rn(rng, 32)
    out_hw = (h // stride, w_ // stride)
    xd, kd, bd = ops.to_device(x), ops.to_device(k), ops.to_device(b)
    _assert_equivariant(lambda s: ops.conv3x3_direct(xd * s, kd, bd * s, stride, pad, pad, out_hw, relu=True))


_DW_CASES = [(mode, stride, rate, h) for mode in (0, 1, 2)
             for stride, rate, h in ((1, 1, 16), (1, 1, 20), (1, 2, 16), (2, 1, 32), (2, 1, 38))] + \
            [(mode, 1, 6, 16) for mode in (0, 1)]          # rate 6: direct only (the streaming form is not built for it)


@pytest.mark.parametrize("mode,stride,rate,h", _DW_CASES)
@pytest.mark.parametrize("pre,post", [(True, False), (False, True)])
def test_dwconv3x3_f32_is_power_of_two_equivariant(dev, mode, stride, rate, h, pre, post):
    """Every kernel of asr_dwconv3x3_nhwc_f32: auto / direct / streaming (full 16-row strips and ragged ones); the
    streaming form exists for (stride 1, rate 1|2) and (stride 2, rate 1)."""
    from asr_amd import ops
    rng = np.random.default_rng(stride * 100 + rate * 10 + h)
    c = 72
    x, k, b = _rn(rng, 2, h, 24, c), _rn(rng, 3, 3, c, scale=0.3), _rn(rng, c)
    xd, kd, bd = ops.to_device(x), ops.to_device(k), ops.to_device(b)
    out_hw = None if stride == 1 else ((h + 2 - 3) // 2 + 1, (24 + 2 - 3) // 2 + 1)
    pad = rate if stride == 1 else 1
    _assert_equivariant(lambda s: ops.dwconv3x3(xd * s, kd, bd * s, stride=stride, rate=rate, pad_top=pad, pad_left=pad,
                                                out_hw=out_hw, pre_relu=pre, post_relu=post, force_direct=mode))


@pytest.mark.parametrize("h,w_,c,rates,pre,post", [
    (16, 24, 72, (6, 12, 18), False, True),
    (33, 45, 40, (2, 4, 6), True, False),
])
def test_aspp_dwconv3_f32_is_power_of_two_equivariant(dev, h, w_, c, rates, pre, post):
    from asr_amd import ops
    rng = np.random.default_rng(h + c)
    x, k3, b3 = _rn(rng, 2, h, w_, c), _rn(rng, 3, 3, 3, c, scale=0.3), _rn(rng, 3, c)
    xd, kd, bd = ops.to_device(x), ops.to_device(k3), ops.to_device(b3)
    _assert_equivariant(lambda s: ops.aspp_dwconv3(xd * s, kd, bd * s, rates=rates, pre_relu=pre, post_relu=post))


def test_gap_f32_is_power_of_two_equivariant(dev):
    from asr_amd import ops
    xd = ops.to_device(_rn(np.random.default_rng(1), 3, 13, 17, 260))
    _assert_equivariant(lambda s: ops.gap(xd * s))


@pytest.mark.parametrize("hw_in,hw_out", [((7, 9), (13, 20)),      # generic kernel
                                          ((16, 24), (64, 96)),    # the x4 kernel (w_out == 4 * w_in)
                                          ((1, 1), (16, 24))])     # 1 x 1 broadcast (image pooling)
def test_resize_bilinear_f32_is_power_of_two_equivariant(dev, hw_in, hw_out):
    from asr_amd import ops
    xd = ops.to_device(_rn(np.random.default_rng(2), 2, hw_in[0], hw_in[1], 24))
    _assert_equivariant(lambda s: ops.resize_bilinear(xd * s, hw_out))


def _tfs(rng, n, h, w):
    from asr_amd import transforms as T
    ang = rng.uniform(-0.4, 0.4, n).astype(np.float32)
    sh = rng.uniform(-6, 6, (n, 2)).astype(np.float32)
    return T.rotation_transforms(ang, h, w), T.translation_transforms(sh)


@pytest.mark.parametrize("interpolation", ["bilinear", "nearest"])
def test_warp_affine_f32_is_power_of_two_equivariant(dev, interpolation):
    from asr_amd import ops
    rng = np.random.default_rng(3)
    img = _rn(rng, 4, 32, 40, 3)
    rot, _tr = _tfs(rng, 4, 32, 40)
    imgd, tfd = ops.to_device(img), ops.to_device(rot)
    _assert_equivariant(lambda s: ops.warp_affine(imgd * s, tfd, out_hw=(30, 41), interpolation=interpolation))


def test_augment_copies_f32_is_power_of_two_equivariant(dev):
    from asr_amd import ops
    rng = np.random.default_rng(4)
    img = _rn(rng, 48, 40, 3)
    rot, tr = _tfs(rng, 6, 48, 40)
    imgd, rd, td = ops.to_device(img), ops.to_device(rot), ops.to_device(tr)
    _assert_equivariant(lambda s: ops.augment_copies(imgd * s, rd, td))


def _sr_tfs(rng, b, n, H):
    """[b, n, 8] rotation and translation transforms on the device."""
    from asr_amd import ops
    pairs = [_tfs(rng, n, H, H) for _ in range(b)]
    return ops.to_device(np.stack([p[0] for p in pairs])), ops.to_device(np.stack([p[1] for p in pairs]))


@pytest.mark.parametrize("mode", ["max", "mean", "both"])
def test_realign_f32_is_power_of_two_equivariant(dev, mode):
    from asr_amd import ops
    rng = np.random.default_rng(5)
    b, n, H, h = 2, 5, 64, 16
    yd = ops.to_device(_rn(rng, b, n, h, h))
    rot, tr = _sr_tfs(rng, b, n, H)
    _assert_equivariant(lambda s: ops.realign(yd * s, tr, rot, (H, H), mode))


def test_sr_forward_residual_f32_is_power_of_two_equivariant(dev):
    from asr_amd import ops
    rng = np.random.default_rng(6)
    b, n, H, h = 2, 5, 64, 16
    xd, yd = ops.to_device(_rn(rng, b, H, H)), ops.to_device(_rn(rng, b, n, h, h))
    rot, tr = _sr_tfs(rng, b, n, H)
    _assert_equivariant(lambda s: ops.sr_forward_residual(xd * s, yd * s, rot, tr))


@pytest.mark.parametrize("os_", [16, 8])
def test_f32_model_is_power_of_two_equivariant(dev, os_):
    """The whole precision="f32" Xception DeepLabV3+ (synthetic weights, 64 x 96, batch 2): input and every bias-like
    parameter (BN beta / moving mean, conv biases) scaled by 2^k -> logits scaled by exactly 2^k.  MobileNetV2 is not
    covered: its ReLU6 is not positively homogeneous."""
    from asr_amd import weights as W
    from asr_amd.model import DeeplabModel
    w = W.make_synthetic_weights(1234, 21)
    x = np.random.default_rng(21).random((2, 64, 96, 3), dtype=np.float32)

    def run(s):
        m = DeeplabModel(fx.scaled(w, s), (64, 96, 3), 21, final_upsample=False, last_activation=None, precision="f32", OS=os_)
        return m.predict_device(x * np.float32(s), batch_size=2)
    _assert_equivariant(run)


# ---- non-vacuity: the split-f16 arithmetic fails the same check ----------------------------------------------------
def test_split_f16_entry_points_are_not_power_of_two_equivariant(dev):
    from asr_amd import ops
    rng = np.random.default_rng(7)
    m, k, n = 333, 128, 256
    xd, bd = ops.to_device(_rn(rng, m, k)), ops.to_device(_rn(rng, n))
    wp16 = ops.pack_pw_weights_f16x3(ops.to_device(_rn(rng, k, n, scale=0.1)))
    xs, k1, b1 = ops.to_device(_rn(rng, 2, 32, 48, 3)), ops.to_device(_rn(rng, 3, 3, 3, 32, scale=0.3)), ops.to_device(_rn(rng, 32))
    w2 = ops.pack_pw_weights_f16x3(ops.to_device(_rn(rng, 288, 64, scale=0.08)))
    b2 = ops.to_device(_rn(rng, 64))
    xc, wdw, bdw = ops.to_device(_rn(rng, 2, 16, 24, 64)), ops.to_device(_rn(rng, 3, 3, 64, scale=0.3)), ops.to_device(_rn(rng, 64))
    wpw = ops.pack_pw_weights_f16x3(ops.to_device(_rn(rng, 64, 128, scale=0.1)))
    bpw = ops.to_device(_rn(rng, 128))
    fns = {
        "asr_pwconv_mfma_f16x3": lambda s: ops.pwconv(xd * s, wp16, bd * s, k, n, f16x3=True),
        "asr_entry_stem_f16x3": lambda s: ops.entry_stem_fused(xs * s, k1, b1 * s, w2, b2 * s),
        "asr_sepconv_fused_f16x3": lambda s: ops.sepconv_fused(xc * s, wdw, bdw * s, wpw, bpw * s, 128, pre_relu=True),
    }
    for name, fn in fns.items():
        base = _outputs(fn(1.0))
        for s in (2.0 ** 40, 2.0 ** -40):
            assert not _equivariant_at(fn, s, base), f"{name} is bit-equivariant at s = 2^{int(np.log2(s))}"


def test_split_f16_model_is_not_power_of_two_equivariant(dev):
    from asr_amd import weights as W
    from asr_amd.model import DeeplabModel
    w = W.make_synthetic_weights(1234, 21)
    x = np.random.default_rng(21).random((2, 64, 96, 3), dtype=np.float32)

    def run(s):
        m = DeeplabModel(fx.scaled(w, s), (64, 96, 3), 21, final_upsample=False, last_activation=None, precision="f16x3")
        return m.predict_device(x * np.float32(s), batch_size=2)
    base = _outputs(run(1.0))
    for s in (2.0 ** 40, 2.0 ** -40):
        assert not _equivariant_at(run, s, base)
