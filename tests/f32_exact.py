"""Bit-exact CPU replay of the exact-f32 GEMM (csrc/gemm.hip, pw_gemm_kernel) and the 2^k scaling helper of the exact-f32
equivariance tests.  Test infrastructure only (a plain module, imported by tests/test_f32_exact.py and
tests/test_gpu_exact_f32.py).

On gfx950 v_mfma_f32_32x32x2_f32 is a k-ordered chain of single-rounding f32 fmas per output element: no wider internal
accumulation, subnormals kept.  pw_gemm_kernel starts every accumulator at +0.0, walks its K-tiles in order (no split-K),
and within a BK = 32 tile issues 16 MFMAs (kk = 0..3, t = 0..3) whose lanes 0-31 carry k0 = 8*kk + t and lanes 32-63
k1 = 8*kk + 4 + t.  With k0 accumulated before k1 (what tests/test_gpu_exact_f32.py::test_mfma_chain_order_probe
establishes on the device) the chain order inside a tile is 0,4,1,5,2,6,3,7, 8,12,9,13, ...; the zero-padded k of the
last tile are fmas with a zero product.  The epilogue is ((acc + bias) -> ReLU -> ReLU6) + residual, one f32 rounding per
add (gemm_common.h, pw_epilogue).

The depthwise kernels (csrc/dwconv.hip) are one nine-step fmaf chain from the bias per output, taps in (ky, kx) order:
dwconv_exact; split_f16_exact restates the hi / lo split of their split-f16 outputs (tests/dw_shapes.py builds on both).
"""
from __future__ import annotations

import numpy as np

BK = 32


def fmaf(a, b, c):
    """Correctly rounded f32 fused multiply-add, vectorised (broadcasting) over numpy arrays.

    The product of two f32 is exact in f64 (48 <= 53 bits).  s = fl64(p + c) and its rounding error e (TwoSum) represent
    p + c exactly.  Rounding s to f32 is then correct unless s sits exactly on a midpoint of two f32 neighbours while e != 0
    (double rounding): the true sum lies on the side of e, so the neighbour on that side is the answer.  Finite inputs and
    results only."""
    a = np.asarray(a, np.float32).astype(np.float64)
    b = np.asarray(b, np.float32).astype(np.float64)
    c = np.asarray(c, np.float32).astype(np.float64)
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    r = s.astype(np.float32)
    r64 = r.astype(np.float64)
    towards = np.nextafter(r, np.where(s > r64, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
    mid = (r64 + towards.astype(np.float64)) * 0.5
    fix = (s != r64) & (s == mid) & (e != 0)
    if np.any(fix):
        # s on a midpoint: e > 0 means the exact sum is above it, so the upper neighbour is the correct rounding
        upper = np.maximum(r, towards)
        lower = np.minimum(r, towards)
        r = np.where(fix, np.where(e > 0, upper, lower), r)
    return np.asarray(r, np.float32)


def naive_fmaf(a, b, c):
    """float32(a*b + c) evaluated in f64: wrong exactly in the double-rounding midpoint cases."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def kernel_k_order(k, first="k0"):
    """The order in which pw_gemm_kernel feeds k into each output's fma chain, over the K padded to BK (entries >= k are the
    zero padding).  first="k1" / "natural": the alternatives the order probe rules out."""
    kpad = -(-k // BK) * BK
    if first == "natural":
        return np.arange(kpad)
    order = []
    for kt in range(kpad // BK):
        for kk in range(4):
            for t in range(4):
                k0, k1 = kt * BK + 8 * kk + t, kt * BK + 8 * kk + 4 + t
                order += [k0, k1] if first == "k0" else [k1, k0]
    return np.asarray(order)


def gemm_chain(x, w, k_order):
    """acc[m, n] = the fmaf chain over k in k_order of x[m, k] * w[k, n], from +0.0; k >= K are zero products (padding)."""
    x = np.asarray(x, np.float32)
    w = np.asarray(w, np.float32)
    m, kdim = x.shape
    acc = np.zeros((m, w.shape[1]), np.float32)
    zero = np.float32(0.0)
    for k in k_order:
        if k < kdim:
            acc = fmaf(x[:, k:k + 1], w[k:k + 1, :], acc)
        else:
            acc = fmaf(zero, zero, acc)
    return acc


def epilogue(acc, bias=None, relu=0, residual=None):
    """pw_epilogue: v = acc + bias (+0.0 without a bias); relu >= 1: max(v, 0); relu == 2: min(v, 6); then v + residual."""
    v = np.asarray(acc, np.float32) + (np.asarray(bias, np.float32) if bias is not None else np.float32(0.0))
    if relu:
        v = np.maximum(v, np.float32(0.0))
    if relu == 2:
        v = np.minimum(v, np.float32(6.0))
    if residual is not None:
        v = v + np.asarray(residual, np.float32)
    return v.astype(np.float32)


def pwconv_exact(x, w, bias=None, relu=0, residual=None):
    """What asr_pwconv_mfma_f32 must return, bit for bit, for rows x [M, K] and W [K, N]."""
    return epilogue(gemm_chain(x, w, kernel_k_order(x.shape[1])), bias, relu, residual)


def im2col3x3(x, stride, pad, dil, h_out, w_out):
    """x [B,H,W,C] -> [B*h_out*w_out, 9*C] with k = (dy*3 + dx)*C + c (the implicit GEMM's k); out-of-image taps are 0."""
    b, h, w, c = x.shape
    xp = np.zeros((b, h + 2 * pad + (h_out * stride + 2 * dil), w + 2 * pad + (w_out * stride + 2 * dil), c), np.float32)
    xp[:, pad:pad + h, pad:pad + w] = x
    cols = []
    for dy in range(3):
        for dx in range(3):
            ys, xs = dy * dil, dx * dil
            cols.append(xp[:, ys:ys + (h_out - 1) * stride + 1:stride, xs:xs + (w_out - 1) * stride + 1:stride])
    return np.concatenate(cols, axis=-1).reshape(b * h_out * w_out, 9 * c)


def conv3x3_exact(x, w_hwio, bias, stride, pad, dil, relu=0):
    """What asr_conv3x3_mfma_f32 must return, bit for bit: x [B,H,W,cin], w [3,3,cin,cout] -> [B,Ho,Wo,cout]."""
    b, h, w, cin = x.shape
    cout = w_hwio.shape[-1]
    ho = (h + 2 * pad - (2 * dil + 1)) // stride + 1
    wo = (w + 2 * pad - (2 * dil + 1)) // stride + 1
    a = im2col3x3(np.asarray(x, np.float32), stride, pad, dil, ho, wo)
    y = epilogue(gemm_chain(a, np.asarray(w_hwio, np.float32).reshape(9 * cin, cout), kernel_k_order(9 * cin)), bias, relu)
    return y.reshape(b, ho, wo, cout)


def wide_range(rng, shape, lo=-30, hi=30):
    """Full-mantissa f32 values (random low-order bits) of random sign over 2^lo .. 2^hi, exponent uniform per element."""
    mant = rng.uniform(1.0, 2.0, shape)
    return (np.sign(rng.standard_normal(shape)) * np.ldexp(mant, rng.integers(lo, hi + 1, shape))).astype(np.float32)


BIAS_LIKE = ("/beta", "/moving_mean", "/bias")


def scaled(weights, s):
    """A weight dict whose bias-like parameters (BN beta and moving mean, conv biases) are multiplied by s = 2^k: with the
    input also scaled by s, every activation of a ReLU network scales by s (BN folding: b - m * scale commutes)."""
    s = np.float32(s)
    return {k: (np.asarray(v, np.float32) * s if k.endswith(BIAS_LIKE) else v) for k, v in weights.items()}


# ---- depthwise 3x3 (csrc/dwconv.hip): one fmaf chain per output, from the bias, over the taps in (ky, kx) order -------------
TAPS = tuple((ky, kx) for ky in range(3) for kx in range(3))


def _tap_range(n_out, n_in, stride, pad, off):
    """The outputs o in [0, n_out) whose tap o * stride - pad + off lies inside [0, n_in): (first o, one past the last o)."""
    lo = max(0, -(-(pad - off) // stride))
    hi = min(n_out, (n_in - 1 + pad - off) // stride + 1)
    return lo, max(hi, lo)


def dwconv_exact(x, w, bias, stride, rate, pad_top, pad_left, out_hw, pre_relu=0, post_relu=0, rows=None, taps=TAPS, fma=fmaf):
    """What every depthwise kernel must return, bit for bit: x [B,H,W,C], w [3,3,C], bias [C] -> [B,h_out,w_out,C] with
    acc = bias; for (ky, kx) row-major: acc = fmaf(act(x[oy*stride - pad_top + ky*rate, ox*stride - pad_left + kx*rate]), w[ky, kx], acc),
    a tap outside the image skipped (a zero tap value, or a zero weight on a finite value, leaves acc unchanged as well);
    act = ReLU if pre_relu; then post_relu 1: max(acc, 0), 2: min(max(acc, 0), 6).
    rows = (r0, r1): output rows r0 .. r1 - 1 only.  taps / fma: the tap order and the multiply-add, for tests that need a
    deliberately different chain (fma is called once per tap, in order)."""
    x = np.asarray(x, np.float32)
    w = np.asarray(w, np.float32)
    b, h, wd, c = x.shape
    ho, wo = out_hw
    r0, r1 = rows if rows is not None else (0, ho)
    if pre_relu:
        x = np.maximum(x, np.float32(0.0))
    acc = np.broadcast_to(np.asarray(bias, np.float32), (b, r1 - r0, wo, c)).copy()
    for ky, kx in taps:
        ya, yb = _tap_range(ho, h, stride, pad_top, ky * rate)
        ya, yb = max(ya, r0), max(min(yb, r1), max(ya, r0))
        xa, xb = _tap_range(wo, wd, stride, pad_left, kx * rate)
        iy0, ix0 = ya * stride - pad_top + ky * rate, xa * stride - pad_left + kx * rate
        xv = x[:, iy0:iy0 + (yb - ya - 1) * stride + 1:stride, ix0:ix0 + (xb - xa - 1) * stride + 1:stride] if yb > ya and xb > xa \
            else np.zeros((b, 0, 0, c), np.float32)
        region = (slice(None), slice(ya - r0, ya - r0 + xv.shape[1]), slice(xa, xa + xv.shape[2]))
        acc[region] = fma(xv, w[ky, kx], acc[region])
    if post_relu:
        acc = np.maximum(acc, np.float32(0.0))
    if post_relu == 2:
        acc = np.minimum(acc, np.float32(6.0))
    return acc


F16_MAX = np.float32(65504.0)


def split_f16_exact(v):
    """asr_split_f16 (csrc/asr_common.h) restated: hi = f16(clip(v, +-65504)), lo = f16(clip(v - f32(hi), +-65504)), the
    subtraction in float32, both conversions round-to-nearest-even with f16 subnormals kept -> (hi, lo) as uint16 bit patterns."""
    v = np.asarray(v, np.float32)
    hi = np.clip(v, -F16_MAX, F16_MAX).astype(np.float16)
    lo = np.clip(v - hi.astype(np.float32), -F16_MAX, F16_MAX).astype(np.float16)
    return hi.view(np.uint16), lo.view(np.uint16)
