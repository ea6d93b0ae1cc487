"""The CPU emulation behind the bit-exact GPU tests (tests/f32_exact.py): fmaf against glibc's, the fma chain against a
scalar loop, the k order of pw_gemm_kernel, and the weight-scaling helper against the CPU oracle."""
import ctypes
import ctypes.util
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))      # tests/f32_exact.py, whatever pytest's import mode
import f32_exact as fx  # noqa: E402


@pytest.fixture(scope="module")
def libm_fmaf():
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    f = libm.fmaf
    f.restype = ctypes.c_float
    f.argtypes = [ctypes.c_float, ctypes.c_float, ctypes.c_float]
    return lambda a, b, c: np.array([f(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], np.float32)


def _midpoint_cases(rng, n):
    """a*b + c whose exact value lies a hair off an f32 midpoint, so close that the f64 sum lands ON it: c = r or its upper
    neighbour, a*b = +-ulp(r)/2 * (1 - u^2 2^-46) with a = ulp/2 * (1 + u 2^-23), b = 1 - u 2^-23 (both exact in f32)."""
    r = np.abs(fx.wide_range(rng, n, -40, 40))
    half = np.spacing(r).astype(np.float64) / 2.0
    u = rng.integers(1, 1 << 11, n).astype(np.float64)
    a = (half * (1.0 + u * 2.0 ** -23)).astype(np.float32)
    b = (1.0 - u * 2.0 ** -23).astype(np.float32)
    up = rng.random(n) < 0.5                                   # c above the midpoint, a*b negative: exact sum just above it
    c = np.where(up, np.nextafter(r, np.float32(np.inf)), r).astype(np.float32)
    a = np.where(up, -a, a).astype(np.float32)
    neg = rng.random(n) < 0.5                                  # and the mirror image below zero
    return np.where(neg, -a, a), b, np.where(neg, -c, c).astype(np.float32)


def test_fmaf_matches_glibc_on_wide_random_operands(libm_fmaf):
    rng = np.random.default_rng(0)
    n = 200_000
    a, b, c = (fx.wide_range(rng, n, -60, 60) for _ in range(3))
    # plus cancelling ones: c close to -a*b, where the result is the rounding error of the product
    a2, b2 = fx.wide_range(rng, n // 4, -30, 30), fx.wide_range(rng, n // 4, -30, 30)
    c2 = (-(a2.astype(np.float64) * b2)).astype(np.float32)
    a, b, c = np.concatenate([a, a2]), np.concatenate([b, b2]), np.concatenate([c, c2])
    got = fx.fmaf(a, b, c)
    ref = libm_fmaf(a, b, c)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def test_fmaf_matches_glibc_on_double_rounding_midpoints(libm_fmaf):
    rng = np.random.default_rng(1)
    a, b, c = _midpoint_cases(rng, 20_000)
    got = fx.fmaf(a, b, c)
    ref = libm_fmaf(a, b, c)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    # the cases are hard: the f64-then-round form gets a good share of them wrong
    naive_wrong = np.count_nonzero(fx.naive_fmaf(a, b, c).view(np.uint32) != ref.view(np.uint32))
    assert naive_wrong > 1000, naive_wrong


def test_gemm_chain_equals_a_scalar_fmaf_loop(libm_fmaf):
    rng = np.random.default_rng(2)
    m, k, n = 5, 12, 7
    x, w = fx.wide_range(rng, (m, k), -20, 20), fx.wide_range(rng, (k, n), -20, 20)
    for order in (np.arange(k), fx.kernel_k_order(k)):
        got = fx.gemm_chain(x, w, order)
        ref = np.zeros((m, n), np.float32)
        for i in range(m):
            for j in range(n):
                acc = np.float32(0.0)
                for kk in order:
                    if kk < k:
                        acc = libm_fmaf([x[i, kk]], [w[kk, j]], [acc])[0]
                ref[i, j] = acc
        assert np.array_equal(got, ref)


def test_kernel_k_order_is_the_documented_permutation():
    o = fx.kernel_k_order(40)
    assert list(o[:10]) == [0, 4, 1, 5, 2, 6, 3, 7, 8, 12]
    assert len(o) == 64 and sorted(o) == list(range(64))
    assert list(o[32:36]) == [32, 36, 33, 37]
    assert list(fx.kernel_k_order(8, "k1")[:4]) == [4, 0, 5, 1]


def test_im2col_matches_conv2d():
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 9, 11, 4)).astype(np.float32)
    w = rng.standard_normal((3, 3, 4, 5)).astype(np.float32)
    for stride, pad, dil in ((1, 1, 1), (2, 1, 1), (1, 2, 2), (2, 3, 3)):
        ho = (9 + 2 * pad - (2 * dil + 1)) // stride + 1
        wo = (11 + 2 * pad - (2 * dil + 1)) // stride + 1
        got = fx.im2col3x3(x, stride, pad, dil, ho, wo).astype(np.float64) @ w.reshape(36, 5).astype(np.float64)
        ref = F.conv2d(torch.from_numpy(x).permute(0, 3, 1, 2).double(), torch.from_numpy(w).permute(3, 2, 0, 1).double(),
                       stride=stride, padding=pad, dilation=dil).permute(0, 2, 3, 1).reshape(-1, 5).numpy()
        np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("s", [2.0 ** -40, 2.0 ** 13])
def test_oracle_is_bit_equivariant_under_power_of_two_scaling(s):
    """The CPU oracle (float32) with the input and every bias-like parameter scaled by 2^k: logits scale by exactly 2^k.
    The property tests/test_gpu_exact_f32.py asks of the exact-f32 engine."""
    from asr_amd import weights as W
    from oracle.model import OracleDeeplabV3Plus
    w = W.make_synthetic_weights(1234, 21)
    x = np.random.default_rng(4).random((1, 64, 96, 3), dtype=np.float32)
    ref = OracleDeeplabV3Plus(w).forward(x)
    got = OracleDeeplabV3Plus(fx.scaled(w, s)).forward(x * np.float32(s))
    assert np.array_equal(got, ref * np.float32(s))
