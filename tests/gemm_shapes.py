"""Case table and data builders shared by tests/test_gpu_gemm_shapes.py (the split-f16 GEMM kernels on the GPU) and
tests/test_gemm_shapes_host.py (numpy float64: the emulated split arithmetic passes the bound, subtly wrong kernels do
not).  Not a test module: both files import it, so the GPU kernels and the host emulation draw the same inputs.

A case names a kernel ("ring" = asr_pwconv_mfma_f16x3_presplit, "split" = asr_pwconv_mfma_f16x3, "conv" =
asr_conv3x3_mfma_f16x3), the GEMM shape, the epilogue (bias, relu 0 / 1 / 2, residual) and the memory layout of every
operand.  build(case) returns the host operands, the float64 reference and the bound of
test_gpu_layers.py::test_pwconv_split_f16_is_f32_grade:  4e-6 * (sum_k |a||w| + |bias| + |residual|)."""
from dataclasses import dataclass, replace
from types import SimpleNamespace

import numpy as np

TOL = 4e-6                  # of sum |a||w| + |bias| + |residual|: the project's f32-grade bound
SENTINEL = -7.0             # prefill of every output buffer
RING = 5                    # slots of the ring kernel's LDS ring (KT mod RING = the ring phase of the last K-step)


def _rand(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


@dataclass(frozen=True)
class Case:
    id: str
    kernel: str             # "ring" | "split" | "conv"
    m: int
    k: int
    n: int
    relu: int = 0
    bias: bool = True
    res: bool = False
    ldy: int = 0            # floats per output row (0 = n)
    y_lead: int = 0         # floats between the start of the output buffer and y (column offset or misalignment)
    ldres: int = 0          # floats per residual row (0 = n); columns n..ldres are NaN
    res_lead: int = 0       # floats the residual pointer is advanced by
    bias_lead: int = 0      # floats the bias pointer is advanced by
    ldx: int = 0            # "split": floats per x row (0 = k), columns k..ldx NaN; "ring": chunks per row (0 = ceil(k / 32))
    sub: tuple = None       # "split": (b, h, w) of the input map gathered with sub_stride = 2; skipped pixels NaN
    conv: tuple = None      # "conv": (b, h, w, cin, cout, stride, pad, dil)
    seed: int = 0

    @property
    def kt(self):           # K-steps
        return -(-self.k // 32)


def _ring(id, m, k, n, seed, **kw):
    return Case(id, "ring", m, k, n, seed=seed, **kw)


def _split(id, m, k, n, seed, **kw):
    return Case(id, "split", m, k, n, seed=seed, **kw)


# ---- ring kernel, one tile per workgroup (m = 293: one full 256-row tile + a ragged 37-row tile) ----------------------
RING_M = 293
# 1. every ring phase: KT = 1..7 and 10 with / without a residual; bias and relu spread so that every activation mode meets
#    a residual at least twice (relu = i % 3 over the eight K: 0 three times, 1 three times, 2 twice -- and K = 40 a third)
RING_PHASE = []
for _i, _k in enumerate((32, 64, 96, 128, 160, 192, 224, 320)):
    RING_PHASE.append(_ring(f"K{_k}-res-relu{_i % 3}-{'bias' if _i % 2 == 0 else 'nobias'}", RING_M, _k, 256, 100 + _i,
                            relu=_i % 3, bias=_i % 2 == 0, res=True))
    RING_PHASE.append(_ring(f"K{_k}-relu{(_i + 1) % 3}-{'bias' if _i % 2 == 1 else 'nobias'}", RING_M, _k, 256, 120 + _i,
                            relu=(_i + 1) % 3, bias=_i % 2 == 1))
RING_PHASE.append(_ring("K40-res-relu2-bias", RING_M, 40, 256, 140, relu=2, res=True))     # zero padding inside the last chunk
# 2. M edges with a residual
RING_M_EDGES = [_ring(f"m{_m}", _m, 64, 256, 200 + _m, relu=1, res=True) for _m in (1, 15, 16, 37, 255, 256, 257)]
# 3. padded last N-tile (CTV = 2, 2, 4, 6, 8 in its right half), N % 4 != 0, the product's 728 with ragged M
RING_N_TILES = []
for _n in (132, 392, 440, 472, 512, 250):
    RING_N_TILES.append(_ring(f"N{_n}-res", RING_M, 160, _n, 300 + _n, relu=1, res=True))
    RING_N_TILES.append(_ring(f"N{_n}", RING_M, 160, _n, 1300 + _n, relu=1))
RING_N_TILES.append(_ring("N728-res", RING_M, 160, 728, 300 + 728, relu=1, res=True))
# 4. one data set, several layouts: (name, layout keywords); every one must reproduce "contiguous" bit for bit
RING_LAYOUT_DATA = _ring("layouts", RING_M, 160, 256, 400, relu=1, res=True)
RING_LAYOUTS = [
    ("contiguous", {}),                                                   # (i)   fast epilogue
    ("concat-slice", dict(ldy=520, y_lead=260, ldres=260)),              # (ii)  fast epilogue, strided
    ("y+3", dict(y_lead=3)),                                              # (iii) slow: y not 16-byte aligned
    ("ldy257", dict(ldy=257)),                                            # (iv)  slow: ldy % 4 != 0
    ("bias+1", dict(bias_lead=1)),                                        # (v)   slow: bias not 16-byte aligned
    ("ldres257", dict(ldres=257)),                                        # (vi)  slow: ldres % 4 != 0
    ("res+1", dict(res_lead=1)),                                          # (vii) slow: residual not 16-byte aligned
]
RING_LAYOUTS_NORES = ("contiguous", "y+3", "bias+1")                     # repeated without a residual
RING_LAYOUTS_NOBIAS = ("contiguous", "concat-slice")                     # repeated with bias = None
RING_LAYOUT_DATA_NORES = replace(RING_LAYOUT_DATA, id="layouts-nores", res=False)      # same a, w and bias (same seed)
RING_LAYOUT_DATA_NOBIAS = replace(RING_LAYOUT_DATA, id="layouts-nobias", bias=False)
# 5. ldx_chunks > chunks: K = 96 in rows of 5 chunks, the two spare chunks NaN
RING_LDX = [_ring("K96-ldx5-res", RING_M, 96, 256, 500, relu=1, res=True, ldx=5),
            _ring("K96-ldx5", RING_M, 96, 256, 501, relu=1, ldx=5)]
# persistent walk: more tiles than CUs; the whole launch into a slice of a wider buffer
WALK = _ring("walk", 70000 + 37, 160, 256, 77, relu=1)

# ---- in-kernel-split kernel -------------------------------------------------------------------------------------------
# 6. the 128 x 64 tile (N <= 64)
SPLIT_TILE64 = [
    _split("decoder-293x256x48-at-256-of-304", 293, 256, 48, 600, relu=1, ldy=304, y_lead=256),
    _split("130x64x64", 130, 64, 64, 601),
    _split("200x36x21-res", 200, 36, 21, 602, res=True),                 # scalar store path, K tail of 4
    _split("1x4x8", 1, 4, 8, 603),
]
# 7. the 128 x 128 tile at its edges
SPLIT_TILE128 = [
    _split("293x36x65", 293, 36, 65, 700),
    _split("293x4x100-res-ldres104", 293, 4, 100, 701, res=True, ldres=104),
    _split("130x728x130", 130, 728, 130, 702),
    _split("257x64x128-res-ldres129", 257, 64, 128, 703, res=True, ldres=129),
]
# 8. relu == 2 on both tiles
SPLIT_RELU6 = [_split(f"relu6-n{_n}{'-res' if _r else ''}", 200, 64, _n, 800 + _n + _r, relu=2, res=bool(_r))
               for _n in (48, 160) for _r in (0, 1)]
# 9. ldx > k
SPLIT_LDX = [_split(f"ldx72-n{_n}", 200, 64, _n, 900 + _n, relu=1, ldx=72) for _n in (48, 160)]
# 10. sub_stride = 2 on an odd map: b = 2, h = 11, w = 9 -> 6 x 5 outputs per image
SPLIT_SUB = [
    _split("sub2-n40-at-16-of-72", 60, 64, 40, 1000, ldy=72, y_lead=16, sub=(2, 11, 9)),
    _split("sub2-n160-res", 60, 64, 160, 1001, res=True, sub=(2, 11, 9)),
]


# 11. implicit 3x3 GEMM
def _conv(b, h, w, cin, cout, stride, pad, dil, relu, seed):
    ho = (h + 2 * pad - (2 * dil + 1)) // stride + 1
    wo = (w + 2 * pad - (2 * dil + 1)) // stride + 1
    return Case(f"conv-{b}x{h}x{w}x{cin}-{cout}-s{stride}p{pad}d{dil}", "conv", b * ho * wo, 9 * cin, cout, relu=relu,
                conv=(b, h, w, cin, cout, stride, pad, dil), seed=seed)


CONV = [_conv(2, 11, 13, 32, 21, 1, 1, 1, 0, 1100), _conv(2, 12, 9, 64, 48, 2, 1, 1, 1, 1101),
        _conv(1, 9, 10, 32, 160, 1, 2, 2, 2, 1102), _conv(2, 8, 8, 32, 64, 1, 0, 1, 1, 1103)]

RING_CASES = (RING_PHASE + RING_M_EDGES + RING_N_TILES + [RING_LAYOUT_DATA, RING_LAYOUT_DATA_NORES, RING_LAYOUT_DATA_NOBIAS]
              + RING_LDX)
SPLIT_CASES = SPLIT_TILE64 + SPLIT_TILE128 + SPLIT_RELU6 + SPLIT_LDX + SPLIT_SUB
HOST_CASES = RING_CASES + SPLIT_CASES + CONV         # WALK: the same arithmetic as RING_PHASE's K = 160, 20 M elements


def conv_out_hw(conv):
    b, h, w, cin, cout, stride, pad, dil = conv
    return (h + 2 * pad - (2 * dil + 1)) // stride + 1, (w + 2 * pad - (2 * dil + 1)) // stride + 1


def im2col(x, conv):
    """x [b, h, w, cin] -> [b * ho * wo, 9 * cin], taps row-major (dy, dx), zero padding"""
    b, h, w, cin, cout, stride, pad, dil = conv
    ho, wo = conv_out_hw(conv)
    xp = np.zeros((b, h + 2 * pad, w + 2 * pad, cin), x.dtype)
    xp[:, pad:pad + h, pad:pad + w] = x
    cols = [xp[:, dy * dil:dy * dil + (ho - 1) * stride + 1:stride, dx * dil:dx * dil + (wo - 1) * stride + 1:stride]
            for dy in range(3) for dx in range(3)]
    return np.concatenate(cols, axis=-1).reshape(b * ho * wo, 9 * cin)


def split16(v):
    """hi = f16(v), lo = f16(v - hi) of a float32 array"""
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def activation(v, relu):
    if relu:
        v = np.maximum(v, 0)
    if relu == 2:
        v = np.minimum(v, 6)
    return v


def build(case):
    """Host operands of a case (float32 / float16), its float64 reference and bound.
      a        [m, k] float32: the GEMM's A operand ("ring": hi + lo, exactly); x: what the kernel is handed ("split": [m, k] or
               the [b, h, w, k] map of a sub_stride gather; "conv": [b, h, w, cin]; "ring": hi, lo [m, k] float16)
      w        [k, n]; bias_full [n + 1] or None; res_full [m + 1, n] or None -- one spare element / row, so that a kernel that
               reads one column / row late can be emulated (and would read defined memory): bias = bias_full[:n], res = res_full[:m]
      pre      float64 a @ w + bias; ref = act(pre) + res; bound = TOL * (|a| @ |w| + |bias| + |res|)  (conv: the magnitude
               convolution alone, as test_gpu_layers.py::test_conv3x3_mfma_matches_conv2d)
    relu == 2: x is scaled by 6 so that the outputs spread over all three pieces of the clamp (asserted by the tests)."""
    c = case
    rng = np.random.default_rng(c.seed)
    xs = 6.0 if c.relu == 2 else 1.0
    d = SimpleNamespace(case=c)
    if c.conv:
        b, h, w, cin = c.conv[:4]
        d.x = _rand(rng, b, h, w, cin, scale=xs)
        d.a = im2col(d.x, c.conv)
    elif c.sub:
        b, h, w = c.sub
        d.x = _rand(rng, b, h, w, c.k, scale=xs)
        d.a = np.ascontiguousarray(d.x[:, ::2, ::2]).reshape(-1, c.k)
    else:
        d.x = d.a = _rand(rng, c.m, c.k, scale=xs)
    assert d.a.shape == (c.m, c.k)
    d.hi, d.lo = split16(d.a)
    if c.kernel == "ring":                       # the operand IS the pair of halves
        d.a = d.hi.astype(np.float32) + d.lo.astype(np.float32)
        assert np.array_equal(d.a.astype(np.float64), d.hi.astype(np.float64) + d.lo.astype(np.float64))
        d.x = (d.hi, d.lo)
    d.w = _rand(rng, c.k, c.n, scale=1.0 / np.sqrt(c.k))
    d.bias_full = _rand(rng, c.n + 1) if c.bias else None
    d.res_full = _rand(rng, c.m + 1, c.n) if c.res else None
    d.bias = d.bias_full[:c.n] if c.bias else None
    d.res = d.res_full[:c.m] if c.res else None
    a64, w64 = d.a.astype(np.float64), d.w.astype(np.float64)
    d.pre = a64 @ w64 + (d.bias if c.bias else 0.0)
    d.ref = activation(d.pre, c.relu) + (d.res if c.res else 0.0)
    mag = np.abs(a64) @ np.abs(w64)
    if not c.conv:
        mag = mag + (np.abs(d.bias) if c.bias else 0.0) + (np.abs(d.res) if c.res else 0.0)
    d.bound = TOL * mag
    return d


def relu6_spread(d):
    """fractions of the float64 pre-activation below 0, inside (0, 6), above 6"""
    return float((d.pre < 0).mean()), float(((d.pre > 0) & (d.pre < 6)).mean()), float((d.pre > 6).mean())


def ring_lines(hi, lo, ldx_chunks=0):
    """The ring kernel's A operand: per row and 32-deep K chunk one 128-byte line [hi(32) | lo(32)], the padding columns up to
    ceil32(k) zero (the contract), chunks beyond ceil(k / 32) -- rows of ldx_chunks chunks -- NaN.  -> float16 [m, ldx_chunks, 2, 32]"""
    m, k = hi.shape
    chunks = -(-k // 32)
    ldx_chunks = ldx_chunks or chunks
    lines = np.full((m, ldx_chunks, 2, 32), np.nan, np.float16)
    pad = chunks * 32 - k
    lines[:, :chunks, 0, :] = np.pad(hi, ((0, 0), (0, pad))).reshape(m, chunks, 32)
    lines[:, :chunks, 1, :] = np.pad(lo, ((0, 0), (0, pad))).reshape(m, chunks, 32)
    return lines


# ---- the split arithmetic in float64, and kernels that are subtly wrong -------------------------------------------------
MUTATIONS = ("drop_lo_whi", "drop_last_chunk", "res_row_late", "bias_col_late", "res_before_act", "no_clamp6")


def applies(case, mutation):
    return {"drop_lo_whi": True, "drop_last_chunk": True, "res_row_late": case.res, "bias_col_late": case.bias,
            "res_before_act": case.res and case.relu != 0, "no_clamp6": case.relu == 2}[mutation]


def emulate(d, mutation=None):
    """hi * whi + hi * wlo + lo * whi -- f16 x f16 products are exact in float64, the sum is float64 -- then the epilogue in
    float64; `mutation` = one of MUTATIONS makes it the result of a kernel with that defect."""
    c = d.case
    assert mutation is None or (mutation in MUTATIONS and applies(c, mutation))
    hi, lo = d.hi.astype(np.float64), d.lo.astype(np.float64)
    whi, wlo = (h.astype(np.float64) for h in split16(d.w))
    kk = 32 * ((c.k - 1) // 32) if mutation == "drop_last_chunk" else c.k
    acc = hi[:, :kk] @ whi[:kk] + hi[:, :kk] @ wlo[:kk]
    if mutation != "drop_lo_whi":
        acc = acc + lo[:, :kk] @ whi[:kk]
    if c.bias:
        acc = acc + (d.bias_full[1:] if mutation == "bias_col_late" else d.bias)
    res = 0.0
    if c.res:
        res = d.res_full[1:] if mutation == "res_row_late" else d.res
    if mutation == "res_before_act":
        return activation(acc + res, c.relu)
    return activation(acc, 1 if mutation == "no_clamp6" else c.relu) + res
