"""Case table, data builders and checks shared by tests/test_gpu_dw_shapes.py (every depthwise kernel of csrc/dwconv.hip on
the GPU) and tests/test_dw_shapes_host.py (numpy only: the oracle against torch, deliberately wrong producers against the
checks, the table against the dispatch and against the built library).  Not a test module.

Every kernel of csrc/dwconv.hip computes, per output element, acc = bias; for (ky, kx) row-major: acc = fma(x, w, acc) -- a
tap outside the image is skipped, a zero value or a zero weight on a finite value, each of which leaves acc unchanged.  The
oracle is therefore tests/f32_exact.py::dwconv_exact and the assertion is EQUALITY; the split-f16 outputs are held to the
bit patterns of f32_exact.split_f16_exact of it.

A case names the entry point ("f32" = asr_dwconv3x3_nhwc_f32, "split" = asr_dwconv3x3_nhwc_split_f16, "aspp_f32" /
"aspp_split" = asr_aspp_dwconv3_nhwc_{f32,split_f16}), the geometry, the activations and the memory layout.  kernel_of(case)
restates the dispatch of csrc/dwconv.hip and names the instantiation the case runs.  build(case) draws standard-normal x and
bias and weights scaled 0.3 from the case's seed; where ldx > c the gap columns of x are NaN; every output buffer is
prefilled (float32: NaN, split: 0xFF bytes) and extends one pixel row beyond the end."""
from dataclasses import dataclass, replace
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

import f32_exact as fx

SCOLS = 16                      # output columns of a workgroup (csrc/dwconv.hip)
SMALL_MAX = 64                  # ASR_DW_SMALL_MAX: maps of up to this many rows walk 16-row strips, taller ones 32-row strips
DIRECT_GRID = 8192 * 256        # threads of dw_direct_kernel's capped grid: more channel quads than this take a second pass
GAMMA10 = 10 * 2.0 ** -24       # of sum |x||w| + |bias|: a chain of ten terms (the bias and nine products), one rounding per step
PREFILL16 = 0xFFFF              # split buffers are prefilled with 0xFF bytes


@dataclass(frozen=True)
class Case:
    id: str
    entry: str                  # "f32" | "split" | "aspp_f32" | "aspp_split"
    b: int
    h_in: int
    w_in: int
    c: int
    stride: int = 1
    rate: object = 1            # int; aspp: the three rates
    pad_top: int = 1
    pad_left: int = 1
    h_out: int = 0
    w_out: int = 0
    pre: int = 0
    post: int = 0
    mode: int = 0               # "f32": 0 auto, 1 direct, 2 streaming
    ldx: int = 0                # floats per input pixel (0 = c); columns c..ldx are NaN
    ldy: int = 0                # "f32" / "aspp_f32": floats per output pixel (0 = c); split entries: ldy_chunks (0 = ceil(c / 32))
    y_lead: int = 0             # float32 outputs: channel offset of y inside the wider buffer
    seed: int = 0
    rows: tuple = None          # fma chain checked on these (r0, r1) output row ranges only (None: everywhere)
    unsupported: bool = False   # the entry must return ASR_ERR_UNSUPPORTED and leave the buffer untouched

    @property
    def split(self):
        return self.entry in ("split", "aspp_split")

    @property
    def aspp(self):
        return self.entry.startswith("aspp")

    @property
    def chunks(self):           # chunks of 32 channels that hold data
        return -(-self.c // 32)

    @property
    def ld_in(self):
        return self.ldx or self.c

    @property
    def ld_out(self):           # floats (f32) or chunks (split) per output pixel
        return self.ldy or (self.chunks if self.split else self.c)

    @property
    def pixels(self):
        return self.b * self.h_out * self.w_out


# ---- the dispatch of csrc/dwconv.hip, restated -----------------------------------------------------------------------------
GEOMETRIES = ((1, 1), (2, 1), (1, 2))          # (R, S): rate and stride of the streaming kernels
UNSUPPORTED = ("unsupported",)


def stream_geometry(stride, rate):
    """(R, S) of the register-window kernels, or None where only dw_direct_kernel applies"""
    if stride == 1 and rate in (1, 2):
        return rate, 1
    if stride == 2 and rate == 1:
        return 1, 2
    return None


def strip_rows(h_out):
    return 16 if h_out <= SMALL_MAX else 32


def kernel_of(case):
    """The instantiation a case runs: ("direct",), ("stream", R, S, SROWS), ("full", R, S, SROWS, PF, SPLIT, ACT),
    ("aspp", SPLIT) -- or UNSUPPORTED where the entry point refuses (asr_dwconv3x3_nhwc_f32's mode choice, launch_stream)."""
    c = case
    if c.aspp:
        return ("aspp", int(c.split))
    geo = stream_geometry(c.stride, c.rate) if c.b <= 65535 else None
    if c.entry == "split":
        if geo is None or c.c % 8:
            return UNSUPPORTED
    else:
        mode = c.mode or (2 if geo else 1)
        if mode == 1:
            return ("direct",)
        if geo is None:
            return UNSUPPORTED
    srows = strip_rows(c.h_out)
    if c.h_out % srows == 0:
        act = 0
        if srows == 16:
            act = 1 if (c.pre, c.post) == (1, 0) else (2 if (c.pre, c.post) == (0, 1) else 0)
        return ("full",) + geo + (srows, 4 if srows == 16 else 1, int(c.split), act)
    if c.split:
        return UNSUPPORTED
    return ("stream",) + geo + (srows,)


ALL_KERNELS = sorted(
    [("direct",)]
    + [("stream", r, s, sr) for r, s in GEOMETRIES for sr in (16, 32)]
    + [("full", r, s, 16, 4, sp, act) for r, s in GEOMETRIES for sp in (0, 1) for act in (0, 1, 2)]
    + [("full", r, s, 32, 1, sp, 0) for r, s in GEOMETRIES for sp in (0, 1)]
    + [("aspp", 0), ("aspp", 1)])
assert len(ALL_KERNELS) == 33


def aspp_geometry(h, w, rates):
    """(g, nxg) of aspp_dw3_phase_kernel's launch (csrc/dwconv.hip: aspp_geometry): the phase period and the number of
    column-phase groups a row phase is cut into until a workgroup's lines fit 48 KB of LDS"""
    g = int(np.gcd.reduce(rates))
    rows = -(-h // g)
    nxg = 1
    while True:
        cols = -(-w // g) * (g // nxg)
        lds = 4 * (rows * cols + 1) * 32 + 4 * cols
        if (lds <= 48 * 1024 and cols <= 128) or nxg == g:
            return g, nxg
        nxg += 1
        while g % nxg:
            nxg += 1


# ---- the case table ----------------------------------------------------------------------------------------------------------
B, W_OUT, C = 2, 20, 72         # one full 16-column tile + a ragged one; one full 64-channel block + 8 channels: c % 32 != 0,
#                                 c % 8 == 0, three chunks, padding channels 72..95
ACT16 = ((1, 0), (0, 1), (0, 0), (1, 1), (0, 2), (1, 2))      # ACT 1, ACT 2, and the four pairs that take ACT 0


def _dw(id, entry, geo, h_out, seed, w_out=W_OUT, c=C, act=(0, 0), pad=None, odd=False, **kw):
    """A streaming-geometry case from its OUTPUT size: stride 1 is 'same' (pad = rate), stride 2 has the explicit pad 1 of the
    Xception sepconvs on an input of 2 * out (odd: 2 * out - 1) or, pad = 0, the TF-SAME padding of MobileNet on an even input"""
    r, s = geo
    if s == 1:
        h_in, w_in, p = h_out, w_out, r
    else:
        p = 1 if pad is None else pad
        h_in, w_in = 2 * h_out - int(odd), 2 * w_out - int(odd)
    return Case(id, entry, B, h_in, w_in, c, stride=s, rate=r, pad_top=p, pad_left=p, h_out=h_out, w_out=w_out, pre=act[0],
                post=act[1], seed=seed, **kw)


def _gname(geo):
    return f"r{geo[0]}s{geo[1]}"


# 1. full strips at 16 rows: two strips, one seam; every compiled-in activation pattern, f32 and split (same seed: same data)
FULL16 = [_dw(f"{_gname(g)}-h32-{e}-pre{a[0]}post{a[1]}", e, g, 32, 1000 + 10 * gi + ai, act=a)
          for gi, g in enumerate(GEOMETRIES) for ai, a in enumerate(ACT16) for e in ("f32", "split")]
# 2. full strips at 32 rows: three strips
ACT32 = ((1, 0), (0, 1), (1, 2))
FULL32 = [_dw(f"{_gname(g)}-h96-{e}-pre{a[0]}post{a[1]}", e, g, 96, 1100 + gi, act=a)
          for gi, g in enumerate(GEOMETRIES) for e, a in (("f32", ACT32[gi]), ("split", ACT32[(gi + 1) % 3]))]
# 3. ragged strips: the generic kernel, 16- and 32-row form; the split entry refuses them
RAGGED = [_dw(f"{_gname(g)}-h{h}-f32-pre{a[0]}post{a[1]}", "f32", g, h, 1200 + 10 * gi + hi, act=a)
          for gi, g in enumerate(GEOMETRIES) for hi, (h, a) in enumerate(((20, ACT16[gi]), (70, ACT16[gi + 3])))]
SPLIT_RAGGED_REFUSED = _dw("r1s1-h20-split-refused", "split", (1, 1), 20, 1290, act=(1, 0), unsupported=True)
# 4. stride 2: pad 1 on an even and on an odd input, TF-SAME (pad 0) on an even input -- full strip, ragged strip, direct
STRIDE2 = []
for _pi, (_pn, _pkw) in enumerate((("pad1-even", {}), ("pad1-odd", dict(odd=True)), ("same-pad0", dict(pad=0)))):
    _a = ((1, 0), (0, 2), (1, 1))[_pi]
    STRIDE2.append(_dw(f"s2-{_pn}-h32-f32", "f32", (1, 2), 32, 1300 + _pi, act=_a, **_pkw))
    STRIDE2.append(_dw(f"s2-{_pn}-h32-split", "split", (1, 2), 32, 1300 + _pi, act=_a, **_pkw))
    STRIDE2.append(_dw(f"s2-{_pn}-h20-f32", "f32", (1, 2), 20, 1310 + _pi, act=_a, **_pkw))
    STRIDE2.append(_dw(f"s2-{_pn}-h20-direct", "f32", (1, 2), 20, 1320 + _pi, act=_a, mode=1, **_pkw))
# 5. leading dimensions: x rows of 80 floats (the gap NaN), y at channel 8 of 88-float pixels; split: four chunks per pixel
LEADING = [
    _dw("ld-r1s1-h32-f32", "f32", (1, 1), 32, 1400, act=(1, 0), ldx=80, ldy=88, y_lead=8),
    _dw("ld-r2s1-h20-f32", "f32", (2, 1), 20, 1401, act=(0, 1), ldx=80, ldy=88, y_lead=8),
    _dw("ld-r1s2-h96-f32", "f32", (1, 2), 96, 1402, act=(1, 1), ldx=80, ldy=88, y_lead=8),
    replace(_dw("ld-direct-rate3-f32", "f32", (1, 1), 16, 1403, act=(0, 2), ldx=80, ldy=88, y_lead=8), rate=3, pad_top=3, pad_left=3),
    _dw("ld-r1s1-h32-split", "split", (1, 1), 32, 1400, act=(1, 0), ldx=80, ldy=4),
    _dw("ld-r1s2-h96-split", "split", (1, 2), 96, 1402, act=(1, 1), ldx=80, ldy=4),
]
# 6. narrow and tiny maps
NARROW = [
    _dw("w3-f32", "f32", (1, 1), 32, 1500, w_out=3, act=(1, 0)),
    _dw("w3-split", "split", (1, 1), 32, 1500, w_out=3, act=(1, 0)),
    _dw("w16-f32", "f32", (2, 1), 32, 1501, w_out=16, act=(0, 1)),
    _dw("w16-split", "split", (2, 1), 32, 1501, w_out=16, act=(0, 1)),
    _dw("h1-f32", "f32", (1, 1), 1, 1502, act=(1, 1)),
    _dw("c4-f32", "f32", (1, 1), 32, 1503, c=4, act=(0, 0)),
    _dw("c8-f32", "f32", (1, 2), 32, 1504, c=8, act=(1, 0)),
    _dw("c8-split", "split", (1, 2), 32, 1504, c=8, act=(1, 0)),
]
# 7. direct kernel: the ASPP rates (and 3) on a 16 x 20 map; rate 6 with more channel quads than the capped grid has threads
DIRECT = [Case(f"direct-rate{r}", "f32", B, 16, W_OUT, C, rate=r, pad_top=r, pad_left=r, h_out=16, w_out=W_OUT, pre=a[0], post=a[1],
               seed=1600 + r) for r, a in ((6, (0, 1)), (12, (1, 0)), (18, (1, 1)), (3, (0, 2)))]
DIRECT_TWO_PASSES = Case("direct-rate6-two-passes", "f32", 1, 64, 66, 2048, rate=6, pad_top=6, pad_left=6, h_out=64, w_out=66,
                         post=1, seed=1650, rows=((0, 4), (60, 64)))
# 8. fused ASPP
def _aspp(id, entry, h, w, c, rates, seed, act=(0, 1), **kw):
    return Case(id, entry, B, h, w, c, rate=rates, pad_top=0, pad_left=0, h_out=h, w_out=w, pre=act[0], post=act[1], seed=seed, **kw)


ASPP = [
    _aspp("aspp-17x21x40-f32-ld", "aspp_f32", 17, 21, 40, (6, 12, 18), 1700, act=(1, 0), ldx=48, ldy=56),
    _aspp("aspp-17x21x64-split-ldx72-pre", "aspp_split", 17, 21, 64, (6, 12, 18), 1701, act=(1, 0), ldx=72),
    _aspp("aspp-33x45x32-split-r2-4-6-relu6", "aspp_split", 33, 45, 32, (2, 4, 6), 1702, act=(0, 2)),
    _aspp("aspp-64x64x32-split-nxg2", "aspp_split", 64, 64, 32, (6, 12, 18), 1703),
    _aspp("aspp-17x21x64-split-3chunks", "aspp_split", 17, 21, 64, (6, 12, 18), 1704, ldy=3),
    _aspp("aspp-33x45x40-f32-r2-4-6-relu6", "aspp_f32", 33, 45, 40, (2, 4, 6), 1705, act=(1, 2)),
]

# Seeds of the post_relu = 2 data sets, chosen so that the float64 pre-activations reach both pieces of the clamp (below 0, above
# 6: asserted by tests/test_dw_shapes_host.py) -- with O(1) operands an output beyond 6 is a 4.5-sigma event.
RESEED = {1004: 321004, 1005: 651005, 1014: 21014, 1015: 371015, 1024: 111024, 1025: 501025, 1101: 81101, 1102: 21102, 1211: 61211,
          1221: 501221, 1301: 41301, 1311: 441311, 1403: 91403, 1603: 141603, 1702: 341702, 1705: 341705}


def _reseeded(cases):
    return [replace(c, seed=RESEED.get(c.seed, c.seed)) for c in cases]


FULL16, FULL32, RAGGED, STRIDE2, LEADING, NARROW, DIRECT, ASPP = (_reseeded(g) for g in (FULL16, FULL32, RAGGED, STRIDE2, LEADING, NARROW,
                                                                                          DIRECT, ASPP))
F32_CASES = [c for c in FULL16 + FULL32 + RAGGED + STRIDE2 + LEADING + NARROW + DIRECT if c.entry == "f32"]
SPLIT_CASES = [c for c in FULL16 + FULL32 + STRIDE2 + LEADING + NARROW if c.entry == "split"]
CASES = F32_CASES + SPLIT_CASES + [DIRECT_TWO_PASSES] + ASPP             # SPLIT_RAGGED_REFUSED runs no kernel
SMALL_CASES = [c for c in CASES if c is not DIRECT_TWO_PASSES]


# ---- data ----------------------------------------------------------------------------------------------------------------------
def dwconv_f64(x, w, bias, stride, rate, pad_top, pad_left, out_hw, pre_relu):
    """(bias + sum x * w, |bias| + sum |x||w|) in float64 before the post-activation, taps outside the image skipped"""
    x = np.asarray(x, np.float64)
    if pre_relu:
        x = np.maximum(x, 0.0)
    b, h, wd, c = x.shape
    ho, wo = out_hw
    acc = np.broadcast_to(np.asarray(bias, np.float64), (b, ho, wo, c)).copy()
    mag = np.abs(acc)
    for ky, kx in fx.TAPS:
        ya, yb = fx._tap_range(ho, h, stride, pad_top, ky * rate)
        xa, xb = fx._tap_range(wo, wd, stride, pad_left, kx * rate)
        if yb <= ya or xb <= xa:
            continue
        iy0, ix0 = ya * stride - pad_top + ky * rate, xa * stride - pad_left + kx * rate
        p = x[:, iy0:iy0 + (yb - ya - 1) * stride + 1:stride, ix0:ix0 + (xb - xa - 1) * stride + 1:stride] * w[ky, kx].astype(np.float64)
        acc[:, ya:yb, xa:xb] += p
        mag[:, ya:yb, xa:xb] += np.abs(p)
    return acc, mag


def activation(v, post):
    if post:
        v = np.maximum(v, 0)
    if post == 2:
        v = np.minimum(v, 6)
    return v


def branches(case):
    """[(rate, pad)] of the convolutions a case computes: one, or the three of the fused ASPP ('same': pad = rate)"""
    return [(r, r) for r in case.rate] if case.aspp else [(case.rate, None)]


def build(case):
    """Host operands and expectations of a case:
      x [b,h,w,c], xbuf the flat input buffer with ldx floats per pixel (gap NaN), w [3,3,c] / bias [c] (aspp: [3,3,3,c] / [3,c]);
      per branch: exact (dwconv_exact; rows: a list of (r0, exact rows)), pre64 / ref64 (float64 before / after the
      post-activation), bound = GAMMA10 * (sum |x||w| + |bias|), hi / lo (split_f16_exact of exact, uint16)."""
    c = case
    rng = np.random.default_rng(c.seed)
    d = SimpleNamespace(case=c)
    d.x = rng.standard_normal((c.b, c.h_in, c.w_in, c.c)).astype(np.float32)
    nb = 3 if c.aspp else 1
    w = (rng.standard_normal((nb, 3, 3, c.c)) * 0.3).astype(np.float32)
    bias = rng.standard_normal((nb, c.c)).astype(np.float32)
    d.w, d.bias = (w, bias) if c.aspp else (w[0], bias[0])
    xbuf = np.full((c.b * c.h_in * c.w_in, c.ld_in), np.nan, np.float32)
    xbuf[:, :c.c] = d.x.reshape(-1, c.c)
    d.xbuf = xbuf.reshape(-1)
    d.exact, d.pre64, d.ref64, d.bound, d.hi, d.lo = [], [], [], [], [], []
    for i, (rate, pad) in enumerate(branches(c)):
        pt, pl = (pad, pad) if c.aspp else (c.pad_top, c.pad_left)
        geom = (c.stride, rate, pt, pl, (c.h_out, c.w_out))
        if c.rows:
            d.exact.append([(r0, fx.dwconv_exact(d.x, w[i], bias[i], *geom, c.pre, c.post, rows=(r0, r1))) for r0, r1 in c.rows])
        else:
            d.exact.append(fx.dwconv_exact(d.x, w[i], bias[i], *geom, c.pre, c.post))
            if c.split:
                hi, lo = fx.split_f16_exact(d.exact[-1])
                d.hi.append(hi)
                d.lo.append(lo)
        pre64, mag = dwconv_f64(d.x, w[i], bias[i], *geom, c.pre)
        d.pre64.append(pre64)
        d.ref64.append(activation(pre64, c.post))
        d.bound.append(GAMMA10 * mag)
    return d


build_shared = lru_cache(maxsize=None)(build)     # for a module that visits every case many times; it clears the cache when it is done


def relu6_reach(d):
    """how many float64 pre-activations of a post_relu = 2 case lie below 0, and above 6"""
    return min(int((p < 0).sum()) for p in d.pre64), min(int((p > 6).sum()) for p in d.pre64)


# ---- output buffers --------------------------------------------------------------------------------------------------------------
def out_buffer(case):
    """The prefilled output buffer of one branch, one pixel row longer than the output: float32 NaN [y_lead + (pixels + w_out) *
    ldy], or uint16 0xFFFF [(pixels + w_out), ldy_chunks, 2, 32] flattened."""
    n = case.pixels + case.w_out
    if case.split:
        return np.full(n * case.ld_out * 64, PREFILL16, np.uint16)
    return np.full(case.y_lead + n * case.ld_out, np.nan, np.float32)


def store_f32(case, buf, y):
    """what a correct float32 kernel does to the buffer with the result y [b, h_out, w_out, c]"""
    view = buf[case.y_lead:case.y_lead + case.pixels * case.ld_out].reshape(case.pixels, case.ld_out)
    view[:, :case.c] = y.reshape(case.pixels, case.c)
    return buf


def store_split(case, buf, hi, lo):
    """what a correct split kernel does to the buffer with the halves hi, lo [b, h_out, w_out, c] (uint16): the chunks that hold
    data, their padding channels zero; asr_dwconv3x3_nhwc_split_f16 also zeroes every further chunk up to ldy_chunks, the fused
    ASPP (c % 32 == 0) leaves them alone"""
    lines = buf[:case.pixels * case.ld_out * 64].reshape(case.pixels, case.ld_out, 2, 32)
    zeroed = case.chunks if case.aspp else case.ld_out
    pad = zeroed * 32 - case.c
    lines[:, :zeroed, 0, :] = np.pad(hi.reshape(case.pixels, case.c), ((0, 0), (0, pad))).reshape(case.pixels, zeroed, 32)
    lines[:, :zeroed, 1, :] = np.pad(lo.reshape(case.pixels, case.c), ((0, 0), (0, pad))).reshape(case.pixels, zeroed, 32)
    return buf


# ---- the checks (section by section what tests/test_gpu_dw_shapes.py asserts) -----------------------------------------------------
def _first(diff):
    return tuple(int(i) for i in np.argwhere(diff)[0])


def read_f32(case, buf):
    """[b, h_out, w_out, c] out of a float32 output buffer; everything else must still hold the NaN prefill"""
    assert buf.shape == out_buffer(case).shape
    body = buf[case.y_lead:case.y_lead + case.pixels * case.ld_out].reshape(case.pixels, case.ld_out)
    outside = np.concatenate([buf[:case.y_lead], body[:, case.c:].ravel(), buf[case.y_lead + case.pixels * case.ld_out:]])
    written = ~np.isnan(outside)
    assert not written.any(), f"{case.id}: {int(written.sum())} floats outside the output (ldy gap, channel offset, guard row) were written"
    return body[:, :case.c].reshape(case.b, case.h_out, case.w_out, case.c)


def check_f32(d, got, branch=0):
    """got [b, h_out, w_out, c] float32: equal to the fma chain (on the case's rows), and within gamma_10 of the float64 sum"""
    c = d.case
    assert got.shape == d.ref64[branch].shape and got.dtype == np.float32
    assert np.isfinite(got).all(), f"{c.id}[{branch}]: {int((~np.isfinite(got)).sum())} non-finite outputs (prefill left, or a NaN gap column read)"
    parts = d.exact[branch] if c.rows else [(0, d.exact[branch])]
    for r0, exact in parts:
        diff = got[:, r0:r0 + exact.shape[1]] != exact
        assert not diff.any(), (f"{c.id}[{branch}] {kernel_of(c)}: {int(diff.sum())} of {diff.size} outputs differ from the fma chain, "
                                f"first at (b, y, x, ch) = {_first(diff)} (rows from {r0})")
    err = np.abs(got.astype(np.float64) - d.ref64[branch])
    over = err > d.bound[branch]
    assert not over.any(), f"{c.id}[{branch}]: {int(over.sum())} outputs beyond 10 * 2^-24 * (sum |x||w| + |bias|), first at {_first(over)}"


def read_split(case, buf):
    """(hi, lo) [b, h_out, w_out, c] uint16 out of a split output buffer.  Padding channels of the data chunks must be 0x0000;
    further chunks up to ldy_chunks 0x0000 (asr_dwconv3x3_nhwc_split_f16) or untouched (fused ASPP); the guard row untouched."""
    assert buf.shape == out_buffer(case).shape
    n = case.pixels * case.ld_out * 64
    lines = buf[:n].reshape(case.pixels, case.ld_out, 2, 32)
    guard = buf[n:] != PREFILL16
    assert not guard.any(), f"{case.id}: {int(guard.sum())} halves of the guard row were written"
    zeroed = case.chunks if case.aspp else case.ld_out
    flat = lines[:, :zeroed].transpose(0, 2, 1, 3).reshape(case.pixels, 2, zeroed * 32)
    padding = flat[:, :, case.c:] != 0
    assert not padding.any(), (f"{case.id}: {int(padding.sum())} padding halves (channels {case.c}..{zeroed * 32 - 1}) are not 0x0000, "
                               f"first at (pixel, hi/lo, channel - c) = {_first(padding)}")
    spare = lines[:, zeroed:] != PREFILL16
    assert not spare.any(), f"{case.id}: {int(spare.sum())} halves of the chunks beyond the data were written"
    shape = (case.b, case.h_out, case.w_out, case.c)
    return flat[:, 0, :case.c].reshape(shape), flat[:, 1, :case.c].reshape(shape)


def check_split(d, hi, lo, branch=0):
    """the halves equal split_f16_exact of the fma chain, bit for bit"""
    c = d.case
    for name, got, want in (("hi", hi, d.hi[branch]), ("lo", lo, d.lo[branch])):
        diff = got != want
        if diff.any():
            sub = (want[diff] & 0x7C00) == 0                    # expected half is zero or an f16 subnormal
            delta = np.abs(got[diff].view(np.float16).astype(np.float64) - want[diff].view(np.float16).astype(np.float64))
            raise AssertionError(f"{c.id}[{branch}] {kernel_of(c)}: {int(diff.sum())} of {diff.size} {name} halves differ from the split of "
                                 f"the fma chain ({int(sub.sum())} of them where a subnormal or zero is expected, largest difference "
                                 f"{float(np.nanmax(delta)):.3e}), first at (b, y, x, ch) = {_first(diff)}: {int(got[diff][0]):#06x} for "
                                 f"{int(want[diff][0]):#06x}")


def check_same_operand(case, hi, lo, y_f32, branch=0):
    """the split entry's halves equal the numpy split of what the float32 entry returned at the same geometry"""
    want_hi, want_lo = fx.split_f16_exact(y_f32)
    diff = (hi != want_hi) | (lo != want_lo)
    assert not diff.any(), (f"{case.id}[{branch}]: {int(diff.sum())} elements of the split operand differ from the split of the float32 "
                            f"entry's output, first at {_first(diff)}")


# ---- deliberately wrong producers (applied on the CPU by tests/test_dw_shapes_host.py) ---------------------------------------------
MUTATIONS = ("tap_order_kx_ky", "last_tap_mul_add", "stride2_pad_other_side", "strip_seam_stale_window", "pre_relu_on_bias",
             "relu6_as_relu", "lo_before_hi_rounded", "padding_channel_left", "odd_quads_hi_lo_exchanged")


def applies(case, mutation):
    if case.rows or case.unsupported:
        return False
    k = kernel_of(case)
    rate = min(case.rate) if case.aspp else case.rate
    corners = rate < min(case.h_in, case.w_in)          # some output has taps of two rows and two columns inside the image
    return {"tap_order_kx_ky": corners, "last_tap_mul_add": corners,
            "stride2_pad_other_side": case.stride == 2,
            "strip_seam_stale_window": k[0] in ("full", "stream") and case.h_out > k[3],
            "pre_relu_on_bias": bool(case.pre), "relu6_as_relu": case.post == 2,
            "lo_before_hi_rounded": case.split,
            "padding_channel_left": case.split and case.c % 32 != 0,
            "odd_quads_hi_lo_exchanged": case.split and case.c >= 8}[mutation]


def produce(d, mutation=None):
    """The output buffers (one per branch) a kernel leaves behind, computed on the CPU; mutation = one of MUTATIONS: a kernel
    with that defect."""
    c = d.case
    assert mutation is None or (mutation in MUTATIONS and applies(c, mutation)), (c.id, mutation)
    bufs = []
    for i, (rate, pad) in enumerate(branches(c)):
        w, bias = (d.w[i], d.bias[i]) if c.aspp else (d.w, d.bias)
        pt, pl = (pad, pad) if c.aspp else (c.pad_top, c.pad_left)
        kw = {}
        x, pre = d.x, c.pre
        post = c.post
        if mutation == "tap_order_kx_ky":
            kw["taps"] = tuple((ky, kx) for kx in range(3) for ky in range(3))
        elif mutation == "last_tap_mul_add":
            calls = []

            def fma(a, b_, acc):
                calls.append(1)
                if len(calls) == 9:
                    return (np.asarray(a, np.float32) * np.asarray(b_, np.float32)).astype(np.float32) + acc
                return fx.fmaf(a, b_, acc)
            kw["fma"] = fma
        elif mutation == "stride2_pad_other_side":
            pt, pl = 1 - pt, 1 - pl
        elif mutation == "pre_relu_on_bias":
            pre, bias = 0, np.maximum(bias, np.float32(0))
        elif mutation == "relu6_as_relu":
            post = 1
        if mutation is None:
            y = d.exact[i]
        else:
            y = fx.dwconv_exact(x, w, bias, c.stride, rate, pt, pl, (c.h_out, c.w_out), pre, post, **kw)
        if mutation == "strip_seam_stale_window":
            srows = kernel_of(c)[3]
            y = y.copy()
            y[:, srows] = y[:, srows - 1]
        buf = out_buffer(c)
        if not c.split:
            bufs.append(store_f32(c, buf, y))
            continue
        hi, lo = fx.split_f16_exact(y)
        if mutation == "lo_before_hi_rounded":
            v = np.clip(y, -fx.F16_MAX, fx.F16_MAX)
            lo = (y - v).astype(np.float16).view(np.uint16)
        elif mutation == "odd_quads_hi_lo_exchanged":
            odd = (np.arange(c.c) // 4) % 2 == 1
            hi, lo = np.where(odd, lo, hi), np.where(odd, hi, lo)
        store_split(c, buf, hi, lo)
        if mutation == "padding_channel_left":
            buf.reshape(-1, c.ld_out, 2, 32)[c.pixels // 2, c.chunks - 1, 1, 31] = PREFILL16
        bufs.append(buf)
    return bufs


def check_buffers(d, bufs):
    """every check of tests/test_gpu_dw_shapes.py that needs one launch only, on the buffers of a (real or emulated) kernel"""
    c = d.case
    for i, buf in enumerate(bufs):
        if c.split:
            hi, lo = read_split(c, buf)
            check_split(d, hi, lo, i)
        else:
            check_f32(d, read_f32(c, buf), i)
