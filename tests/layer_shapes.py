"""Case table, data builders, oracles and checks shared by tests/test_gpu_layer_shapes.py (the kernels of csrc/layers.hip and
csrc/sepconv.hip on the GPU) and tests/test_layer_shapes_host.py (numpy / torch only: the oracles against torch, deliberately
wrong producers against the checks, the table against the restated launch geometry and the sources).  Not a test module.

The launch geometry of the two files is restated here so that a case can say which path it runs:
  * entry_stem_fused_kernel   16 x 16 output tiles, row-major per image, grid = min(tiles, CUs), tile += gridDim   (stem_walk)
  * sepconv_fused_kernel      8 x 14 tiles, grid = min(tiles, CUs * (2 if cin == 64 else 1)), every workgroup walks ONE run
                              [g * per_wg, min((g + 1) * per_wg, tiles)) with per_wg = ceil(tiles / grid)           (sepconv_walk)
  * conv3x3_*_kernel          cap_grid(work items) <= 8192 workgroups of 256 threads, grid-stride beyond            (conv_work)
  * asr_resize_bilinear_f32   the three-column x4 kernel iff w_out == 4 * w_in and w_in >= 2                         (resize_kernel)
Shapes that depend on the CU count are functions of `cus`: table(cus).

build(case) draws seeded standard-normal data (weights scaled as in tests/test_gpu_layers.py); where ldx > c the gap columns
of the input are NaN; out_buffer(case) is NaN everywhere, `lead` floats in front of the output, ldy floats per pixel, one
pixel row behind the end.  read_out asserts that everything outside the written slice still holds the prefill.

Oracles and bounds (none tuned):
  * GAP: the kernel's arithmetic is a fixed sequence of f32 adds and one multiply (four partial sums over pixels grp, grp + 4,
    ..., ((p0 + p1) + p2) + p3, times float32(1) / float32(hw)): gap_exact replays it, the assertion is EQUALITY;
  * VALU convolutions (conv3x3_stem_kernel, conv3x3_direct_kernel): float64 convolution, GAMMA28 = 28 * 2^-24 of
    sum |x||w| + |bias| -- a chain of 27 products and the bias, one rounding per step whether or not the compiler contracts;
  * split-f16 MFMA kernels (MFMA stem, fused stem, fused sepconv): the project's f32-grade figure F32_GRADE = 4e-6 of
    sum |a||w| + |bias| against float64; the two-layer fused stem propagates layer 1's bound through |w2| (ReLU is
    1-Lipschitz): 4e-6 * (|w2| * mid64 + |b2|) + |w2| * (4e-6 * (|w1| * |x| + |b1|));
  * fused sepconv: its `a` is f32_exact.dwconv_exact (the fma chain of the depthwise stage) of the input;
  * resize: float64 lerp at float64 positions with TF half-pixel taps; see resize_f64 for the bound's derivation."""
from dataclasses import dataclass, replace
from types import SimpleNamespace

import numpy as np
import torch

import f32_exact as fx

ES_T = 16                       # entry_stem_fused_kernel's output tile
SF_TH, SF_TW = 8, 14            # sepconv_fused_kernel's output tile
SP = 4                          # output pixels of a thread of conv3x3_stem_kernel
CAP_BLOCKS, BLOCK = 8192, 256   # cap_grid
GAMMA28 = 28 * 2.0 ** -24
F32_GRADE = 4e-6
U = 2.0 ** -24
ASR_ERR_INVALID_ARG, ASR_ERR_UNSUPPORTED = -1, -2


def cdiv(a, b):
    return -(-a // b)


@dataclass(frozen=True)
class Case:
    id: str
    family: str                 # "stem" | "sepconv" | "conv" | "gap" | "resize"
    b: int
    h: int                      # input rows (gap: hw)
    w: int                      # input columns (gap: 1)
    cin: int
    cout: int
    h_out: int
    w_out: int
    kernel: str = ""            # conv: "valu" | "mfma" | "generic"; resize: "x4" | "generic"
    stride: int = 1
    pad: int = 0                # conv: pad_top = pad_left
    relu: int = 0               # conv: 0 | 1 | 2
    act: tuple = (0, 0, 0)      # sepconv: (pre_relu, dw_relu, out_relu)
    ldx: int = 0                # floats per input pixel (0 = cin); columns cin..ldx are NaN
    ldy: int = 0                # floats per output pixel (0 = cout)
    lead: int = 0               # channel offset of the output inside the wider buffer
    seed: int = 0
    xscale: float = 1.0
    path: str = ""              # what of the launch geometry the case is there for

    @property
    def ld_in(self):
        return self.ldx or self.cin

    @property
    def ld_out(self):
        return self.ldy or self.cout

    @property
    def pixels(self):
        return self.b * self.h_out * self.w_out

    @property
    def bytes(self):            # device buffers of one launch
        return 4 * (self.b * self.h * self.w * self.ld_in + self.lead + (self.pixels + self.w_out) * self.ld_out)


# ---- the launch geometry, restated ------------------------------------------------------------------------------------------
def stem_walk(b, h_in, w_in, cus):
    """entry_stem_fused_kernel: tiles, grid and the tiles of every workgroup (tile = blockIdx; tile < total; tile += gridDim)"""
    h1, w1d = h_in // 2, w_in // 2
    ty, tx = cdiv(h1, ES_T), cdiv(w1d, ES_T)
    tiles = b * ty * tx
    grid = min(tiles, cus)
    return SimpleNamespace(h1=h1, w1d=w1d, tiles_y=ty, tiles_x=tx, tiles=tiles, grid=grid,
                           of=[list(range(g, tiles, grid)) for g in range(grid)])


def stem_tile_region(wk, tile):
    """(image, row slice, column slice) of a tile's valid outputs"""
    txi = tile % wk.tiles_x
    tt = tile // wk.tiles_x
    tyi, img = tt % wk.tiles_y, tt // wk.tiles_y
    return img, slice(tyi * ES_T, min(tyi * ES_T + ES_T, wk.h1)), slice(txi * ES_T, min(txi * ES_T + ES_T, wk.w1d))


def sepconv_walk(b, h, w, cin, cus):
    """sepconv_fused_kernel: tiles, grid, per_wg and every workgroup's run [first, last) (idle: first >= last)"""
    ty, tx = cdiv(h, SF_TH), cdiv(w, SF_TW)
    tiles = b * ty * tx
    want = cus * (2 if cin == 64 else 1)        # launch_sepconv_fused: two workgroups per CU where the LDS is <= 80 KB
    grid = min(tiles, want)
    per_wg = cdiv(tiles, grid)
    runs = [(g * per_wg, min(g * per_wg + per_wg, tiles)) for g in range(grid)]
    return SimpleNamespace(tiles_y=ty, tiles_x=tx, per_image=ty * tx, tiles=tiles, want=want, grid=grid, per_wg=per_wg, runs=runs)


def sepconv_run_properties(wk):
    """which of the four things a run can do occur in this walk"""
    live = [(f, l) for f, l in wk.runs if f < l]
    steps = [t for f, l in live for t in range(f, l - 1)]             # t and t + 1 in the same run
    return dict(
        crosses_tile_row_end=any((t + 1) % wk.tiles_x == 0 and (t + 1) % wk.per_image != 0 for t in steps),
        crosses_image_end=any((t + 1) % wk.per_image == 0 for t in steps),
        shorter_last_run=len({l - f for f, l in live}) > 1 and live[-1][1] - live[-1][0] < wk.per_wg,
        idle_workgroup=any(f >= l for f, l in wk.runs))


def sepconv_tile_origin(wk, tile):
    txi = tile % wk.tiles_x
    tt = tile // wk.tiles_x
    return tt // wk.tiles_y, (tt % wk.tiles_y) * SF_TH, txi * SF_TW


def cap_grid(total):
    return min(max(cdiv(total, BLOCK), 1), CAP_BLOCKS)


def conv_kernel(entry, cin, cout):
    """asr_conv3x3_direct_f32 runs the VALU stem kernel for 3 -> 32 and the generic kernel otherwise; asr_conv3x3_stem_f16x3 the MFMA stem"""
    if entry == "asr_conv3x3_stem_f16x3":
        return "mfma"
    return "valu" if (cin, cout) == (3, 32) else "generic"


def conv_work(kernel, b, h_out, w_out, cout):
    """threads the launch asks cap_grid for, the grid, the passes of the grid-stride loop, and (VALU stem) the pixel groups"""
    if kernel == "valu":
        groups = b * h_out * cdiv(w_out, SP)
        threads = cdiv(groups, 8) * 64
    elif kernel == "mfma":
        groups = b * h_out * cdiv(w_out, 32)
        threads = groups * 64
    else:
        groups = threads = b * h_out * w_out * (cout // 4)
    grid = cap_grid(threads)
    return SimpleNamespace(groups=groups, threads=threads, grid=grid, passes=cdiv(threads, grid * BLOCK),
                           masked_groups=(cdiv(groups, 8) * 8 - groups) if kernel == "valu" else 0,
                           first_pass_groups=grid * BLOCK // {"valu": 8, "mfma": 64, "generic": 1}[kernel])


def resize_kernel(w_in, w_out):
    return "x4" if w_out == 4 * w_in and w_in >= 2 else "generic"


def entry_of(case):
    c = case
    if c.family == "conv":
        return "asr_conv3x3_stem_f16x3" if c.kernel == "mfma" else "asr_conv3x3_direct_f32"
    return {"stem": "asr_entry_stem_f16x3", "sepconv": "asr_sepconv_fused_f16x3", "gap": "asr_gap_f32", "resize": "asr_resize_bilinear_f32"}[c.family]


def call_args(case, x, weights, y):
    """the arguments of the case's entry point after its pointers' and before the stream: x, the weight pointers in the ABI's
    order and y are device addresses"""
    c = case
    if c.family == "stem":
        return (x, *weights, y, c.b, c.h, c.w, c.ld_in, c.ld_out)
    if c.family == "sepconv":
        return (x, *weights, y, c.b, c.h, c.w, c.cin, c.cout, c.ld_in, c.ld_out, *c.act)
    if c.family == "conv":
        return (x, *weights, y, c.b, c.h, c.w, c.cin, c.cout, c.stride, c.pad, c.pad, c.h_out, c.w_out, c.ld_in, c.ld_out, c.relu)
    if c.family == "gap":
        return (x, y, c.b, c.h, c.cin, c.ld_in)
    return (x, y, c.b, c.h, c.w, c.cin, c.h_out, c.w_out, c.ld_in, c.ld_out)


# ---- the case table ---------------------------------------------------------------------------------------------------------
ACTS = ((0, 0, 0), (1, 0, 0), (0, 1, 1), (1, 1, 1))
SMALL_MAPS = ((1, 1), (1, 30), (30, 1), (7, 13), (8, 14), (9, 15))
GEOS = ("s2-pad0-even", "s2-pad1-odd", "s1-pad1")


def _stem(id, b, h, w, seed, path, **kw):
    return Case(f"stem-{id}", "stem", b, h, w, 3, 64, h // 2, w // 2, seed=seed, path=path, **kw)


def stem_cases(cus):
    walk_b = (2 * cus) // 12 + 1                 # 12 tiles per image: the first batch with tiles > 2 * cus, at most 12 beyond
    out = [_stem("walk-80x112", walk_b, 80, 112, 2000, "walk")]
    out += [_stem(f"small-{h}x{w}", 2, h, w, 2001 + i, "small") for i, (h, w) in enumerate(((2, 2), (2, 40), (40, 2), (30, 30)))]
    out.append(_stem("ldx4-34x50", 2, 34, 50, 2010, "ldx", ldx=4))
    out.append(_stem("ldy96-34x50", 2, 34, 50, 2011, "ldy", ldy=96, lead=16))
    return out


def _sep(id, cin, b, h, w, act, seed, path, **kw):
    return Case(f"sep{cin}-{id}", "sepconv", b, h, w, cin, 128, h, w, act=act, seed=seed, path=path, **kw)


def sepconv_walk_batch(cin, cus, per_wg):
    """12 x 61 maps (10 tiles each): the smallest batch whose walk has this per_wg -- and, for per_wg = 3, a tile count that is no
    multiple of 3, so that the last live run is shorter"""
    want = cus * (2 if cin == 64 else 1)
    b = ((per_wg - 1) * want) // 10 + 1
    while per_wg == 3 and (10 * b) % 3 == 0:
        b += 1
    return b


def sepconv_cases(cus):
    out = []
    for ci, cin in enumerate((64, 128)):
        s = 3000 + 100 * ci
        out.append(_sep("walk3-12x61", cin, sepconv_walk_batch(cin, cus, 3), 12, 61, ACTS[1], s, "walk3"))
        out.append(_sep("walk2-12x61", cin, sepconv_walk_batch(cin, cus, 2), 12, 61, ACTS[2], s + 1, "walk2"))
        out += [_sep(f"small-{h}x{w}", cin, 2, h, w, ACTS[(i + ci) % 4], s + 10 + i, "small") for i, (h, w) in enumerate(SMALL_MAPS)]
        out += [_sep("act%d%d%d-17x30" % a, cin, 2, 17, 30, a, s + 20 + i, "act") for i, a in enumerate(ACTS)]
        out.append(_sep("ldx-17x30", cin, 2, 17, 30, ACTS[1], s + 30, "ldx", ldx=cin + 8))
        out.append(_sep("ldy160-17x30", cin, 2, 17, 30, ACTS[3], s + 31, "ldy", ldy=160, lead=32))
    return out


def _conv(id, kernel, cin, cout, b, h_out, w_out, geo, relu, seed, path, **kw):
    stride, pad, h, w = {"s2-pad0-even": (2, 0, 2 * h_out, 2 * w_out), "s2-pad1-odd": (2, 1, 2 * h_out - 1, 2 * w_out - 1),
                         "s1-pad1": (1, 1, h_out, w_out)}[geo]
    return Case(f"conv-{kernel}-{id}", "conv", b, h, w, cin, cout, h_out, w_out, kernel=kernel, stride=stride, pad=pad, relu=relu, seed=seed,
                xscale=6.0 if relu == 2 else 1.0, path=path, **kw)


CONV_WIDTHS = {"valu": (1, 2, 3, 5, 6, 7), "mfma": (1, 31, 33, 70), "generic": (1, 5, 9)}
CONV_CH = {"valu": (3, 32), "mfma": (3, 32), "generic": (2, 4)}
# second pass of the capped grid: w_out = 1, batch * h_out just beyond what 8192 x 256 threads cover in one pass
#   VALU stem: 262144 groups of <= 4 pixels; 262165 leaves a last wave with five live and three masked groups
#   MFMA stem: 32768 waves of <= 32 pixels;  generic 3 -> 8: 2097152 threads of one pixel and four channels
SECOND_PASS = {"valu": (5, 52433, 3, 32, 1), "mfma": (13, 2521, 3, 32, 2), "generic": (5, 209719, 3, 8, 0)}


def conv_cases(cus=None):
    out = []
    for ki, kernel in enumerate(("valu", "mfma", "generic")):
        cin, cout = CONV_CH[kernel]
        s = 4000 + 100 * ki
        for i, wo in enumerate(CONV_WIDTHS[kernel]):
            out.append(_conv(f"w{wo}-{GEOS[i % 3]}-relu{(i + ki) % 3}", kernel, cin, cout, 2, 5, wo, GEOS[i % 3], (i + ki) % 3, s + i, "ragged"))
        out.append(_conv("ldx4-w9", kernel, cin, cout, 2, 5, 9, GEOS[1], 2, s + 20, "ldx", ldx=4))
        out.append(_conv("ldy48-w9", kernel, cin, cout, 2, 5, 9, GEOS[0], 1, s + 21, "ldy", ldy=48, lead=16))
        b, ho, c_in, c_out, relu = SECOND_PASS[kernel]
        out.append(_conv("second-pass", kernel, c_in, c_out, b, ho, 1, GEOS[2], relu, s + 30, "second_pass"))
    out.append(_conv("3to8-w6", "generic", 3, 8, 2, 5, 6, GEOS[1], 2, 4250, "ragged"))
    return out


def gap_cases(cus=None):
    out = []
    for i, hw in enumerate((1, 3, 5, 1025)):
        for j, c in enumerate((4, 252, 260, 320)):
            out.append(Case(f"gap-hw{hw}-c{c}-b{(1, 3)[(i + j) % 2]}", "gap", (1, 3)[(i + j) % 2], hw, 1, c, c, 1, 1, seed=5000 + 10 * i + j, path="plain"))
    for i, (hw, c, b) in enumerate(((5, 252, 3), (1025, 260, 1), (3, 4, 3))):
        out.append(Case(f"gap-ldx-hw{hw}-c{c}-b{b}", "gap", b, hw, 1, c, c, 1, 1, ldx=c + 12, seed=5100 + i, path="ldx"))
    return out


def _rs(id, b, h, w, c, ho, wo, seed, path, **kw):
    return Case(f"resize-{id}", "resize", b, h, w, c, c, ho, wo, kernel=resize_kernel(w, wo), seed=seed, path=path, **kw)


def resize_cases(cus=None):
    out = []
    for i, (ho, name) in enumerate(((16, "4"), (8, "2"), (4, "1"), (10, "2.5"), (2, "0.5"))):      # h_in = 4
        w_in = (2, 3, 9)[i % 3]
        out.append(_rs(f"x4-w{w_in}-hx{name}", 2, 4, w_in, 8 if i % 2 else 12, ho, 4 * w_in, 6000 + i, "x4"))
    out.append(_rs("x4-h1-w3", 2, 1, 3, 8, 4, 12, 6010, "x4"))
    out.append(_rs("x4-w9-c256", 1, 3, 9, 256, 12, 36, 6011, "x4"))                                 # 576 threads per row: 2.25 blocks
    out.append(_rs("x4-ld-w3", 2, 4, 3, 8, 10, 12, 6012, "x4", ldx=12, ldy=20, lead=4))
    out.append(_rs("gen-w1to4", 2, 3, 1, 8, 6, 4, 6020, "generic"))                                 # 4 * w_in, but w_in < 2
    out.append(_rs("gen-1x1to5x7", 2, 1, 1, 8, 5, 7, 6021, "generic"))
    out.append(_rs("gen-down-9x11to4x5", 2, 9, 11, 8, 4, 5, 6022, "generic"))
    out.append(_rs("gen-3x", 2, 4, 5, 8, 12, 15, 6023, "generic"))
    out.append(_rs("gen-2.5x", 2, 4, 6, 8, 10, 15, 6024, "generic"))
    out.append(_rs("gen-c4", 2, 4, 5, 4, 7, 9, 6025, "generic"))
    out.append(_rs("gen-ld", 2, 4, 5, 8, 7, 9, 6026, "generic", ldx=12, ldy=20, lead=4))
    out.append(_rs("gen-c260-two-blocks", 1, 3, 5, 260, 5, 9, 6027, "generic"))                     # 585 threads per row
    return out


FAMILIES = {"stem": stem_cases, "sepconv": sepconv_cases, "conv": conv_cases, "gap": gap_cases, "resize": resize_cases}


def table(cus):
    """{family: [cases]} for a device with `cus` compute units"""
    return {f: fn(cus) for f, fn in FAMILIES.items()}


def ids(family):
    """the case ids of a family; they do not depend on the CU count"""
    return [c.id for c in FAMILIES[family](256)]


def case_by_id(family, id, cus):
    return next(c for c in FAMILIES[family](cus) if c.id == id)


# ---- rejections: arguments the wrappers refuse before any launch ---------------------------------------------------------------
@dataclass(frozen=True)
class Reject:
    id: str
    entry: str
    nptr: int                   # leading pointer arguments (y is the last of them)
    ints: tuple                 # the int arguments behind them
    rc: int
    message: str                # a piece of the message asr_last_error() holds, as it stands in the source
    macro: str                  # the macro of the source line that refuses
    misalign: int = -1          # index of a pointer argument that is passed 4 bytes off


_U, _R = "ASR_UNSUPPORTED", "ASR_REQUIRE"
REJECTS = [
    Reject("stem-odd-h", "asr_entry_stem_f16x3", 6, (2, 31, 30, 3, 64), ASR_ERR_UNSUPPORTED, "even input size required", _U),
    Reject("stem-odd-w", "asr_entry_stem_f16x3", 6, (2, 30, 31, 3, 64), ASR_ERR_UNSUPPORTED, "even input size required", _U),
    Reject("stem-misaligned-w2", "asr_entry_stem_f16x3", 6, (2, 30, 30, 3, 64), ASR_ERR_UNSUPPORTED, "w2_packed must be 16-byte aligned", _U, misalign=3),
    Reject("sep-cin96", "asr_sepconv_fused_f16x3", 6, (2, 9, 15, 96, 128, 96, 128, 1, 0, 0), ASR_ERR_UNSUPPORTED, "cin in {64, 128} -> 128 only", _U),
    Reject("sep-cout64", "asr_sepconv_fused_f16x3", 6, (2, 9, 15, 64, 64, 64, 64, 1, 0, 0), ASR_ERR_UNSUPPORTED, "cin in {64, 128} -> 128 only", _U),
    Reject("sep-ldx66", "asr_sepconv_fused_f16x3", 6, (2, 9, 15, 64, 128, 66, 128, 1, 0, 0), ASR_ERR_UNSUPPORTED, "16-byte aligned x / weights required", _U),
    Reject("sep-misaligned-x", "asr_sepconv_fused_f16x3", 6, (2, 9, 15, 64, 128, 64, 128, 1, 0, 0), ASR_ERR_UNSUPPORTED, "16-byte aligned x / weights required", _U,
           misalign=0),
    Reject("mfma-stem-output-does-not-fit", "asr_conv3x3_stem_f16x3", 4, (2, 8, 8, 3, 32, 2, 0, 0, 5, 4, 3, 32, 1), ASR_ERR_INVALID_ARG, "does not fit input", _R),
    Reject("mfma-stem-cin4", "asr_conv3x3_stem_f16x3", 4, (2, 8, 8, 4, 32, 2, 0, 0, 4, 4, 4, 32, 1), ASR_ERR_UNSUPPORTED, "cin = 3, cout = 32 only", _U),
    Reject("direct-weights-beyond-lds", "asr_conv3x3_direct_f32", 4, (2, 8, 8, 32, 64, 1, 1, 1, 8, 8, 32, 64, 1), ASR_ERR_UNSUPPORTED,
           "9*cin*cout <= 12288 required", _U),
    Reject("direct-cout6", "asr_conv3x3_direct_f32", 4, (2, 8, 8, 3, 6, 1, 1, 1, 8, 8, 3, 8, 1), ASR_ERR_UNSUPPORTED, "9*cin*cout <= 12288 required", _U),
    Reject("gap-c6", "asr_gap_f32", 2, (2, 5, 6, 8), ASR_ERR_UNSUPPORTED, "c, ldx multiples of 4", _U),
]


def reject_condition_holds(r):
    """the refusing condition of the source line, restated on the arguments"""
    a = r.ints
    return {
        "stem-odd-h": lambda: (a[1] | a[2]) & 1 and a[1] & 1, "stem-odd-w": lambda: (a[1] | a[2]) & 1 and a[2] & 1,
        "stem-misaligned-w2": lambda: r.misalign == 3 and not (a[1] | a[2]) & 1,
        "sep-cin96": lambda: not (a[3] in (64, 128) and a[4] == 128) and a[4] == 128,
        "sep-cout64": lambda: not (a[3] in (64, 128) and a[4] == 128) and a[3] == 64,
        "sep-ldx66": lambda: a[5] & 3 and a[5] >= a[3], "sep-misaligned-x": lambda: r.misalign == 0 and not a[5] & 3,
        "mfma-stem-output-does-not-fit": lambda: not ((a[8] - 1) * a[5] - a[6] + 2 < a[1] + 2),
        "mfma-stem-cin4": lambda: a[3] != 3, "direct-weights-beyond-lds": lambda: 9 * a[3] * a[4] > 12288 and not a[4] & 3,
        "direct-cout6": lambda: a[4] & 3 and not a[11] & 3 and 9 * a[3] * a[4] <= 12288, "gap-c6": lambda: a[2] & 3 and not a[3] & 3,
    }[r.id]()


# ---- oracles --------------------------------------------------------------------------------------------------------------------
def _mm(a, b):
    return (torch.from_numpy(np.ascontiguousarray(a)) @ torch.from_numpy(np.ascontiguousarray(b))).numpy()


def conv3x3_f64(x, w, bias, stride, pad_top, pad_left, out_hw):
    """(bias + sum x * w, |bias| + sum |x||w|) in float64: x [b,h,w,cin], w [3,3,cin,cout]; taps outside the image skipped"""
    x = np.asarray(x, np.float64)
    w = np.asarray(w, np.float64)
    b, h, wd, cin = x.shape
    cout = w.shape[-1]
    ho, wo = out_hw
    acc = np.broadcast_to(np.asarray(bias, np.float64), (b, ho, wo, cout)).copy()
    mag = np.abs(acc)
    ax = np.abs(x)
    for ky in range(3):
        for kx in range(3):
            ya, yb = fx._tap_range(ho, h, stride, pad_top, ky)
            xa, xb = fx._tap_range(wo, wd, stride, pad_left, kx)
            if yb <= ya or xb <= xa:
                continue
            iy0, ix0 = ya * stride - pad_top + ky, xa * stride - pad_left + kx
            sl = (slice(None), slice(iy0, iy0 + (yb - ya - 1) * stride + 1, stride), slice(ix0, ix0 + (xb - xa - 1) * stride + 1, stride))
            shape = (b, yb - ya, xb - xa, cout)
            acc[:, ya:yb, xa:xb] += _mm(x[sl].reshape(-1, cin), w[ky, kx]).reshape(shape)
            mag[:, ya:yb, xa:xb] += _mm(ax[sl].reshape(-1, cin), np.abs(w[ky, kx])).reshape(shape)
    return acc, mag


def activation(v, relu):
    if relu:
        v = np.maximum(v, 0)
    if relu == 2:
        v = np.minimum(v, 6)
    return v


def gap_exact(x):
    """gap_kernel replayed in float32: x [b, hw, c]"""
    x = np.asarray(x, np.float32)
    b, hw, c = x.shape
    part = []
    for grp in range(4):
        acc = np.zeros((b, c), np.float32)
        for i in range(grp, hw, 4):
            acc = acc + x[:, i]
        part.append(acc)
    s = ((part[0] + part[1]) + part[2]) + part[3]
    return (s * (np.float32(1.0) / np.float32(hw))).astype(np.float32)


def resize_positions(n_out, n_in):
    """float64 source positions pos = q - 0.5, q = (o + 0.5) * n_in / n_out, of the outputs of one axis, and delta: how far the
    kernel's float32 position may lie from them.  One ulp_f32(max(1, |pos|)) is not enough where n_in / n_out is inexact (3x,
    2.5x, 9 -> 4): the terms are
      * scale = float32(n_in) / float32(n_out) is off by up to 2^-24 relative, which (o + 0.5) multiplies:      q * 2^-24
      * the product (o + 0.5) * scale is rounded at the magnitude of q, not of pos (absent when contracted):  ulp_f32(q) / 2
      * the subtraction of 0.5 (or the fma) is rounded at the magnitude of pos:                                 ulp_f32(pos) / 2
    (o + 0.5 itself is exact).  tests/test_layer_shapes_host.py replays both float32 forms and holds them to delta."""
    q = (np.arange(n_out) + 0.5) * (n_in / n_out)
    pos = q - 0.5
    ulp = lambda v: np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)
    delta = q * U + 0.5 * ulp(q * (1 + 2 * U)) + 0.5 * ulp(pos)
    return pos, delta


def resize_positions_f32(n_out, n_in):
    """the kernel's float32 positions, the multiply-subtract separate and contracted into one fma"""
    scale = np.float32(n_in) / np.float32(n_out)
    o = np.arange(n_out, dtype=np.float32) + np.float32(0.5)
    plain = (o * scale).astype(np.float32) - np.float32(0.5)
    fused = (o.astype(np.float64) * np.float64(scale) - 0.5).astype(np.float32)      # the product of two floats is exact in float64
    return plain, fused


def _clip(k, n):
    return np.clip(k, 0, n - 1).astype(np.int64)


def resize_f64(x, out_hw):
    """(ref, bound): the float64 bilinear resize of x [b,h,w,c] with TF half-pixel taps (lo = max(floor(pos), 0), hi =
    min(ceil(pos), n - 1), t = pos - floor(pos)) at float64 positions pos = (o + 0.5) * n_in / n_out - 0.5, and the bound on a
    float32 kernel's distance from it.

    The interpolant is continuous and piecewise linear in the position, flat outside [0, n - 1].  The kernel rounds
    (o + 0.5) * scale - 0.5 in float32 (contracted or not), which moves a position by at most delta (resize_positions: about one ulp_f32 of it);
    that moves the result by at most delta times the slope of the segments [pos - delta, pos + delta] touches (two where the
    position lies within delta of an integer): horizontally max(|tr - tl|, |br - bl|) over the rows involved, vertically
    |bot - top| at the float64 column position.  The three lerps' own roundings add 6 * 2^-24 * max |tap|."""
    x = np.asarray(x, np.float64)
    b, h, w, c = x.shape
    ho, wo = out_hw
    py, dy = resize_positions(ho, h)
    px, dx = resize_positions(wo, w)

    def xlerp(rows, kx0):
        """rows [b, ho, w, c] interpolated at the float64 column positions, on the segment kx0 -> [b, ho, wo, c]"""
        t = np.clip(px - kx0, 0.0, 1.0)[None, None, :, None]
        lo, hi = rows[:, :, _clip(kx0, w)], rows[:, :, _clip(kx0 + 1, w)]
        return lo + (hi - lo) * t

    fy, fxx = np.floor(py), np.floor(px)
    top, bot = x[:, _clip(fy, h)], x[:, _clip(np.ceil(py), h)]
    ty = (py - fy)[None, :, None, None]
    xl, xh, tx = _clip(fxx, w), _clip(np.ceil(px), w), (px - fxx)[None, None, :, None]
    t64 = top[:, :, xl] + (top[:, :, xh] - top[:, :, xl]) * tx
    b64 = bot[:, :, xl] + (bot[:, :, xh] - bot[:, :, xl]) * tx
    ref = t64 + (b64 - t64) * ty
    lx = np.zeros_like(ref)
    ly = np.zeros_like(ref)
    tap = np.zeros_like(ref)
    for ky in (np.floor(py - dy), np.floor(py + dy)):
        r0, r1 = x[:, _clip(ky, h)], x[:, _clip(ky + 1, h)]
        for kx in (np.floor(px - dx), np.floor(px + dx)):
            c0, c1 = _clip(kx, w), _clip(kx + 1, w)
            for r in (r0, r1):
                lx = np.maximum(lx, np.abs(r[:, :, c1] - r[:, :, c0]))
                tap = np.maximum(tap, np.maximum(np.abs(r[:, :, c0]), np.abs(r[:, :, c1])))
            ly = np.maximum(ly, np.abs(xlerp(r1, kx) - xlerp(r0, kx)))
    bound = dx[None, None, :, None] * lx + dy[None, :, None, None] * ly + 6 * U * tap
    return ref, bound


# ---- data -----------------------------------------------------------------------------------------------------------------------
def _normal(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def build(case, oracle=True):
    """Host operands and expectations of a case: x [b,h,w,cin], xbuf the flat input with ldx floats per pixel (gap NaN), the
    weights, and (oracle) ref64 [b,h_out,w_out,cout] with bound (same shape) or, GAP, exact (float32)."""
    c = case
    rng = np.random.default_rng(c.seed)
    d = SimpleNamespace(case=c)
    d.x = _normal(rng, c.b, c.h, c.w, c.cin, scale=c.xscale)
    xbuf = np.full((c.b * c.h * c.w, c.ld_in), np.nan, np.float32)
    xbuf[:, :c.cin] = d.x.reshape(-1, c.cin)
    d.xbuf = xbuf.reshape(-1)
    d.exact = None
    if c.family == "stem":
        d.k1, d.b1 = _normal(rng, 3, 3, 3, 32, scale=0.3), _normal(rng, 32, scale=0.2)
        d.k2, d.b2 = _normal(rng, 3, 3, 32, 64, scale=(2.0 / 288) ** 0.5), _normal(rng, 64, scale=0.2)
        if oracle:
            pre1, mag1 = conv3x3_f64(d.x, d.k1, d.b1, 2, 0, 0, (c.h_out, c.w_out))
            d.mid64 = np.maximum(pre1, 0)
            pre2, _ = conv3x3_f64(d.mid64, d.k2, d.b2, 1, 1, 1, (c.h_out, c.w_out))
            # 4e-6 * (|w2| * mid64 + |b2|) + |w2| * (4e-6 * (|w1| * |x| + |b1|)) as one convolution with |w2|
            carried, _ = conv3x3_f64(F32_GRADE * d.mid64 + F32_GRADE * mag1, np.abs(d.k2), F32_GRADE * np.abs(d.b2), 1, 1, 1, (c.h_out, c.w_out))
            d.ref64, d.bound = np.maximum(pre2, 0), carried
    elif c.family == "sepconv":
        d.wd, d.bd = _normal(rng, 3, 3, c.cin, scale=0.3), _normal(rng, c.cin, scale=0.1)
        d.wk, d.bk = _normal(rng, c.cin, c.cout, scale=(1.0 / c.cin) ** 0.5), _normal(rng, c.cout, scale=0.1)
        if oracle:
            d.a = fx.dwconv_exact(d.x, d.wd, d.bd, 1, 1, 1, 1, (c.h, c.w), c.act[0], c.act[1])
            d.ref64, d.bound = sepconv_product(d, d.a)
    elif c.family == "conv":
        d.k, d.bias = _normal(rng, 3, 3, c.cin, c.cout, scale=0.3), _normal(rng, c.cout)
        if oracle:
            d.pre64, mag = conv3x3_f64(d.x, d.k, d.bias, c.stride, c.pad, c.pad, (c.h_out, c.w_out))
            d.ref64, d.bound = activation(d.pre64, c.relu), (F32_GRADE if c.kernel == "mfma" else GAMMA28) * mag
    elif c.family == "gap":
        if oracle:
            d.exact = gap_exact(d.x.reshape(c.b, c.h, c.cin)).reshape(c.b, 1, 1, c.cin)
            d.ref64, d.bound = d.exact.astype(np.float64), np.zeros(d.exact.shape)
    elif oracle:
        d.ref64, d.bound = resize_f64(d.x, (c.h_out, c.w_out))
    return d


def sepconv_product(d, a):
    """(ref64, bound) of the pointwise stage on the depthwise output a [b,h,w,cin] (float32)"""
    c = d.case
    a64 = np.asarray(a, np.float64).reshape(-1, c.cin)
    ref = _mm(a64, d.wk.astype(np.float64)) + d.bk
    mag = _mm(np.abs(a64), np.abs(d.wk).astype(np.float64)) + np.abs(d.bk)
    return activation(ref, c.act[2]).reshape(c.b, c.h, c.w, c.cout), (F32_GRADE * mag).reshape(c.b, c.h, c.w, c.cout)


def relu6_reach(d):
    """how many float64 pre-activations of a relu = 2 convolution lie below 0, and above 6"""
    return int((d.pre64 < 0).sum()), int((d.pre64 > 6).sum())


# ---- output buffers and checks -------------------------------------------------------------------------------------------------
def out_buffer(case):
    """NaN [lead + (pixels + w_out) * ldy]: the output at channel offset `lead`, one pixel row of guard behind it"""
    return np.full(case.lead + (case.pixels + case.w_out) * case.ld_out, np.nan, np.float32)


def store(case, buf, y):
    """what a correct kernel does to the buffer with the result y [b, h_out, w_out, cout]"""
    c = case
    view = buf[c.lead:c.lead + c.pixels * c.ld_out].reshape(c.pixels, c.ld_out)
    view[:, :c.cout] = np.asarray(y).reshape(c.pixels, c.cout)
    return buf


def read_out(case, buf):
    """[b, h_out, w_out, cout] out of an output buffer; everything else must still hold the NaN prefill"""
    c = case
    assert buf.shape == out_buffer(c).shape and buf.dtype == np.float32
    end = c.lead + c.pixels * c.ld_out
    body = buf[c.lead:end].reshape(c.pixels, c.ld_out)
    for name, part in (("channel offset", buf[:c.lead]), ("ldy gap", body[:, c.cout:]), ("guard row", buf[end:])):
        written = ~np.isnan(part)
        assert not written.any(), f"{c.id}: {int(written.sum())} floats of the {name} were written"
    return body[:, :c.cout].reshape(c.b, c.h_out, c.w_out, c.cout)


def _first(mask):
    return tuple(int(i) for i in np.argwhere(mask)[0])


def check(d, got, what="kernel"):
    """got [b, h_out, w_out, cout] float32 against the case's oracle; returns the largest error as a fraction of its bound
    (GAP: the number of differing elements, which must be 0)"""
    c = d.case
    assert got.shape == d.ref64.shape and got.dtype == np.float32, (got.shape, d.ref64.shape)
    bad = ~np.isfinite(got)
    assert not bad.any(), f"{c.id} ({what}): {int(bad.sum())} non-finite outputs (prefill left, or a NaN gap column read), first at {_first(bad)}"
    if d.exact is not None:
        diff = got != d.exact
        assert not diff.any(), f"{c.id} ({what}): {int(diff.sum())} of {diff.size} outputs differ from the float32 replay, first at {_first(diff)}"
        return 0.0
    err = np.abs(got.astype(np.float64) - d.ref64)
    over = err > d.bound
    assert not over.any(), (f"{c.id} ({what}): {int(over.sum())} of {over.size} outputs beyond the bound, first at (b, y, x, ch) = {_first(over)}: "
                            f"error {err[over].max():.3e}, largest ratio {np.max(err[over] / d.bound[over]):.2f}")
    return float(np.max(err / np.maximum(d.bound, 1e-300)))


def check_buffer(d, buf, what="kernel"):
    return check(d, read_out(d.case, buf), what)


# ---- deliberately wrong producers (applied on the CPU by tests/test_layer_shapes_host.py) ----------------------------------------
MUTATIONS = ("stem_second_tile_from_first_tiles_intermediate", "sepconv_halo_row_from_previous_prefetch", "second_pass_unwritten",
             "channel_quad_shifted", "relu6_as_relu", "write_past_ragged_edge", "write_into_gap_channels", "off_by_two_bounds")


def applies(case, mutation):
    c = case
    return {"stem_second_tile_from_first_tiles_intermediate": c.family == "stem" and c.path == "walk",
            "sepconv_halo_row_from_previous_prefetch": c.family == "sepconv" and c.path.startswith("walk"),
            "second_pass_unwritten": c.path == "second_pass",
            "channel_quad_shifted": c.cout >= 8,
            "relu6_as_relu": c.family == "conv" and c.relu == 2,
            "write_past_ragged_edge": True,
            "write_into_gap_channels": c.ld_out > c.cout,
            "off_by_two_bounds": True}[mutation]


def produce(d, mutation=None, cus=256):
    """The output buffer a kernel leaves behind, computed on the CPU from the oracle (the float64 reference rounded to float32);
    mutation = one of MUTATIONS: a kernel with that defect (cus: the CU count the case was built for)."""
    c = d.case
    assert mutation is None or (mutation in MUTATIONS and applies(c, mutation)), (c.id, mutation)
    y = (d.exact if d.exact is not None else d.ref64).astype(np.float32).copy()
    if mutation == "stem_second_tile_from_first_tiles_intermediate":
        wk = stem_walk(c.b, c.h, c.w, cus)
        first, second = next(t for t in wk.of if len(t) >= 2)[:2]
        (bi, ys, xs), (bj, yt, xt) = stem_tile_region(wk, first), stem_tile_region(wk, second)
        nh, nw = min(ys.stop - ys.start, yt.stop - yt.start), min(xs.stop - xs.start, xt.stop - xt.start)
        y[bj, yt.start:yt.start + nh, xt.start:xt.start + nw] = y[bi, ys.start:ys.start + nh, xs.start:xs.start + nw]
    elif mutation == "sepconv_halo_row_from_previous_prefetch":
        wk = sepconv_walk(c.b, c.h, c.w, c.cin, cus)
        # a tile below the first tile row that is not the first of its run and whose predecessor lies in the same tile row: its
        # halo row (input row y0 - 1, columns x0 - 1 .. x0 + 14) comes from the rows the previous tile asked for
        tile = next(t for f, l in wk.runs for t in range(f + 1, l) if sepconv_tile_origin(wk, t)[1] > 0 and sepconv_tile_origin(wk, t)[2] > 0)
        img, y0, x0 = sepconv_tile_origin(wk, tile)
        xm = d.x[img:img + 1].copy()
        cols = np.arange(x0 - 1, min(x0 + SF_TW + 1, c.w))
        xm[0, y0 - 1, cols] = d.x[img, y0 - 1, np.maximum(cols - SF_TW, 0)]
        a = fx.dwconv_exact(xm, d.wd, d.bd, 1, 1, 1, 1, (c.h, c.w), c.act[0], c.act[1])
        dm = SimpleNamespace(case=replace(c, b=1), wk=d.wk, bk=d.bk)
        wrong = sepconv_product(dm, a)[0].astype(np.float32)
        y[img, y0:y0 + SF_TH, x0:x0 + SF_TW] = wrong[0, y0:y0 + SF_TH, x0:x0 + SF_TW]
    elif mutation == "second_pass_unwritten":
        wkk = conv_work(c.kernel, c.b, c.h_out, c.w_out, c.cout)
        assert c.w_out == 1 and wkk.passes == 2                  # w_out = 1: a pixel group of the stem kernels is one pixel
        if c.kernel == "generic":
            y.reshape(-1)[wkk.first_pass_groups * 4:] = np.nan
        else:
            y.reshape(-1, c.cout)[wkk.first_pass_groups:] = np.nan
    elif mutation == "channel_quad_shifted":
        y[..., 0:4], y[..., 4:8] = y[..., 4:8].copy(), y[..., 0:4].copy()
    elif mutation == "relu6_as_relu":
        y = activation(d.pre64, 1).astype(np.float32)
    elif mutation == "off_by_two_bounds":
        at = np.unravel_index(np.argmax(d.bound), d.bound.shape)
        y[at] = np.nextafter(y[at], np.float32(np.inf)) if d.exact is not None else np.float32(d.ref64[at] + 2 * d.bound[at])
    buf = store(c, out_buffer(c), y)
    if mutation == "write_past_ragged_edge":
        buf[c.lead + c.pixels * c.ld_out] = 0.0                 # the pixel behind the last one: the first of the guard row
    elif mutation == "write_into_gap_channels":
        buf[c.lead + (c.pixels // 2) * c.ld_out + c.cout] = 0.0
    return buf
