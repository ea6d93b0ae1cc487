"""Cases, seeded data and plain numpy references for the base kernels of csrc/reduce.hip (minmax, argmax, single-class OPM,
minmax_normalize, threshold, iou_counts, class_counts, class_activation) and csrc/warp.hip (warp_affine, augment_copies).  No GPU
here: tests/test_base_kernel_cases_host.py proves on the CPU that the table reaches every launch path it names, that the
references agree with oracle/ and that subtly wrong kernels fail the checks; tests/test_gpu_base_kernels.py and
tests/test_gpu_warp_shapes.py run the table on the device through the same check_* functions.

References: int64 numpy for counts, float64 for activations, and float32 restatements (every step one correctly rounded IEEE
operation, like the units built with -ffp-contract=off) where the result is defined operation by operation.  None of them calls
asr_amd.ops.  The launch geometry of the two units is restated below (minmax_grid, stream_grid, the 64 / 128 / 4096 caps); the host
test reads the same constants out of the sources, so a changed cap fails there instead of silently un-covering a path.

Out of scope, on purpose: NaN (min / max / thresholds of NaN are not exact, the kernel comments say so; the pipeline feeds logits
and normalised scores), denormals (the normalisation's flush behaviour is not pinned), infinite warp coordinates (TF, the oracle
and the kernel all give NaN there; every coordinate here is finite or belongs to a pixel that proj == 0 zeroes), more than 65535
segments (refused by the library) and the 32-bit per-thread counters' overflow (needs more than 2^32 pixels)."""
import functools
import math
import zlib

import numpy as np

f32 = np.float32
FLT_MAX = np.finfo(np.float32).max


class Case:
    def __init__(self, entry, id, **kw):
        self.entry, self.id = entry, id
        self.__dict__.update(kw)

    def __repr__(self):
        return f"{self.entry}:{self.id}"


def seed_of(case):
    return zlib.crc32(repr(case).encode())


def cdiv(a, b):
    return -(-a // b)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------------------------------------------
# launch geometry of reduce.hip / warp.hip
# ---------------------------------------------------------------------------------------------------------------------------
MINMAX_BLOCK = 1024          # threads of a minmax workgroup: a workgroup's share is every grid-th run of 1024 elements
MINMAX_SPLIT = 16384         # elements per workgroup before a segment is split
MINMAX_WG_CAP = 1024         # workgroups of a launch: at most 1024 / segments per segment (1 from 1024 segments on)
BLOCK = 256                  # threads (= pixels of a tile) of every other kernel here
STREAM_CAP = 2048            # stream_grid
IOU_CAP = 64                 # iou_counts, iou_counts_shared_truth
COUNTS_CAP = 64              # class_counts
IOU_CLASSES_CAP = 128        # iou_counts_classes
WARP_CAP = 4096              # warp_affine (256 CUs x 16 blocks)
MAX_STAGE_CLASSES = 32       # rows of up to 32 classes go through LDS
MAX_IOU_MASKS = 8
MAX_GRID_YZ = 65535


def minmax_grid(per, segments):
    cap = 1 if segments >= MINMAX_WG_CAP else MINMAX_WG_CAP // segments
    return min(cdiv(per, MINMAX_SPLIT), cap)


def minmax_share(per, grid, b):
    """indices of workgroup b's share of a segment, ascending"""
    i = np.arange(per, dtype=np.int64)
    return i[(i // MINMAX_BLOCK) % grid == b]


def stream_grid(n):
    return min(max(cdiv(n, BLOCK), 1), STREAM_CAP)


def capped_grid(n, cap):
    return min(stream_grid(n), cap)


def warp_grid(total):
    return min(cdiv(total, BLOCK), WARP_CAP)


def passes(n, grid):
    return cdiv(n, grid * BLOCK)


def second_pass_tiles(n, grid):
    """(full, ragged) tiles of 256 that a grid of `grid` workgroups reaches only in its second or a later trip"""
    first = grid * BLOCK
    if n <= first:
        return 0, 0
    return (n - first) // BLOCK, int((n - first) % BLOCK != 0)


def staged(classes):
    return classes <= MAX_STAGE_CLASSES


# ---------------------------------------------------------------------------------------------------------------------------
# minmax
# ---------------------------------------------------------------------------------------------------------------------------
MINMAX_KINDS = ("neg", "mixed", "pos", "zeros", "fltmax", "inf")     # a segment's kind is (kind0 + segment) mod 6


def _minmax_kind(kind, s):
    """(body lo, body hi, planted minimum, planted maximum) of segment s: same-kind segments differ through d"""
    d = f32(s % 50)
    if kind == "neg":
        hi = -(f32(100) + 2 * d)
        return hi - f32(1.5), hi, hi - f32(1.75), hi + f32(0.25)
    if kind == "pos":
        lo = f32(100) + 2 * d
        return lo, lo + f32(1.5), lo - f32(0.25), lo + f32(1.75)
    if kind == "mixed":
        return f32(-1), f32(1), -(f32(1.5) + d / 64), f32(1.5) + d / 64
    if kind == "zeros":
        return f32(0), f32(0), f32(-0.0), f32(0.0)
    if kind == "fltmax":
        return f32(-1e30), f32(1e30), -FLT_MAX, FLT_MAX
    return f32(-5), f32(5), f32(-np.inf), f32(np.inf)


def minmax_kinds(case):
    return [MINMAX_KINDS[(case.kind0 + s) % 6] for s in range(case.segments)]


@functools.lru_cache(maxsize=2)
def _minmax_body(per, segments, kind0):
    rng = np.random.default_rng(1000 * kind0 + segments + per % 997)
    u = rng.random((segments, per), dtype=np.float32)
    kinds = [MINMAX_KINDS[(kind0 + s) % 6] for s in range(segments)]
    rows = [_minmax_kind(k, s) for s, k in enumerate(kinds)]
    lo = np.array([r[0] for r in rows], np.float32)[:, None]
    hi = np.array([r[1] for r in rows], np.float32)[:, None]
    x = lo + u * (hi - lo)
    for s, k in enumerate(kinds):
        if k == "zeros":
            x[s] = np.where(u[s] < 0.5, f32(-0.0), f32(0.0))
    x.setflags(write=False)
    return x


def minmax_position_indices(per, segments):
    """name -> (index of the minimum, index of the maximum); names whose indices repeat an earlier one are left out"""
    g = minmax_grid(per, segments)
    named = [("e0", (0, per - 1)), ("last", (per - 1, 0))]
    if g > 1:
        last_chunk = (per - 1) // MINMAX_BLOCK
        for j in range(g):
            first = j * MINMAX_BLOCK
            k = last_chunk - ((last_chunk - j) % g)
            last = min(per, (k + 1) * MINMAX_BLOCK) - 1
            named += [(f"wg{j}_first", (first, last)), (f"wg{j}_last", (last, first))]
    out, seen = {}, set()
    for name, pair in named:
        if pair not in seen:
            seen.add(pair)
            out[name] = pair
    return out


def build_minmax(case):
    """-> x [segments, per] f32 (a fresh writable copy), planted [segments, 2]"""
    x = _minmax_body(case.per, case.segments, case.kind0).copy()
    imin, imax = minmax_position_indices(case.per, case.segments)[case.position]
    planted = np.empty((case.segments, 2), np.float32)
    for s, k in enumerate(minmax_kinds(case)):
        _, _, mn, mx = _minmax_kind(k, s)
        if case.per == 1:
            mx = mn
        x[s, imax] = mx
        x[s, imin] = mn
        planted[s] = (mn, mx)
    return x, planted


def minmax_ref(x):
    return np.stack([np.min(x, axis=1), np.max(x, axis=1)], axis=1)


def check_minmax(case, x, got):
    ref = minmax_ref(x)
    assert got.shape == ref.shape and got.dtype == np.float32, (case.id, got.shape, got.dtype)
    bad = np.flatnonzero(~(got == ref).all(axis=1))          # ==: the sign of a zero extreme is not pinned
    assert bad.size == 0, (case.id, "segment", int(bad[0]), got[bad[0]].tolist(), ref[bad[0]].tolist(), minmax_kinds(case)[bad[0]])


def _minmax_cases():
    out = []

    def add(per, segments, kind0s):
        for kind0 in kind0s:
            for pos in minmax_position_indices(per, segments):
                out.append(Case("minmax", f"p{per}_s{segments}_k{kind0}_{pos}", per=per, segments=segments, kind0=kind0, position=pos))

    for per in (1, 63, 64, 65, 1023, 1024, 1025, 16384, 16385, 3 * 16384 + 5):
        add(per, 1, range(6))
        add(per, 3, (0, 3))
    add(5 * 16384 + 1, 7, (0,))            # uncapped: 6 workgroups per segment
    add(4 * 16384 + 5, 300, (0,))          # capped from 5 to 3 workgroups: each runs on into what a fourth and fifth would take
    add(16385, 1024, (0,))                 # one workgroup per segment
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# minmax_normalize / opm_slice: new_min + ((x - mn) * span) / den in float32, den = 1 when mx == mn
# ---------------------------------------------------------------------------------------------------------------------------
def normalize_ref(x, mn, mx, new_min, new_max):
    """x f32 array, mn / mx f32 scalars: the kernel's statements, one rounding each"""
    x = np.asarray(x, np.float32)
    mn, mx = f32(mn), f32(mx)
    d = mx - mn
    den = d if d != 0 else f32(1)
    span = f32(new_max) - f32(new_min)
    return (f32(new_min) + ((x - mn) * span) / den).astype(np.float32)


def _norm_segments(case, rng):
    shape = (case.segments, case.per)
    x = rng.standard_normal(shape).astype(np.float32)
    if case.data == "neg":
        x = (-np.abs(x) - f32(2)).astype(np.float32)
    elif case.data == "const_mid":
        x[1] = f32(-3.25)
        x[2] *= f32(1e4)                       # per-segment extrema 1e4 apart
    return x


def build_normalize(case):
    return _norm_segments(case, np.random.default_rng(seed_of(case)))


def normalize_segments_ref(case, x):
    return np.stack([normalize_ref(s, s.min(), s.max(), case.new_min, case.new_max) for s in x])


def check_normalize(case, x, got):
    ref = normalize_segments_ref(case, x)
    assert got.shape == ref.shape and got.dtype == np.float32, case.id
    bad = np.argwhere(bits(got) != bits(ref))
    assert bad.size == 0, (case.id, len(bad), bad[0].tolist(), float(got[tuple(bad[0])]), float(ref[tuple(bad[0])]))


def _normalize_cases():
    out = []
    for new_min, new_max in ((0.0, 1.0), (-1.0, 1.0), (0.0, 255.0)):
        tag = f"{new_min:g}_{new_max:g}"
        out.append(Case("normalize", f"split_neg_{tag}", per=2 * 16384 + 5, segments=1, data="neg", new_min=new_min, new_max=new_max))
        out.append(Case("normalize", f"const_mid_{tag}", per=1000, segments=3, data="const_mid", new_min=new_min, new_max=new_max))
        out.append(Case("normalize", f"const_mid_split_{tag}", per=16385, segments=3, data="const_mid", new_min=new_min,
                        new_max=new_max))
    return out


def build_opm_slice(case):
    """-> logits [copies, per_copy, classes]: copy 1 constant, copy 2 scaled to 1e4, all of copy 0 negative when asked"""
    rng = np.random.default_rng(seed_of(case))
    x = rng.standard_normal((case.copies, case.per_copy, case.classes)).astype(np.float32)
    if case.data == "neg":
        x = (-np.abs(x) - f32(2)).astype(np.float32)
    if case.copies > 1:
        x[1] = f32(0.75)
    if case.copies > 2:
        x[2] *= f32(1e4)
    return x


def opm_slice_ref(case, x, class_id):
    return np.stack([normalize_ref(c[:, class_id], c.min(), c.max(), case.new_min, case.new_max) for c in x])


def check_opm_slice(case, x, class_id, got):
    ref = opm_slice_ref(case, x, class_id)
    assert got.shape == ref.shape and got.dtype == np.float32, (case.id, class_id)
    bad = np.argwhere(bits(got) != bits(ref))
    assert bad.size == 0, (case.id, class_id, len(bad), bad[0].tolist(), float(got[tuple(bad[0])]), float(ref[tuple(bad[0])]))


def _opm_slice_cases():
    out = []
    for classes, per_copy in ((1, 257), (21, 257), (21, 1000), (33, 600), (32, 256)):     # 21 x 1000, 33 x 600: a split min/max
        for new_min, new_max in ((0.0, 1.0), (-1.0, 1.0), (0.0, 255.0)):
            for copies, data in ((3, "normal"), (1, "neg")):
                out.append(Case("opm_slice", f"c{classes}_p{per_copy}_n{copies}_{data}_{new_min:g}_{new_max:g}", classes=classes,
                                per_copy=per_copy, copies=copies, data=data, new_min=new_min, new_max=new_max,
                                class_ids=sorted({0, classes // 2, classes - 1})))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# logits for argmax / opm_argmax / opm_slice_max
# ---------------------------------------------------------------------------------------------------------------------------
LOGIT_SHAPE = (3, 37, 41)    # copies, h, w of the class-set tests: 1517 pixels per copy, 4551 in all


def first_argmax(x):
    return np.argmax(x, axis=-1)             # numpy: first maximum, like tf.argmax and the kernels


def make_logits(classes, ids, seed, shape=LOGIT_SHAPE):
    """Seeded [*shape, classes] logits in which every id of `ids` wins >= 1 % of the pixels and ties for the maximum
    on some; rows of +-0.0 maxima and rows scaled to ~1e4."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    x = rng.standard_normal((n, classes)).astype(np.float32)
    big = rng.random(n) < 0.2
    x[big] *= np.float32(1e4)
    order = rng.permutation(n)
    per = max(n // 60, 1)                    # 1.7 % of the pixels per id: strict wins
    cur = 0
    for c in ids:
        rows = order[cur:cur + per]
        cur += per
        x[rows, c] = np.abs(x[rows]).max(axis=1) + np.float32(1.0)
    for c in ids:                            # exact ties for the maximum: with the next class, and with the previous one
        for other in ((c + 1) % classes, (c - 1) % classes):
            rows = order[cur:cur + 3]
            cur += 3
            m = np.abs(x[rows]).max(axis=1) + np.float32(2.0)
            x[rows, c] = m
            x[rows, other] = m
    for c in ids:                            # +-0.0: the maximum is a zero of either sign
        rows = order[cur:cur + 2]
        cur += 2
        x[rows] = -np.abs(x[rows]) - np.float32(1.0)
        x[rows, c] = np.float32(-0.0)
        x[rows, (c + 3) % classes] = np.float32(0.0)
    assert cur < n
    # the non-vacuity condition, checked on the host
    arg = first_argmax(x)
    rowmax = x.max(axis=1)
    for c in ids:
        assert (arg == c).mean() >= 0.01, c
        at_max = x == rowmax[:, None]
        assert (at_max[:, c] & (at_max.sum(axis=1) >= 2)).any(), c
    assert (x == 0).any() and np.signbit(x[x == 0]).any() and (~np.signbit(x[x == 0])).any()
    assert np.abs(x).max() > 1e4
    return x.reshape(tuple(shape) + (classes,))


BIG_PIXELS = STREAM_CAP * BLOCK + 257        # a second trip of one full tile and a one-row tile
LOGIT_PIXELS = (1, 255, 256, 257)
LOGIT_CLASSES = (1, 2, 21, 32, 33, 40)
BIG_CLASSES = (21, 33)


def _row_kind(x, r, c, kind):
    """row r becomes a strict win of class c (0), a tie of c with the next (1) or with the previous class (2)"""
    classes = x.shape[1]
    m = np.abs(x[r][np.isfinite(x[r])]).max(initial=0) + f32(1 + (kind > 0))
    x[r, c] = m
    if kind == 1:
        x[r, (c + 1) % classes] = m
    elif kind == 2:
        x[r, (c - 1) % classes] = m


def _special_rows(x, rows):
    """rows of all -inf, rows with one +inf, a row with +inf in the first and the last class"""
    classes = x.shape[1]
    rows = list(rows)
    for i, r in enumerate(rows[:2]):
        x[r] = f32(-np.inf)
    for i, r in enumerate(rows[2:4]):
        x[r, (7 * i + 1) % classes] = f32(np.inf)
    for r in rows[4:5]:
        x[r, 0] = x[r, classes - 1] = f32(np.inf)


def small_logits(classes, pixels, seed):
    """make_logits' rows for pixel counts too small for it: as many of the rows as fit, wins first"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((pixels, classes)).astype(np.float32)
    x[rng.random(pixels) < 0.2] *= f32(1e4)
    order = list(rng.permutation(pixels))
    take = lambda k: [order.pop() for _ in range(min(k, len(order)))]
    for c in range(classes):
        for r in take(max(math.ceil(0.01 * pixels), 1)):
            _row_kind(x, r, c, 0)
    for c in range(classes):
        for kind in ((1, 2) if classes > 2 else (1,) if classes == 2 else ()):
            for r in take(1):
                _row_kind(x, r, c, kind)
    for c in range(min(classes, 3)):
        for r in take(1):
            x[r] = -np.abs(x[r]) - f32(1)
            x[r, c] = f32(-0.0)
            if classes > 1:
                x[r, (c + 3) % classes if (c + 3) % classes != c else (c + 1) % classes] = f32(0.0)
    _special_rows(x, take(5))
    return x


@functools.lru_cache(maxsize=2)
def _big_logits(classes):
    x = make_logits(classes, list(range(classes)), seed=classes, shape=(BIG_PIXELS,))
    first = STREAM_CAP * BLOCK
    for j in range(BIG_PIXELS - first - 1):          # the second trip's full tile: wins and both ties of every class
        _row_kind(x, first + j, j % classes, (j // classes) % 3)
    _row_kind(x, BIG_PIXELS - 1, classes - 2, 1)     # the one-row tile: the last two classes tie
    _special_rows(x, [5, first - 3, first + 250, 77, first + 251])
    x.setflags(write=False)
    return x


def build_logits(case):
    """-> [pixels, classes] f32 (the big ones are cached and read-only)"""
    if case.pixels == BIG_PIXELS:
        return _big_logits(case.classes)
    return small_logits(case.classes, case.pixels, seed_of(case))


def free_big():
    _big_logits.cache_clear()
    _minmax_body.cache_clear()
    _big_activation.cache_clear()


def _logit_cases(entry, min_classes=1):
    out = []
    for classes in LOGIT_CLASSES:
        if classes < min_classes:
            continue
        for pixels in LOGIT_PIXELS + ((BIG_PIXELS,) if classes in BIG_CLASSES else ()):
            out.append(Case(entry, f"c{classes}_p{pixels}", classes=classes, pixels=pixels,
                            class_ids=sorted({0, classes // 2, classes - 1})))
    return out


def argmax_ref(x, last=False):
    if last:
        return (x.shape[-1] - 1 - np.argmax(x[..., ::-1], axis=-1)).astype(np.int32)
    return np.argmax(x, axis=-1).astype(np.int32)


def check_argmax(case, x, got):
    ref = argmax_ref(x)
    assert got.shape == ref.shape and got.dtype == np.int32, case.id
    bad = np.flatnonzero(got != ref)
    assert bad.size == 0, (case.id, len(bad), int(bad[0]), int(got[bad[0]]), int(ref[bad[0]]))


def opm_argmax_ref(x, class_id):
    return np.where(np.argmax(x, axis=-1) == class_id, class_id, 0).astype(np.float32)


def check_opm_argmax(case, x, class_id, got):
    ref = opm_argmax_ref(x, class_id)
    assert got.shape == ref.shape and got.dtype == np.float32, (case.id, class_id)
    bad = np.flatnonzero(bits(got) != bits(ref))
    assert bad.size == 0, (case.id, class_id, len(bad), int(bad[0]), float(got[bad[0]]), float(ref[bad[0]]))


def slice_max_ref(x, class_id):
    return x[:, class_id].copy(), np.delete(x, class_id, axis=1).max(axis=1)


def check_slice_max(case, x, class_id, got_cls, got_max):
    cls, mx = slice_max_ref(x, class_id)
    assert got_cls.shape == cls.shape and got_max.shape == mx.shape, (case.id, class_id)
    bad = np.flatnonzero(bits(got_cls) != bits(cls))
    assert bad.size == 0, (case.id, class_id, "class plane", len(bad), int(bad[0]))
    bad = np.flatnonzero(~(got_max == mx))             # ==: a maximum among zeros of both signs has no pinned sign
    assert bad.size == 0, (case.id, class_id, "max plane", len(bad), int(bad[0]), float(got_max[bad[0]]), float(mx[bad[0]]))


# ---------------------------------------------------------------------------------------------------------------------------
# class_activation: float64 softmax / sigmoid; bounds of test_class_activation_matches_torch
# ---------------------------------------------------------------------------------------------------------------------------
ACT_RTOL, ACT_ATOL, ACT_SUM_ATOL = 2e-6, 1e-7, 1e-6


def _activation_data(classes, pixels, seed):
    return (3.0 * np.random.default_rng(seed).standard_normal((pixels, classes))).astype(np.float32)


@functools.lru_cache(maxsize=2)
def _big_activation(classes):
    x = _activation_data(classes, BIG_PIXELS, 31 + classes)
    x.setflags(write=False)
    return x


def build_activation(case):
    if case.pixels == BIG_PIXELS:
        return _big_activation(case.classes)
    return _activation_data(case.classes, case.pixels, seed_of(case))


def activation_ref64(x, kind):
    x = np.asarray(x, np.float64)
    if kind == "sigmoid":
        return 1.0 / (1.0 + np.exp(-x))
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def activation_f32(x, kind):
    """the kernel's statements in numpy float32 (numpy's expf is not the device's: inside the bounds, not bit for bit)"""
    x = np.asarray(x, np.float32)
    if kind == "sigmoid":
        return (f32(1) / (f32(1) + np.exp(-x))).astype(np.float32)
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    s = np.zeros(x.shape[:-1], np.float32)
    for c in range(x.shape[-1]):                       # the kernel's sum, in class order
        s = s + e[..., c]
    return (e / s[..., None]).astype(np.float32)


def check_activation(case, x, kind, got):
    """-> largest |got - float64|"""
    ref = activation_ref64(x, kind)
    assert got.shape == ref.shape and got.dtype == np.float32, (case.id, kind)
    err = np.abs(got - ref)
    bad = np.argwhere(~(err <= ACT_ATOL + ACT_RTOL * np.abs(ref)))
    assert bad.size == 0, (case.id, kind, len(bad), bad[0].tolist(), float(got[tuple(bad[0])]), float(ref[tuple(bad[0])]))
    if kind == "softmax":
        s = np.abs(got.astype(np.float64).sum(axis=-1) - 1.0)
        assert (s <= ACT_SUM_ATOL).all(), (case.id, "row sums", float(s.max()))
    return float(err.max())


# ---------------------------------------------------------------------------------------------------------------------------
# threshold: image > f32(max) * f32(factor) (the float32 product, strict), or image >= th_mask
# ---------------------------------------------------------------------------------------------------------------------------
THRESHOLD_KINDS = {"negmax": 1.5, "zero": 0.0, "one": 1.0, "negfactor": -0.5, "f32prod": 0.15, "mask": 0.15}
THRESHOLD_PERS = (257, 16385, STREAM_CAP * BLOCK + 300)


def rounds_up_max(start, factor):
    """the first float32 m >= start whose float32 product with `factor` lies above the exact product"""
    m, fac = f32(start), f32(factor)
    while not float(m * fac) > float(m) * float(fac):
        m = np.nextafter(m, f32(np.inf))
    return m


def build_threshold(case):
    """-> image [segments, per] f32, th_mask (same shape) or None, factor (python float of a float32), th_value"""
    rng = np.random.default_rng(seed_of(case))
    S, per = case.segments, case.per
    fac = float(f32(THRESHOLD_KINDS[case.kind]))
    u = rng.random((S, per), dtype=np.float32)
    some = lambda frac: np.unique(np.concatenate([[0, per - 1, per // 3], np.flatnonzero(rng.random(per) < frac)]))
    img = np.empty((S, per), np.float32)
    mask = None
    for s in range(S):
        if case.kind == "negmax":                         # all negative: the threshold 1.5 * max lies below the maximum
            mx = f32(-(2 + s))
            img[s] = mx - f32(4) * u[s]
            img[s, some(0.01)] = mx * f32(fac)            # equal to the threshold: off
        elif case.kind == "mask":
            img[s] = rng.standard_normal(per).astype(np.float32) * f32(s + 1)
        else:
            mx = rounds_up_max(3 + s, fac) if case.kind == "f32prod" else f32(3 + s)
            img[s] = mx * (u[s] if case.kind == "f32prod" else (2 * u[s] - 1))
            img[s] = np.minimum(img[s], np.nextafter(mx, f32(0)))
            img[s, some(0.01)] = mx * f32(fac)            # equal to the threshold: off (zero: +0.0 against a +0.0 threshold)
            if case.kind == "zero":
                img[s, some(0.01)[1:]] = f32(-0.0)
            if case.kind == "one":
                img[s, some(0.005)] = mx                  # several pixels at the maximum: none above it
        if case.kind != "mask":
            img[s, per // 2] = mx
    if case.kind == "mask":
        mask = (rng.standard_normal((S, per)).astype(np.float32))
        for s in range(S):
            eq = some(0.05)
            mask[s, eq] = img[s, eq]                      # equal values: on
            z = some(0.01)
            img[s, z], mask[s, z] = f32(-0.0), f32(0.0)   # -0.0 >= +0.0: on
            z = some(0.01)[2:]
            img[s, z], mask[s, z] = f32(0.0), f32(-0.0)
    return img, mask, fac, (255 if case.kind == "mask" else 8)


def threshold_ref(img, mask, fac, value, ge=False, mask_gt=False, f64=False, seg0=False):
    out = np.empty(img.shape, np.int32)
    for s in range(img.shape[0]):
        if mask is not None:
            on = img[s] > mask[s] if mask_gt else img[s] >= mask[s]
        else:
            mx = f32(img[0 if seg0 else s].max())
            th = float(mx) * float(f32(fac)) if f64 else f32(mx * f32(fac))
            x = img[s].astype(np.float64) if f64 else img[s]
            on = x >= th if ge else x > th
        out[s] = np.where(on, value, 0)
    return out


def check_threshold(case, data, got):
    img, mask, fac, value = data
    ref = threshold_ref(img, mask, fac, value)
    assert got.shape == ref.shape and got.dtype == np.int32, case.id
    bad = np.argwhere(got != ref)
    assert bad.size == 0, (case.id, len(bad), bad[0].tolist(), int(got[tuple(bad[0])]), int(ref[tuple(bad[0])]))


def _threshold_cases():
    return [Case("threshold", f"p{per}_s{S}_{kind}", per=per, segments=S, kind=kind)
            for per in THRESHOLD_PERS for S in (1, 3) for kind in THRESHOLD_KINDS]


# ---------------------------------------------------------------------------------------------------------------------------
# iou_counts: counts[seg] = {inter_c, union_c, inter_bg, union_bg}; include_bg first sets every truth label != class_id to 0
# ---------------------------------------------------------------------------------------------------------------------------
IOU_TRUTH_LABELS = (0, 8, 3, 255, -1, 300)
IOU_PERS = (255, 16384, 16385, IOU_CAP * BLOCK * 3 + 77)


def iou_ref(t, p, class_id, include_bg, no_remap=False, skip255=False):
    """t, p int arrays of one segment -> int64 [4]"""
    t, p = np.asarray(t).reshape(-1), np.asarray(p).reshape(-1)
    if skip255:
        keep = t != 255
        t, p = t[keep], p[keep]
    if include_bg and not no_remap:
        t = np.where(t != class_id, 0, t)
    tc, pc, tb, pb = t == class_id, p == class_id, t == 0, p == 0
    return np.array([(tc & pc).sum(), (tc | pc).sum(), (tb & pb).sum(), (tb | pb).sum()], np.int64)


def iou_ratio(counts, include_bg):
    """what oracle.augment.single_class_IOU makes of the counts: the mean of the defined ratios"""
    r = [np.float64(counts[0]) / np.float64(counts[1])] if counts[1] else []
    if include_bg and counts[3]:
        r.append(np.float64(counts[2]) / np.float64(counts[3]))
    return float(np.mean(r)) if r else float("nan")


def _mask_of(rng, n, class_id, p_on):
    strays = [l for l in (3, 255, -1, 300, 8) if l != class_id]
    m = np.where(rng.random(n) < p_on, class_id, 0).astype(np.int32)
    at = rng.random(n) < 0.01
    m[at] = rng.choice(strays, size=int(at.sum()))
    return m


def build_iou(case):
    """-> truth [segments, per] (shared: [per]), pred [segments, per] int32"""
    rng = np.random.default_rng(seed_of(case))
    S, per = case.segments, case.per
    truth = rng.choice(np.array(IOU_TRUTH_LABELS, np.int32), size=(per,) if case.shared else (S, per)).astype(np.int32)
    pred = np.stack([_mask_of(rng, per, case.class_id, 0.25 + 0.15 * s) for s in range(S)])
    return truth, pred


def iou_case_ref(case, truth, pred, **mut):
    return np.stack([iou_ref(truth if case.shared else truth[s], pred[s], case.class_id, case.include_bg, **mut)
                     for s in range(case.segments)])


def check_iou(case, data, got):
    truth, pred = data
    ref = iou_case_ref(case, truth, pred)
    assert got.shape == ref.shape and got.dtype == np.int64, case.id
    assert np.array_equal(got, ref), (case.id, got.tolist(), ref.tolist())


def _iou_cases():
    out = []
    for shared in (False, True):
        for per in IOU_PERS:
            for S in ((4,) if shared else (1, 4)):
                for class_id in (0, 8, 255):
                    for bg in (False, True):
                        out.append(Case("iou_shared" if shared else "iou", f"p{per}_s{S}_c{class_id}_bg{int(bg)}", per=per, segments=S,
                                        class_id=class_id, include_bg=bg, shared=shared))
    return out


IOU_CLASSES_PIXELS = IOU_CLASSES_CAP * BLOCK + BLOCK + 77     # a second trip of one full and one ragged tile


def build_iou_classes(case):
    """-> ids, truth [pixels], preds [K, M, pixels] int32"""
    rng = np.random.default_rng(seed_of(case))
    ids = [8] if case.K == 1 else [int(c) for c in rng.permutation(21)]
    truth = rng.choice(np.array(ids + [0, 255, -1, 300], np.int32), size=case.pixels).astype(np.int32)
    preds = np.stack([np.stack([_mask_of(rng, case.pixels, c, 0.2 + 0.08 * m) for m in range(case.M)]) for c in ids])
    return ids, truth, preds


def iou_classes_ref(case, ids, truth, preds):
    return np.stack([np.stack([iou_ref(truth, preds[k, m], c, case.include_bg) for m in range(case.M)]) for k, c in enumerate(ids)])


def check_iou_classes(case, data, got):
    ids, truth, preds = data
    ref = iou_classes_ref(case, ids, truth, preds)
    assert got.shape == ref.shape and got.dtype == np.int64, case.id
    bad = np.argwhere(got != ref)
    assert bad.size == 0, (case.id, len(bad), bad[0].tolist(), int(got[tuple(bad[0])]), int(ref[tuple(bad[0])]))


def _iou_classes_cases():
    return [Case("iou_classes", f"m{M}_k{K}_bg{int(bg)}", M=M, K=K, include_bg=bg, pixels=IOU_CLASSES_PIXELS)
            for M in (1, 8) for K in (1, 21) for bg in (False, True)]


# ---------------------------------------------------------------------------------------------------------------------------
# class_counts: [segments, 3, 256] = |truth == l|, |pred == l|, |truth == l & pred == l|; labels outside 0..255 count nowhere
# ---------------------------------------------------------------------------------------------------------------------------
OUT_OF_RANGE_LABELS = (-1, 256, 511, 1000, np.iinfo(np.int32).min, np.iinfo(np.int32).max)
COUNTS_PERS = (1, 255, 16385, COUNTS_CAP * BLOCK * 2 + 9)


def build_class_counts(case):
    """-> truth, pred [segments, per] int32, keep [segments, per] bool (False where an out-of-range label was planted)"""
    rng = np.random.default_rng(seed_of(case))
    S, per = case.segments, case.per
    truth = np.empty((S, per), np.int32)
    pred = np.empty((S, per), np.int32)
    keep_t = np.ones((S, per), bool)
    keep_p = np.ones((S, per), bool)
    for s in range(S):
        if case.kind == "single":
            truth[s] = pred[s] = 17 + s
            continue
        labels = np.arange(s, 256, S, dtype=np.int32)          # segments == 1: all of 0..255; else the segment's residue class
        truth[s] = rng.choice(labels, size=per)
        pred[s] = np.where(rng.random(per) < 0.5, truth[s], rng.choice(labels, size=per))
        if case.kind == "outside":
            oor = np.array(OUT_OF_RANGE_LABELS, np.int32)
            for arr, keep in ((truth, keep_t), (pred, keep_p)):
                at = rng.random(per) < 0.1
                arr[s, at] = rng.choice(oor, size=int(at.sum()))
                keep[s, at] = False
            both = rng.random(per) < 0.05                      # the same out-of-range label on both sides
            truth[s, both] = pred[s, both] = rng.choice(oor, size=int(both.sum()))
            keep_t[s, both] = keep_p[s, both] = False
            if per >= len(oor):
                truth[s, :len(oor)] = pred[s, :len(oor)] = oor
                keep_t[s, :len(oor)] = keep_p[s, :len(oor)] = False
    return truth, pred, (keep_t, keep_p)


def class_counts_ref(truth, pred, and255=False, both_outside=False):
    out = np.zeros((truth.shape[0], 3, 256), np.int64)
    for s in range(truth.shape[0]):
        t, p = truth[s].astype(np.int64), pred[s].astype(np.int64)
        if and255:
            t, p = t & 255, p & 255
        ok_t, ok_p = (t >= 0) & (t < 256), (p >= 0) & (p < 256)
        out[s, 0] = np.bincount(t[ok_t], minlength=256)
        out[s, 1] = np.bincount(p[ok_p], minlength=256)
        out[s, 2] = np.bincount(t[ok_t & (t == p)], minlength=256)
        if both_outside:                                       # an equal pair outside 0..255 counted into the bin its low bits name
            out[s, 2] += np.bincount(t[~ok_t & (t == p)] & 255, minlength=256)
    return out


def mean_iou_of_counts(c):
    """oracle.augment.Mean_IOU from one segment's counts (labels in 0..255 only): labels present in the truth, 255 left out"""
    ious = [c[2, l] / (c[0, l] + c[1, l] - c[2, l]) for l in range(256) if c[0, l] and l != 255]
    return float(np.mean(ious)) if ious else float("nan")


def check_class_counts(case, data, got):
    truth, pred, _ = data
    ref = class_counts_ref(truth, pred)
    assert got.shape == ref.shape and got.dtype == np.int64, case.id
    bad = np.argwhere(got != ref)
    assert bad.size == 0, (case.id, len(bad), bad[0].tolist(), int(got[tuple(bad[0])]), int(ref[tuple(bad[0])]))


def _class_counts_cases():
    out = [Case("class_counts", f"p{per}_s{S}_{kind}", per=per, segments=S, kind=kind)
           for per in COUNTS_PERS for S in (1, 3) for kind in ("uniform", "single", "outside")]
    out.append(Case("class_counts", "p40000_s1_single", per=40000, segments=1, kind="single"))     # 40000 adds to one bin
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# warps: ImageProjectiveTransformV3 restated in numpy float32, statement by statement as asr_warp_device.h has it
# ---------------------------------------------------------------------------------------------------------------------------
WARP_ATOL = 1e-6             # test_warp_affine_matches_oracle's bound, images in [0, 1)
WARP_IN = (9, 13)
WARP_OUTS = {"same": (9, 13), "11x17": (11, 17), "1x1": (1, 1), "5x300": (5, 300)}
WARP_CHANNELS = (1, 2, 3, 4, 21)
WARP_BATCH = 3


def rotation_tf(angle, h, w):
    """tfa.image.angles_to_projective_transforms for one angle"""
    a = f32(angle)
    cos, sin = f32(np.cos(a)), f32(np.sin(a))
    xo = ((f32(w) - 1) - (cos * (f32(w) - 1) - sin * (f32(h) - 1))) / f32(2)
    yo = ((f32(h) - 1) - (sin * (f32(w) - 1) + cos * (f32(h) - 1))) / f32(2)
    return np.array([cos, -sin, xo, sin, cos, yo, 0, 0], np.float32)


def shift_tf(dx, dy):
    return np.array([1, 0, -f32(dx), 0, 1, -f32(dy), 0, 0], np.float32)


def _warp_transforms():
    h, w = WARP_IN
    t = {
        "identity": shift_tf(0, 0),
        "int_shift": shift_tf(2, -1),
        "rot0.3": rotation_tf(0.3, h, w),
        "rot_pi2": rotation_tf(np.pi / 2, h, w),
        "rot_pi": rotation_tf(np.pi, h, w),
        "rot-3": rotation_tf(-3.0, h, w),
        "shift7.25_-3.5": shift_tf(7.25, -3.5),
        "shift+0.5": shift_tf(0.5, 0),
        "shift-0.5": shift_tf(-0.5, 0),
        "past_frame": shift_tf(400, 0),                  # every tap out of frame, at every output size
        "frac_neg": shift_tf(0.25, 0.75),                # coordinates in (-1, 0) on both axes: floorf and (int) disagree
        "far": np.array([1e8, 0, 3e9, 0, 1e8, -3e9, 0, 0], np.float32),      # finite, beyond the int range
        "proj_neg": np.array([1, 0, -10, 0, 0.2, -2.4, -0.15, 0], np.float32),     # proj < 0 from x = 7 on, in frame there
        "proj_zero": np.array([1, 0, 0.5, 0, 1, 0.5, -0.125, 0], np.float32),      # proj == 0 exactly at x = 8
    }
    return t


WARP_TRANSFORMS = _warp_transforms()
WARP_EXACT_COPIES = {"identity": (0, 0), "int_shift": (2, -1)}
NEAREST_TRANSFORMS = {
    "shift+0.5": shift_tf(0.5, 0), "shift-0.5": shift_tf(-0.5, 0),       # exact halves; -0.5 also reaches w - 0.5 -> w: out
    "shift1.5": shift_tf(1.5, -1.5),
    "neg_zero": shift_tf(0.25, 0.25),                                     # (-0.5, 0) rounds to -0.0 and stays in frame
    "rot0.4": rotation_tf(0.4, *WARP_IN),
    "proj_zero": WARP_TRANSFORMS["proj_zero"],
    "far": WARP_TRANSFORMS["far"],
}
WARP_COMBOS = ("ss", "sb", "bs", "bb")                   # source, transforms: s(hared) or b(atched)


def shift_copy(img, dx, dy):
    """img [..., H, W, C] moved by an integer (dx, dy), zero filled: out[y, x] = img[y - dy, x - dx]"""
    h, w = img.shape[-3], img.shape[-2]
    out = np.zeros_like(img)
    ys, xs = np.arange(h), np.arange(w)
    ys, xs = ys[(ys - dy >= 0) & (ys - dy < h)], xs[(xs - dx >= 0) & (xs - dx < w)]
    if len(ys) and len(xs):
        out[..., ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1, :] = img[..., ys[0] - dy:ys[-1] - dy + 1, xs[0] - dx:xs[-1] - dx + 1, :]
    return out


def _to_index(v):
    """asr_coord_to_int: clamp to +-1e9, then (int)"""
    v = np.where(np.isnan(v), f32(-1e9), np.clip(v, f32(-1e9), f32(1e9)))
    return v.astype(np.int64)


def warp_np(src, tfs, n, out_hw=None, nearest=False, mut=None, taps=False):
    """src [N,H,W,C] or [H,W,C], tfs [N,8] or [8] -> [n,Ho,Wo,C] float32.  mut: a deliberately wrong variant (host test).
    taps=True: also the number of in-frame taps per output pixel (bilinear)."""
    src, tfs = np.asarray(src, np.float32), np.asarray(tfs, np.float32)
    img = src if src.ndim == 4 else np.broadcast_to(src, (n,) + src.shape)
    tf = tfs if tfs.ndim == 2 else np.broadcast_to(tfs, (n, 8))
    if mut == "tf0":
        tf = np.broadcast_to(tf[0], (n, 8))
    _, h, w, c = img.shape
    ho, wo = out_hw or (h, w)
    t = tf.reshape(n, 8, 1, 1)
    xs = np.arange(wo, dtype=np.float32).reshape(1, 1, wo)
    ys = np.arange(ho, dtype=np.float32).reshape(1, ho, 1)
    with np.errstate(all="ignore"):
        nx = t[:, 0] * xs + t[:, 1] * ys + t[:, 2]
        ny = t[:, 3] * xs + t[:, 4] * ys + t[:, 5]
        proj = t[:, 6] * xs + t[:, 7] * ys + f32(1)
        ix, iy = (nx / proj).astype(np.float32), (ny / proj).astype(np.float32)
        ok = np.broadcast_to(proj != 0, ix.shape)
        if mut == "swap_xy":
            ix, iy = iy, ix
        flat = img.reshape(n, h * w, c)

        def read(yi, xi):
            inside = (yi >= 0) & (yi < h) & (xi >= 0) & (xi < w)
            idx = (np.clip(yi, 0, h - 1) * w + np.clip(xi, 0, w - 1)).reshape(n, ho * wo, 1)
            v = np.take_along_axis(flat, idx, axis=1).reshape(n, ho, wo, c)
            if mut == "clamp_edge":
                return v, inside
            return np.where(inside[..., None], v, f32(0)), inside

        if nearest:
            rnd = (lambda v: np.rint(v.astype(np.float64))) if mut == "half_even" else \
                (lambda v: np.sign(v.astype(np.float64)) * np.floor(np.abs(v.astype(np.float64)) + 0.5))
            ry, rx = rnd(iy), rnd(ix)
            inside = ok & (ry >= 0) & (ry < h) & (rx >= 0) & (rx < w)
            v, _ = read(np.where(inside, ry, 0).astype(np.int64), np.where(inside, rx, 0).astype(np.int64))
            return np.where(inside[..., None], v, f32(0)).astype(np.float32)
        fl = np.trunc if mut == "trunc" else np.floor
        xf, yf = fl(ix), fl(iy)
        xc, yc = xf + f32(1), yf + f32(1)
        x0, y0 = _to_index(xf), _to_index(yf)
        (v00, i00), (v01, i01) = read(y0, x0), read(y0, x0 + 1)
        (v10, i10), (v11, i11) = read(y0 + 1, x0), read(y0 + 1, x0 + 1)
        wxl, wxh = (xc - ix)[..., None], (ix - xf)[..., None]
        vyf = wxl * v00 + wxh * v01
        vyc = wxl * v10 + wxh * v11
        out = (yc - iy)[..., None] * vyf + (iy - yf)[..., None] * vyc
        if mut != "proj0":
            out = np.where(ok[..., None], out, f32(0))
    out = out.astype(np.float32)
    if taps:
        return out, (i00.astype(int) + i01 + i10 + i11) * ok
    return out


def warp_image(shape, seed, labels=False):
    rng = np.random.default_rng(seed)
    if labels:
        return rng.choice(np.array([0, 3, 8, 255], np.float32), size=shape).astype(np.float32)
    return rng.random(shape, dtype=np.float32)


def build_warp(case):
    """-> src, tfs, n, out_hw"""
    h, w = case.in_hw
    n = case.n
    src_b, tf_b = case.combo[0] == "b", case.combo[1] == "b"
    src = warp_image(((n,) if src_b else ()) + (h, w, case.c), seed_of(case), labels=case.nearest)
    tf = case.tf
    if tf_b and tf.ndim == 1:        # the case's transform, then two others: a failure of "every image its own transform" shows
        tf = np.stack([case.tf, shift_tf(0, 0), shift_tf(2, -1)][:n] + [case.tf] * max(n - 3, 0))
    return src, tf, n, case.out_hw


def check_warp(case, data, got, ref=None):
    """ref: the oracle's result when the caller has it (the GPU test), else the restatement.  -> largest |got - ref|"""
    src, tf, n, out_hw = data
    mine = warp_np(src, tf, n, out_hw, nearest=case.nearest)
    ref = mine if ref is None else ref
    assert got.shape == ref.shape and got.dtype == np.float32, case.id
    if case.nearest:
        bad = np.argwhere(got != ref)
        assert bad.size == 0, (case.id, len(bad), bad[0].tolist(), float(got[tuple(bad[0])]), float(ref[tuple(bad[0])]))
        return 0.0
    err = np.abs(got - ref)
    bad = np.argwhere(~(err <= WARP_ATOL))
    assert bad.size == 0, (case.id, len(bad), bad[0].tolist(), float(got[tuple(bad[0])]), float(ref[tuple(bad[0])]))
    zero = ref == 0
    assert (got[zero] == 0).all(), (case.id, "pixels the reference makes exactly 0", int((got[zero] != 0).sum()))
    if case.tf_name in WARP_EXACT_COPIES:
        dx, dy = WARP_EXACT_COPIES[case.tf_name]
        img = src if src.ndim == 4 else np.broadcast_to(src, (n,) + src.shape)
        if tuple(out_hw) == tuple(case.in_hw):
            first = slice(0, 1) if case.combo[1] == "b" else slice(None)          # batched transforms: image 0 has this one
            assert same_bits(got[first], shift_copy(img, dx, dy)[first]), (case.id, "not the bit-exact copy")
            if case.combo[1] == "b" and n >= 3:                                   # images 1 and 2: identity and the (2, -1) shift
                assert same_bits(got[1], np.ascontiguousarray(img[1])), (case.id, "image 1: identity")
                assert same_bits(got[2], shift_copy(img, 2, -1)[2]), (case.id, "image 2: integer shift")
    return float(err.max())


def _warp_cases():
    out = []
    for name, tf in WARP_TRANSFORMS.items():
        for c in WARP_CHANNELS:
            for oname, ohw in WARP_OUTS.items():
                for combo in WARP_COMBOS:
                    out.append(Case("warp", f"{name}_c{c}_{oname}_{combo}", tf_name=name, tf=tf, c=c, in_hw=WARP_IN, out_hw=ohw,
                                    combo=combo, n=WARP_BATCH, nearest=False))
    # the grid-stride trip: 5 x 512 x 512 output pixels from one 16 x 16 single-channel source
    tfs = []
    for k in range(5):
        r = rotation_tf(0.2 * k - 0.3, 16, 16)
        r[[0, 1, 3, 4]] *= f32(16 / 512) * f32(1 + 0.1 * k)
        tfs.append(r)
    out.append(Case("warp", "stride_5x512x512", tf_name="stride", tf=np.stack(tfs), c=1, in_hw=(16, 16), out_hw=(512, 512), combo="sb",
                    n=5, nearest=False))
    return out


def _nearest_cases():
    out = []
    for name, tf in NEAREST_TRANSFORMS.items():
        for c in (1, 3):
            for oname in ("same", "11x17"):
                for combo in ("ss", "bb"):
                    out.append(Case("nearest", f"{name}_c{c}_{oname}_{combo}", tf_name=name, tf=tf, c=c, in_hw=WARP_IN,
                                    out_hw=WARP_OUTS[oname], combo=combo, n=WARP_BATCH, nearest=True))
    return out


# ---- augment_copies: translate(rotate(tile(image))) ----------------------------------------------------------------------
AUGMENT_SHAPES = ((3, 5, 300, 3), (2, 3, 257, 1), (2, 2, 256, 3), (1, 1, 1, 1), (4, 40, 24, 3))
# (angle, (dx, dy)); "frame": a shift of w + 3 columns, larger than the frame -> the copy is exactly 0
AUGMENT_POOL = ((0.0, (0, 0)), (0.4, (1.25, -0.75)), (-0.4, (2, -1)), (np.pi / 2, (0, 0)), (np.pi, (0.5, 0.5)), (0.0, (2, -1)),
                (0.0, "frame"), (0.4, (0, 0)))


def build_augment(case):
    """-> image [h,w,c], rot_tf [n,8], trans_tf [n,8], angles, shifts [n,2]"""
    n, h, w, c = case.shape
    image = warp_image((h, w, c), seed_of(case))
    picks = [AUGMENT_POOL[(case.start + i) % len(AUGMENT_POOL)] for i in range(n)]
    angles = np.array([p[0] for p in picks], np.float32)
    shifts = np.array([(w + 3, 0) if p[1] == "frame" else p[1] for p in picks], np.float32)
    rot = np.stack([rotation_tf(a, h, w) for a in angles])
    trans = np.stack([shift_tf(dx, dy) for dx, dy in shifts])
    return image, rot, trans, angles, shifts


def augment_np(image, rot, trans, mut=None):
    n = rot.shape[0]
    out = warp_np(warp_np(image, rot, n, mut=mut), trans, n, mut=mut)
    if mut == "cols256":
        out[:, :, 256:] = f32(0)
    return out


def check_augment(case, data, got, ref=None):
    image, rot, trans, angles, shifts = data
    ref = augment_np(image, rot, trans) if ref is None else ref
    assert got.shape == ref.shape and got.dtype == np.float32, case.id
    err = np.abs(got - ref)
    bad = np.argwhere(~(err <= WARP_ATOL))
    assert bad.size == 0, (case.id, len(bad), bad[0].tolist(), float(got[tuple(bad[0])]), float(ref[tuple(bad[0])]))
    n, h, w, c = case.shape
    for i in range(n):
        dx, dy = float(shifts[i, 0]), float(shifts[i, 1])
        if angles[i] == 0 and dx == int(dx) and dy == int(dy):       # identity and integer shifts: the numpy slice copy, bit for bit
            assert same_bits(got[i], shift_copy(image, int(dx), int(dy))), (case.id, "copy", i, "not the bit-exact copy")
            if abs(dx) >= w or abs(dy) >= h:
                assert not got[i].any(), (case.id, "copy", i, "shifted past the frame but not 0")
            if dx == 0 and dy == 0:                                  # (covers the 12-byte RGB load at the last pixel)
                assert same_bits(got[i][0, 0], image[0, 0]) and same_bits(got[i][h - 1, w - 1], image[h - 1, w - 1]), (case.id, i)
    return float(err.max())


def _augment_cases():
    out = []
    for shape in AUGMENT_SHAPES:
        n = shape[0]
        for start in range(0, len(AUGMENT_POOL), n):
            out.append(Case("augment", "x".join(map(str, shape)) + f"_from{start}", shape=shape, start=start))
    return out


AUGMENT_REFUSALS = {"c2": (2, 3, 5, 2), "c4": (2, 3, 5, 4), "n65536": (65536, 1, 1, 1)}


# ---------------------------------------------------------------------------------------------------------------------------
CASES = {}
for _c in (_minmax_cases() + _normalize_cases() + _opm_slice_cases() + _logit_cases("argmax") + _logit_cases("opm_argmax") +
           _logit_cases("slice_max", min_classes=2) + _logit_cases("activation") + _threshold_cases() + _iou_cases() +
           _iou_classes_cases() + _class_counts_cases() + _warp_cases() + _nearest_cases() + _augment_cases()):
    CASES.setdefault(_c.entry, []).append(_c)


def ids(entry):
    return [c.id for c in CASES[entry]]


def case_by_id(entry, id):
    for c in CASES[entry]:
        if c.id == id:
            return c
    raise KeyError((entry, id))
