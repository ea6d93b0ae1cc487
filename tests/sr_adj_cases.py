"""The transform families and the case table of tests/test_gpu_sr_adj_forms.py: affine rotations that are no pure rotations, so
that the exact-adjoint gather (csrc/sr_adj_kernels.h; include/asr_hip.h, "exact adjoint") leaves its 3 x 3 form -- the counted
loop, its clamps at the plane border, the decision at 1.46875, the fallbacks at half-width 8 and at |translation| 16384 -- and
`instantiations`, the exact dispatch of csrc/sr.hip (sr_solve_impl under ASR_ADJ_EXACT, asr_sr_backward_adj_f32,
sr_data_bound_impl) restated in plain Python, in the style of tests/sr_option_cases.py.  HOST ONLY -- nothing here touches a
device; tests/test_sr_adj_cases_host.py holds the families against the oracle and tests/test_sr_option_cases_host.py holds the
table against the source text.  TEST INFRASTRUCTURE ONLY.

A case is (shape, family, rule, wtv, monitor, chunk, n):
  shape      (H, W, h, w), one of SHAPES
  family     a key of FAMILIES (below)
  rule       "grad": asr_sr_backward_adj_f32 for the gradient alone; "step": the same entry point with an AMSGrad update;
             a solve under "adam" (AMSGrad), "sgd" or "pd" (primal-dual); "bound": asr_sr_data_bound_adj_f32
  wtv        edge-weighted TV on (True) or off
  monitor    "off", "trace" (patience 0: never stops) or "stop"
  chunk      plane_chunk (0: all copies at once)
  n          copies per image"""
import functools
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

from oracle import tf_ops
from sr_adj_ref import MAX_HALF, MAX_SHIFT, _half
from sr_option_cases import ADJ_GATHER_KERNELS, ADJ_KERNELS, _b, log2f             # noqa: F401 (re-exported)

F = np.float32
FIXED_HALF = F(1.46875)             # kAdjFixedHalf: up to it the 3 x 3 form, above it the counted loop
QUARTER = F(np.pi / 4)              # the angle of the widest window: |cos| + |sin| = sqrt(2)

Case = namedtuple("Case", "shape family rule wtv monitor chunk n")

SHAPES = [(12, 20, 3, 5),           # factor 4
          (12, 18, 2, 3),           # factor 6: the generic-factor grad-translate feeds the exact gather
          (8, 8, 4, 4),             # factor 2
          (16, 24, 2, 3),           # factor 8
          (8, 72, 2, 18)]           # factor 4; two gather blocks in x, the second one ragged (8 of 64 columns)
COPIES = (1, 5, 6, 9)
CHUNKS = (0, 3, 1)
RULES = ("grad", "step", "adam", "sgd", "pd", "bound")
MONITORS = ("off", "trace", "stop")

# family -> (scale k handed as sx = sy, a pair (sx, sy), or None for per-copy values; what the image's LARGEST half-width must be; exact?)
#   "fixed": <= 1.46875, the 3 x 3 form; "loop": in (1.46875, 8], the counted loop; "wide": > 8, the registered statements
FAMILIES = {
    "rotations":   (1.0, "fixed", True),       # the regime of tests/test_gpu_sr_adj.py, kept as the anchor: halves <= 1.4299
    "just_fixed":  (0.9733, "fixed", True),    # sqrt(2) / k + 1/64 = 1.468634
    "just_loop":   (0.9731, "loop", True),     # 1.468933
    "zoom2":       (0.5, "loop", True),        # halves 2.0 .. 2.85
    "zoom5":       (0.2, "loop", True),        # halves 5.0 .. 7.09: R^-1 p far outside the plane at the border, all four clamps act
    "shrink":      (1.5, "fixed", True),       # halves below 1: 3 x 3 with windows smaller than 3
    "aniso_shear": (None, "loop", True),       # sx, sy in [0.2, 1.2], shear in [-0.3, 0.3]: ex != ey
    "wide_x":      ((0.4, 1.2), "loop", True),  # every ex in 2.5 .. 3.56, every ey <= 1.195: the decision has to read ex ...
    "wide_y":      ((1.2, 0.4), "loop", True),  # ... and ey
    "near_wide":   (0.18, "loop", True),       # 7.872: the widest window the loop serves, 17 positions a side
    "too_wide":    (0.1768, "wide", False),    # 8.0146
    "far_shift":   (1.0, "fixed", False),      # one copy whose inverse has |i02| > 16384
}
LOOP_FAMILIES = tuple(f for f, (_, side, exact) in FAMILIES.items() if side == "loop" and exact)
# the scales and shears of "aniso_shear", copy by copy (rolled by the image index): narrow on one axis and wide on the other
_ANISO_SX = (0.2, 1.2, 0.6, 1.0, 0.35, 0.9, 0.25, 1.1, 0.5)
_ANISO_SY = (1.2, 0.2, 1.0, 0.45, 0.9, 0.3, 1.1, 0.25, 0.7)
_ANISO_SHEAR = (0.3, -0.3, 0.15, -0.2, 0.0, 0.25, -0.1, 0.05, -0.3)
FAR = F(20000.0)


def affine_rotations(angles, sx, sy, shear, HW):
    """rot_tf [n, 8] float32: the linear map R(angle) @ [[sx, shear], [0, sy]] about the image centre, every operation float32
    and the offsets as tf_ops.angles_to_projective_transforms takes them, so that sx = sy = 1, shear = 0 is that function bit
    for bit.  The inverse is tf_ops.invert_transforms of the result, the rounded inverse the 1/64 margin exists for."""
    a = np.asarray(angles, dtype=np.float32).reshape(-1)
    sx, sy, shear = (np.broadcast_to(np.asarray(v, dtype=np.float32), a.shape) for v in (sx, sy, shear))
    h, w, one, two = F(HW[0]), F(HW[1]), F(1.0), F(2.0)
    cos, sin = np.cos(a).astype(np.float32), np.sin(a).astype(np.float32)
    l00, l01 = cos * sx, cos * shear + (-sin) * sy
    l10, l11 = sin * sx, sin * shear + cos * sy
    x_off = ((w - one) - (l00 * (w - one) + l01 * (h - one))) / two
    y_off = ((h - one) - (l10 * (w - one) + l11 * (h - one))) / two
    z = np.zeros_like(a)
    out = np.stack([l00, l01, x_off, l10, l11, y_off, z, z], axis=1)
    assert out.dtype == np.float32
    return out


def family_transforms(family, n, HW, rng, image=0):
    """(rot, trans, inv_rot, inv_trans) [n, 8] of one image: angles with 0, pi / 2 and pi / 4 among them (rolled by the image
    index; copy 0 is the pi / 4 one where the family is about the widest window), pure translations up to +-0.4 W in x and +-0.4 H in y,
    the last one an integer."""
    k, _, _ = FAMILIES[family]
    H, W = HW
    angles = rng.uniform(-1.6, 1.6, n).astype(np.float32)
    shifts = (rng.uniform(-0.4, 0.4, (n, 2)) * [W, H]).astype(np.float32)                   # dy by H: a wide plane keeps its copies in frame
    shifts[n - 1] = np.round(shifts[n - 1])
    m = min(n, 3)
    angles[:m] = np.roll(np.array([0.0, np.pi / 2, np.pi / 4], np.float32), image)[:m]
    if family in ("just_fixed", "just_loop", "near_wide", "too_wide"):
        angles[0] = QUARTER
    if k is None:
        sx, sy, shear = (np.roll(np.array(v, np.float32), image)[:n] for v in (_ANISO_SX, _ANISO_SY, _ANISO_SHEAR))
    else:
        kx, ky = k if isinstance(k, tuple) else (k, k)
        sx, sy = np.full(n, kx, np.float32), np.full(n, ky, np.float32)
        shear = np.zeros(n, np.float32)
    rot = affine_rotations(angles, sx, sy, shear, HW)
    if family == "far_shift":
        far = min(1, n - 1)
        rot[far] = affine_rotations([0.3], 1.0, 1.0, 0.0, HW)[0]
        rot[far, 2] += FAR
    tr = tf_ops.translations_to_projective_transforms(shifts)
    return rot, tr, tf_ops.invert_transforms(rot), tf_ops.invert_transforms(tr)


def halves(inv_rot_tf):
    """[n, 2] float32: the window half-widths (ex, ey) of every copy, as the kernels and the restatement compute them."""
    inv = np.asarray(inv_rot_tf, np.float32).reshape(-1, 8)
    return np.array([[_half(i[0], i[1]), _half(i[3], i[4])] for i in inv], np.float32)


def side(inv_rot_tf):
    """"fixed", "loop" or "wide": where the image's largest half-width lies."""
    top = halves(inv_rot_tf).max()
    return "fixed" if top <= FIXED_HALF else ("loop" if top <= MAX_HALF else "wide")


def batch_of(shape, n):
    """2 to 4 images, by the case."""
    return 2 + (shape[0] + n) % 3


@functools.lru_cache(maxsize=None)
def problem(shape, family, n, b=None):
    """Host arrays of a case: computed once, shared by the tests, never changed.  One transform set per image."""
    H, W, h, w = shape
    b = batch_of(shape, n) if b is None else b
    rng = np.random.default_rng(1000 * H + 10 * W + n + 100000 * sorted(FAMILIES).index(family))
    tfs = [family_transforms(family, n, (H, W), rng, i) for i in range(b)]
    resid = rng.standard_normal((b, n, h, w)).astype(np.float32)
    x = rng.random((b, H, W), dtype=np.float32)
    y = rng.random((b, n, h, w), dtype=np.float32)
    return SimpleNamespace(H=H, W=W, h=h, w=w, n=n, b=b, tfs=tfs, resid=resid, x=x, y=y, family=family, shape=shape)


def edge_weights(shape, b, seed=9):
    """(wy, wx) float32 [b, H, W]: values in [0, 1] with a tenth exact zeros and a tenth exact ones, as
    sr_option_cases.edge_weights builds them."""
    rng = np.random.default_rng(seed)
    planes = []
    for _ in range(2):
        plane = rng.random((b, shape[0], shape[1]), dtype=np.float32)
        plane[rng.random(plane.shape) < 0.1] = 0.0
        plane[rng.random(plane.shape) < 0.1] = 1.0
        planes.append(plane)
    return tuple(planes)


def perturbed_inverses(inv_rot_tf):
    """The inverse with its two translations moved by (+1/256, -1/256), (-1/256, +1/256) and (+1/128, +1/128): other windows,
    well inside the 1/64 margin, so no value of the exact gradient may change."""
    out = []
    for dx, dy in ((1 / 256, -1 / 256), (-1 / 256, 1 / 256), (1 / 128, 1 / 128)):
        t = np.array(inv_rot_tf, np.float32)
        t[:, 2] += F(dx)
        t[:, 5] += F(dy)
        out.append(t)
    return out


def with_zero_copy(p, image, family="zoom2"):
    """(tfs, resid [n + 1, h, w]) of image `image` of problem p with one more copy appended: a copy of `family` whose residual
    is all zero.  It adds nothing to any gradient and, under "zoom2", moves the whole image to the counted loop."""
    extra = family_transforms(family, 1, (p.H, p.W), np.random.default_rng(77), 1)           # image 1: the pi / 4 copy
    tfs = tuple(np.concatenate([t, e]).astype(np.float32) for t, e in zip(p.tfs[image], extra))
    resid = np.concatenate([p.resid[image], np.zeros((1, p.h, p.w), np.float32)])
    return tfs, resid


# ---- the dispatch ------------------------------------------------------------------------------------------------------------------
def factor(shape):
    H, W, h, w = shape
    assert H % h == 0 and W % w == 0 and H // h == W // w
    return H // h


def instantiations(case, want_loss=False):
    """The set of kernel names (template arguments as the reader of sr_option_cases.source_instantiations writes them) that
    the case launches under adjoint = "exact".  An image the exact form does not apply to runs the same kernels: its mode
    word sends it to the registered statements inside them."""
    case = Case(*case)
    assert case.shape in SHAPES and case.family in FAMILIES and case.rule in RULES and case.monitor in MONITORS
    assert case.chunk >= 0 and case.n >= 1 and isinstance(case.wtv, bool)
    L = log2f(factor(case.shape))
    mon = case.monitor != "off"
    if case.rule in ("grad", "step"):                          # asr_sr_backward_adj_f32: no forward, no monitor
        assert not mon
        return {"sr_adjoint_flags_kernel", f"sr_grad_translate_kernel<{L}>", f"sr_backward_gather_adj_kernel<{_b(case.wtv)},false>"}
    if case.rule == "bound":                                   # sr_data_bound_impl: L2, no prior, no monitor
        assert not case.wtv and not mon
        return {"sr_adjoint_flags_kernel", "sr_bound_next_v_kernel", "sr_forward_residual_kernel<true,true>",
                f"sr_grad_translate_kernel<{L}>", "sr_backward_gather_adj_kernel<false,false>", "sr_bound_maxima_kernel",
                "sr_bound_out_kernel"}
    # sr_solve_impl; asr_sr_solve_adj_f32 always carries a data term
    gather = "sr_backward_gather_pd_adj_kernel" if case.rule == "pd" else "sr_backward_gather_adj_kernel"
    out = {"sr_adjoint_flags_kernel", f"{gather}<{_b(case.wtv)},{_b(mon)}>"}
    if mon:
        return out | {"sr_mon_init_kernel", "sr_forward_residual_kernel<true,true,true>", "sr_mon_loss_df_kernel",
                      f"sr_mon_loss_prior_kernel<{_b(case.wtv)}>", "sr_mon_decide_kernel", f"sr_grad_translate_kernel<{L},true>"}
    out |= {"sr_forward_residual_kernel<true,true>", f"sr_grad_translate_kernel<{L}>"}
    if want_loss:
        out |= {"sr_loss_df_dt_kernel", f"sr_loss_prior_kernel<{_b(case.wtv)}>"}
    return out


# ---- the table ---------------------------------------------------------------------------------------------------------------------
# 1: the gradient alone, every family on every shape with every copy count and every chunking
GRAD_CASES = [Case(s, f, "grad", False, "off", chunk, n) for s in SHAPES for f in FAMILIES for n in COPIES for chunk in CHUNKS]
# 6: the instantiations no suite launched before, (12, 20, 3, 5) with n = 5, each on the 3 x 3 form and on the counted loop
FORM_SHAPE, FORM_N, FORM_FAMILIES = SHAPES[0], 5, ("rotations", "zoom2")
STEP_CASES = [Case(FORM_SHAPE, f, "step", True, "off", 0, FORM_N) for f in FORM_FAMILIES]
SOLVE_CASES = [Case(FORM_SHAPE, f, "adam", True, "off", 0, FORM_N) for f in FORM_FAMILIES]
PD_CASES = [Case(FORM_SHAPE, f, "pd", wtv, "off", chunk, FORM_N) for f in FORM_FAMILIES for wtv in (False, True) for chunk in (0, 3)]
MONITORED = [Case(FORM_SHAPE, f, rule, wtv, mon, 0, FORM_N) for f in FORM_FAMILIES for rule in ("adam", "pd") for wtv in (False, True)
             for mon in ("trace", "stop")]
MONITORED += [Case(FORM_SHAPE, f, "sgd", False, "trace", 0, FORM_N) for f in FORM_FAMILIES]
BOUND_CASES = [Case(FORM_SHAPE, f, "bound", False, "off", chunk, FORM_N) for f in FORM_FAMILIES for chunk in (0, 3)]
TABLE = GRAD_CASES + STEP_CASES + SOLVE_CASES + PD_CASES + MONITORED + BOUND_CASES
