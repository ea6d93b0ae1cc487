"""The guided filter (asr_guided_prepare_f32 / asr_guided_apply_f32, ops.guided_*) against a numpy restatement of the rule in
include/asr_hip.h: clipped windows summed directly (shifted adds, never a cumulative sum) and np.linalg.inv per pixel.  The
restatement is never the library.

Error scale.  (S + eps U)^-1 amplifies cancellation by up to 1/eps, so a reasonable f32 error cannot be derived; it is taken
from the restatement itself: e32 = max |restate(float32) - restate(float64)| on the same inputs, and the library must stay
within max(8 * e32, 2^-18 * max|p|) of the float64 result.  The 8 allows another summation order and another 3x3 solve; it is
not a measurement of the kernel.  Every accuracy check prints its e_gpu / e32."""
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -18


# ---- the restatement -----------------------------------------------------------------------------------------------------
def box_sum(a, r):
    """Clipped (2r+1)^2 window sums over the last two axes by direct shifted adds, in a's dtype."""
    H, W = a.shape[-2:]
    pad = np.zeros(a.shape[:-2] + (H + 2 * r, W + 2 * r), dtype=a.dtype)
    pad[..., r:r + H, r:r + W] = a
    v = np.zeros(a.shape[:-2] + (H, W + 2 * r), dtype=a.dtype)
    for d in range(2 * r + 1):
        v += pad[..., d:d + H, :]
    out = np.zeros(a.shape, dtype=a.dtype)
    for d in range(2 * r + 1):
        out += v[..., :, d:d + W]
    return out


def window_count(H, W, r, dtype):
    ny = np.minimum(np.arange(H) + r, H - 1) - np.maximum(np.arange(H) - r, 0) + 1
    nx = np.minimum(np.arange(W) + r, W - 1) - np.maximum(np.arange(W) - r, 0) + 1
    return (ny[:, None] * nx[None, :]).astype(dtype)


def restate(guide, p, r, eps, dtype):
    """guide [H, W, 3], p [P, H, W] -> q [P, H, W], every step in `dtype`."""
    I = np.ascontiguousarray(guide.astype(dtype).transpose(2, 0, 1))            # [3, H, W]
    p = p.astype(dtype)
    H, W = p.shape[-2:]
    N = window_count(H, W, r, dtype)
    eps = dtype(eps)
    mu = box_sum(I, r) / N
    M = np.empty((H, W, 3, 3), dtype=dtype)
    for a in range(3):
        for b in range(3):
            M[..., a, b] = box_sum(I[a] * I[b], r) / N - mu[a] * mu[b] + (eps if a == b else dtype(0))
    Minv = np.linalg.inv(M)
    assert Minv.dtype == dtype
    m = box_sum(p, r) / N                                                          # [P, H, W]
    c = box_sum(I[None] * p[:, None], r) / N - mu[None] * m[:, None]               # [P, 3, H, W]
    a = np.einsum("hwij,pjhw->pihw", Minv, c).astype(dtype)
    b = m - (a * mu[None]).sum(axis=1, dtype=dtype)
    q = (box_sum(a, r) / N * I[None]).sum(axis=1, dtype=dtype) + box_sum(b, r) / N
    assert q.dtype == dtype
    return q


def double_mean(p, r):
    """The window mean of the window mean of p, float64."""
    N = window_count(p.shape[-2], p.shape[-1], r, np.float64)
    return box_sum(box_sum(p.astype(np.float64), r) / N, r) / N


# ---- inputs --------------------------------------------------------------------------------------------------------------
def make_guide(kind, H, W, rng):
    if kind == "uniform":
        return rng.uniform(0.0, 1.0, (H, W, 3)).astype(np.float32)
    # piecewise constant: four colours on a slanted 2 x 2 layout
    Y, X = np.mgrid[0:H, 0:W]
    region = (Y + X // 3 >= H // 2).astype(int) * 2 + (X - Y // 4 >= W // 2).astype(int)
    colours = np.array([[0.8, 0.3, 0.2], [0.2, 0.5, 0.7], [0.1, 0.9, 0.4], [0.6, 0.6, 0.05]], dtype=np.float32)
    return colours[region]


def make_planes(P, H, W, rng):
    """Signed normal planes and {0, 1} masks, alternating."""
    p = np.empty((P, H, W), dtype=np.float32)
    for k in range(P):
        p[k] = rng.normal(0.0, 1.0, (H, W)) if k % 2 == 0 else (rng.uniform(0, 1, (H, W)) < 0.4)
    return p


SHAPES_RADII = ([(s, r) for s in ((40, 72), (37, 70)) for r in (0, 1, 3, 7)] +
                [((3, 65), 4), ((65, 3), 4), ((1, 1), 2), ((96, 130), 32)])
_CACHE = {}


def case(shape, r, eps, kind, P=20):
    """Inputs and both restatements of one case, computed once and shared (never modified)."""
    key = (shape, r, eps, kind, P)
    if key not in _CACHE:
        rng = np.random.default_rng(zlib.crc32(repr((shape, r, kind, P)).encode()))
        H, W = shape
        guide, p = make_guide(kind, H, W, rng), make_planes(P, H, W, rng)
        q64 = restate(guide, p, r, eps, np.float64)
        e32 = float(np.abs(restate(guide, p, r, eps, np.float32).astype(np.float64) - q64).max())
        for a in (guide, p, q64):
            a.setflags(write=False)
        _CACHE[key] = (guide, p, q64, e32)
    return _CACHE[key]


def bound(e32, p):
    return max(8.0 * e32, FLOOR * float(np.abs(p).max()))


def run(dev, guide, p, r, eps):
    from asr_amd import ops
    q = ops.guided_filter(torch.tensor(guide).to(dev), torch.tensor(p).to(dev), r, eps)
    return q.cpu().numpy()


def report(name, e_gpu, e32, lim):
    print(f"guided {name}: e_gpu {e_gpu:.3e}  e32 {e32:.3e}  e_gpu/e32 {e_gpu / e32 if e32 else float('inf'):.3f}  bound {lim:.3e}")


# ---- accuracy ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["uniform", "piecewise"])
@pytest.mark.parametrize("eps", [1e-2, 1e-3])
@pytest.mark.parametrize("shape,r", SHAPES_RADII)
def test_matches_the_float64_restatement(dev, shape, r, eps, kind):
    guide, p, q64, e32 = case(shape, r, eps, kind)
    q = run(dev, guide, p, r, eps)
    assert q.shape == p.shape and q.dtype == np.float32 and np.isfinite(q).all()
    e_gpu, lim = float(np.abs(q - q64).max()), bound(e32, p)
    report(f"{shape[0]}x{shape[1]} r={r} eps={eps:g} {kind} P=20", e_gpu, e32, lim)
    assert e_gpu <= lim


@pytest.mark.parametrize("P", [1, 3])
def test_small_plane_counts_match_too(dev, P):
    guide, p, q64, e32 = case((37, 70), 3, 1e-3, "uniform", P)
    q = run(dev, guide, p, 3, 1e-3)
    e_gpu, lim = float(np.abs(q - q64).max()), bound(e32, p)
    report(f"37x70 r=3 eps=0.001 uniform P={P}", e_gpu, e32, lim)
    assert e_gpu <= lim


def test_tiny_eps_stays_finite_and_within_its_own_scale(dev):
    guide, p, q64, e32 = case((40, 72), 3, 1e-6, "piecewise")
    q = run(dev, guide, p, 3, 1e-6)
    assert np.isfinite(q).all()
    e_gpu = float(np.abs(q - q64).max())
    report("40x72 r=3 eps=1e-06 piecewise P=20", e_gpu, e32, 8.0 * e32)
    assert e_gpu <= 8.0 * e32


# ---- properties ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,r", [((37, 70), 3), ((96, 130), 32)])
def test_planes_are_independent_repeatable_and_may_alias(dev, shape, r):
    from asr_amd import ops
    guide, p, _, _ = case(shape, r, 1e-3, "uniform")
    g, p3 = torch.tensor(guide).to(dev), torch.tensor(p[:3]).to(dev)
    q3 = ops.guided_filter(g, p3, r, 1e-3)
    for k in range(3):                                    # each plane of a 3-plane call is bitwise the 1-plane call
        q1 = ops.guided_filter(g, p3[k:k + 1].contiguous(), r, 1e-3)
        assert torch.equal(q3[k:k + 1], q1)
        assert torch.equal(ops.guided_filter(g, p3[k].contiguous(), r, 1e-3), q1[0])        # and the [H, W] form
    assert torch.equal(ops.guided_filter(g, p3, r, 1e-3), q3)                  # two identical calls, the same bits
    state = ops.guided_prepare(g, r, 1e-3)                                     # guided_filter == prepare + apply
    assert (state.H, state.W, state.radius) == (shape[0], shape[1], r)
    assert torch.equal(ops.guided_apply(state, g, p3), q3)
    assert torch.equal(ops.guided_apply(state, g, p3), q3)                     # the state is only read
    alias = p3.clone()
    assert ops.guided_apply(state, g, alias, out=alias) is alias               # q aliased to p
    assert torch.equal(alias, q3)


def test_radius_zero_returns_p(dev):
    for eps in (1e-2, 1e-3):
        guide, p, q64, e32 = case((37, 70), 0, eps, "uniform")
        q = run(dev, guide, p, 0, eps)
        assert np.abs(q64 - p).max() <= 1e-12                                 # the rule itself: S = 0, a = 0, b = p
        assert np.abs(q - p).max() <= bound(e32, p)


@pytest.mark.parametrize("kind", ["uniform", "piecewise"])
def test_constant_p_comes_back(dev, kind):
    guide, _, _, _ = case((40, 72), 7, 1e-3, kind)
    p = np.full((1, 40, 72), -2.75, dtype=np.float32)
    q64 = restate(guide, p, 7, 1e-3, np.float64)
    e32 = float(np.abs(restate(guide, p, 7, 1e-3, np.float32) - q64).max())
    assert np.abs(q64 - p).max() <= 1e-9
    q = run(dev, guide, p, 7, 1e-3)
    report(f"40x72 r=7 constant p {kind}", float(np.abs(q - q64).max()), e32, bound(e32, p))
    assert np.abs(q - p).max() <= bound(e32, p)


@pytest.mark.parametrize("shape,r", [((40, 72), 3), ((3, 65), 4), ((96, 130), 32)])
def test_constant_guide_and_huge_eps_give_the_double_window_mean(dev, shape, r):
    _, p, _, _ = case(shape, r, 1e-3, "uniform")
    dm = double_mean(p, r)
    flat = np.broadcast_to(np.array([0.5, 0.25, 0.125], dtype=np.float32), shape + (3,)).copy()      # powers of two: exact scaling
    q64 = restate(flat, p, r, 1e-3, np.float64)
    assert np.abs(q64 - dm).max() == 0.0                                      # the float64 restatement agrees exactly
    e32 = float(np.abs(restate(flat, p, r, 1e-3, np.float32) - q64).max())
    q = run(dev, flat, p, r, 1e-3)
    report(f"{shape[0]}x{shape[1]} r={r} constant guide", float(np.abs(q - dm).max()), e32, bound(e32, p))
    assert np.abs(q - dm).max() <= bound(e32, p)
    guide = case(shape, r, 1e-3, "uniform")[0]                                 # eps = 1e6: a vanishes, b = m
    q64 = restate(guide, p, r, 1e6, np.float64)
    e32 = float(np.abs(restate(guide, p, r, 1e6, np.float32) - q64).max())
    q = run(dev, guide, p, r, 1e6)
    report(f"{shape[0]}x{shape[1]} r={r} eps=1e6", float(np.abs(q - dm).max()), e32, bound(e32, p))
    assert np.abs(q64 - dm).max() <= 1e-5 * np.abs(p).max()                    # |a| <= |c| / eps ~ 1e-6
    assert np.abs(q - q64).max() <= bound(e32, p)


# ---- what it is for ------------------------------------------------------------------------------------------------------
def synthetic_object():
    """A 64 x 64 two-colour image of an ellipse plus a bar, and the score a 4x-downsampled network would give for it."""
    H = W = 64
    Y, X = np.mgrid[0:H, 0:W]
    mask = (((Y - 30) ** 2 / 18.0 ** 2 + (X - 34) ** 2 / 12.0 ** 2) < 1) | ((np.abs(Y - 44) < 6) & (np.abs(X - 20) < 15))
    guide = np.where(mask[..., None], np.array([0.8, 0.3, 0.2]), np.array([0.2, 0.5, 0.7]))
    guide = np.clip(guide + np.random.default_rng(1234).normal(0, 0.03, guide.shape), 0.0, 1.0).astype(np.float32)
    low = mask.astype(np.float64).reshape(16, 4, 16, 4).mean(axis=(1, 3))     # 4 x 4 block mean

    def axis(n_out, n_in):                                                    # half-pixel bilinear taps
        src = np.clip((np.arange(n_out) + 0.5) * n_in / n_out - 0.5, 0, n_in - 1)
        lo = np.floor(src).astype(int)
        hi = np.minimum(lo + 1, n_in - 1)
        return lo, hi, src - lo

    ylo, yhi, fy = axis(H, 16)
    xlo, xhi, fx = axis(W, 16)
    rows = low[ylo] * (1 - fy)[:, None] + low[yhi] * fy[:, None]
    p = rows[:, xlo] * (1 - fx)[None] + rows[:, xhi] * fx[None]
    # within 2 px of the object's boundary: a pixel with a pixel of the other kind at Euclidean distance <= 2
    near = np.zeros_like(mask)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            if dy * dy + dx * dx <= 4:
                sh = np.roll(np.roll(np.pad(mask, 2, mode="edge"), dy, 0), dx, 1)[2:-2, 2:-2]
                near |= sh != mask
    return mask, guide, np.ascontiguousarray(p, dtype=np.float32), near


def iou(a, b, where=None):
    if where is not None:
        a, b = a & where, b & where
    return (a & b).sum() / max((a | b).sum(), 1)


def test_it_moves_an_upsampled_boundary_onto_the_image_edge(dev):
    mask, guide, p, near = synthetic_object()
    q64 = restate(guide, p[None], 4, 1e-3, np.float64)[0]
    q = run(dev, guide, p[None], 4, 1e-3)[0]
    before, after, ref = iou(p > 0.5, mask), iou(q > 0.5, mask), iou(q64 > 0.5, mask)
    b_before, b_after = iou(p > 0.5, mask, near), iou(q > 0.5, mask, near)
    print(f"guided synthetic object: IoU {before:.4f} -> {after:.4f} (float64 {ref:.4f}); within 2 px {b_before:.4f} -> {b_after:.4f}")
    assert ref == 1.0
    assert before <= 0.97 and after >= 0.99
    assert b_before <= 0.93 and b_after >= 0.99
