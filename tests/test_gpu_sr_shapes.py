"""GPU parity of the SR solver kernels (csrc/sr.hip: sr_init, K_fwd, the fused backward, K_gt + gather, the affine-flag
kernel, realign) away from the square, tile-aligned, small-rotation corner the other suites live in: rectangular and
ragged shapes, the generic-factor instantiation (f = 6), wide rotations and shifts, out-of-frame copies, and the general
(affine-but-not-pure and projective) branches of both warp stages -- all against the transform-level CPU oracle
(oracle/sr.py *_tf), which is handed the SAME forward and inverse transform arrays as the kernels.

Tolerances are the ones tests/test_gpu_warp_sr.py and tests/test_gpu_sr_options.py already use for these quantities; the
largest deviation of every comparison is printed before it is asserted (pytest -s shows them)."""
import functools

import numpy as np
import pytest
import torch

from oracle import sr as o_sr
from oracle import tf_ops
from test_gpu_warp_sr import _blob_masks

pytestmark = pytest.mark.gpu

# (H, W) <- (h, w); the edge each one is there for
SHAPES = {
    "A": ((40, 72), (10, 18)),    # f 4: 2nd 64-column block has 8 live lanes, 3rd K_gt wave 8 rows, LR map < one 32 x 8 tile in x
    "B": ((22, 34), (11, 17)),    # f 2: odd LR sizes, W just over one 32-pixel backward tile
    "C": ((24, 80), (3, 10)),     # f 8: wide, h below a tile's row count
    "D": ((36, 60), (6, 10)),     # f 6: the generic-factor instantiation (integer / and %)
    "E": ((136, 24), (34, 6)),    # f 4: tall -- three K_gt block rows, W narrower than any tile
}
LAM = (1.0, 0.3, 0.7, 0.05)
ATOL_X0, ATOL_RESID, ATOL_GRAD, RTOL_TERMS, ATOL_REALIGN = 1e-6, 2e-6, 2e-5, 2e-5, 2e-6
OUT_OF_FRAME = 3                  # the copy shifted by (1.5 W, -1.5 H) in every set with n > 3


def _report(what, value):
    print(f"[sr_shapes] {what}: {value:.3e}")
    return value


def _proj_range(tf8, H, W):
    """min / max of c0 * x + c1 * y + 1 over the frame (linear: the extremes are at the corners)."""
    c = np.asarray(tf8, np.float64).reshape(-1, 8)
    corners = np.array([[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1]], np.float64)
    p = c[:, 6:7] * corners[:, 0] + c[:, 7:8] * corners[:, 1] + 1.0
    return float(p.min()), float(p.max())


def _transform_set(kind, seed, n, H, W):
    """[n,8] rot_tf, trans_tf (float32).  Copy 0 is the identity.
    T0: angles U(-0.6, 0.6), shifts U(-0.3, 0.3) x (W, H); copy 1 an exact integer shift (weights exactly 1 / 0), copy 3
        shifted by (1.5 W, -1.5 H) -- wholly out of frame --, copy 4 turned by pi / 2.
    T1: T0 with projective terms in the rotation of the odd copies.
    T2: T0 with, in turn over the copies other than 0 and 3, an affine-but-not-pure translate stage (a0 = 1.05, a1 = 0.03),
        projective terms in the translate stage, projective terms in the rotation (T1's change, on a disjoint set of copies)."""
    rng = np.random.default_rng(seed)
    ang = rng.uniform(-0.6, 0.6, n)
    sh = rng.uniform(-0.3, 0.3, (n, 2)) * [W, H]
    ang[0] = 0.0
    sh[0] = 0.0
    if n > 1:
        sh[1] = np.round(sh[1]) + [1.0, -2.0]
    if n > OUT_OF_FRAME:
        sh[OUT_OF_FRAME] = [1.5 * W, -1.5 * H]
    if n > 4:
        ang[4] = np.pi / 2
    rot = tf_ops.angles_to_projective_transforms(ang.astype(np.float32), H, W)
    tr = tf_ops.translations_to_projective_transforms(sh.astype(np.float32))
    proj = lambda: (rng.uniform(0.4e-3, 1.5e-3, 2) * rng.choice([-1.0, 1.0], 2)).astype(np.float32)
    if kind == "T1":
        for i in range(1, n, 2):
            rot[i, 6:] = proj()
    elif kind == "T2":
        for k, i in enumerate(i for i in range(1, n) if i != OUT_OF_FRAME):
            if k % 3 == 0:
                tr[i, 0], tr[i, 1] = 1.05, 0.03
            elif k % 3 == 1:
                tr[i, 6:] = proj()
            else:
                rot[i, 6:] = proj()
    else:
        assert kind == "T0"
    for t in (rot, tr):           # nothing divides near zero
        lo, hi = _proj_range(t, H, W)
        assert 0.5 <= lo and hi <= 1.5, (kind, lo, hi)
    return rot, tr


class _Problem:
    """Batch of SR problems on one shape with one transform set per image: host arrays, the oracle's results (computed once,
    never modified) and the device copies the kernels get."""

    def __init__(self, shape, kind, n, seed, batch=2):
        (H, W), (h, w) = SHAPES[shape] if isinstance(shape, str) else shape
        self.H, self.W, self.h, self.w, self.n, self.b = H, W, h, w, n, batch
        rng = np.random.default_rng(seed)
        self.y = np.stack([_blob_masks(rng, n, h, w) for _ in range(batch)])
        self.y = (self.y + rng.uniform(0.05, 0.1) * rng.random(self.y.shape, dtype=np.float32)).astype(np.float32)
        tfs = [_transform_set(kind, seed * 100 + i, n, H, W) for i in range(batch)]
        self.rot = np.stack([t[0] for t in tfs])
        self.tr = np.stack([t[1] for t in tfs])
        # the inverses: computed once, the same arrays go to the kernels and to the oracle
        self.irot = np.stack([tf_ops.invert_transforms(t) for t in self.rot])
        self.itr = np.stack([tf_ops.invert_transforms(t) for t in self.tr])
        for t in (self.irot, self.itr):
            lo, hi = _proj_range(t, H, W)
            assert 0.25 <= lo and hi <= 4.0, (kind, lo, hi)     # inverses of the above: still far from a zero denominator
        self.x0_ref = np.stack([tf_ops.resize_bilinear(torch.from_numpy(self.y[i, 0:1, :, :, None]), (H, W)).numpy()[0, :, :, 0]
                                for i in range(batch)])
        self.x = (self.x0_ref + 0.05 * rng.standard_normal((batch, H, W))).astype(np.float32)

    def oracle(self, lam=LAM, use_btv=False):
        return o_sr.Superresolution(*lam, num_aug=self.n, feature_size=(self.h, self.w), output_size=(self.H, self.W),
                                    use_BTV=use_btv)

    def target(self, i):
        return torch.from_numpy(self.x[i][None, :, :, None])

    def samples(self, i):
        return torch.from_numpy(self.y[i][..., None])

    def device(self):
        from asr_amd import ops
        return [ops.to_device(a) for a in (self.y, self.rot, self.tr, self.irot, self.itr)]


@functools.lru_cache(maxsize=None)
def _problem(shape, kind, n, seed):
    return _Problem(shape, kind, n, seed)


def _alphas(iters, b):
    from asr_amd import transforms as T
    a = np.zeros((iters, b), np.float32)
    for it in range(iters):
        a[it, :] = T.adam_alpha(np.float32(1e-3), np.float32(0.9), np.float32(0.999), it + 1)
    return a


_B1, _B2, _EPS = np.float32(0.9), np.float32(0.999), np.float32(1e-7)


def _solve(yd, rot, tr, irot, itr, hw, iters, lam=LAM):
    from asr_amd import ops
    x, _ = ops.sr_solve(ops.sr_init_target(yd, hw), yd, rot, tr, irot, itr, ops.to_device(_alphas(iters, yd.shape[0])), lam,
                        np.float32(1) - _B1, np.float32(1) - _B2, _EPS, True, want_loss=False)
    return x


def _explicit_steps(yd, rot, tr, irot, itr, hw, iters, lam=LAM):
    """iters x (asr_sr_forward_residual_f32 + the fused asr_sr_backward_adam_f32), AMSGrad."""
    from asr_amd import ops
    alphas = _alphas(iters, yd.shape[0])
    xd = ops.sr_init_target(yd, hw)
    m = torch.zeros_like(xd); v = torch.zeros_like(xd); vh = torch.zeros_like(xd)
    for it in range(iters):
        resid = ops.sr_forward_residual(xd, yd, rot, tr)
        xd, _ = ops.sr_backward_adam(xd, resid, irot, itr, lam,
                                     adam=dict(m=m, v=v, vhat=vh, alphas=ops.to_device(alphas[it]),
                                               one_minus_beta1=np.float32(1) - _B1, one_minus_beta2=np.float32(1) - _B2,
                                               epsilon=_EPS, amsgrad=True))
    return xd


def _check_forward_and_gradient(p, tag, lam=LAM):
    """sr_init_target, K_fwd (unbordered), the fused backward in gradient-only mode and the loss terms of problem p against the
    oracle.  Returns the device tensors for further checks."""
    from asr_amd import ops
    yd, rot, tr, irot, itr = p.device()
    x0 = ops.sr_init_target(yd, (p.H, p.W)).cpu().numpy()
    xd = ops.to_device(p.x)
    resid = ops.sr_forward_residual(xd, yd, rot, tr)
    _, grad = ops.sr_backward_adam(xd, resid, irot, itr, lam, adam=None)
    terms = ops.sr_loss_terms(xd, resid).cpu().numpy()
    resid_np, grad_np = resid.cpu().numpy(), grad.cpu().numpy()
    assert np.isfinite(resid_np).all() and np.isfinite(grad_np).all()
    sr = p.oracle(lam)
    worst = dict(x0=0.0, resid=0.0, grad=0.0, terms=0.0)
    refs = []
    for i in range(p.b):
        r_ref, _, _, df, tv, l2, l1 = sr.loss_terms_tf(p.target(i), p.samples(i), p.rot[i], p.tr[i])
        _, g_ref = sr.loss_and_grad_tf(p.target(i), p.samples(i), p.rot[i], p.tr[i], p.irot[i], p.itr[i])
        t_ref = np.array([float(df), float(tv), float(l2), float(l1)])
        refs.append((r_ref, g_ref))
        worst["x0"] = max(worst["x0"], float(np.abs(x0[i] - p.x0_ref[i]).max()))
        worst["resid"] = max(worst["resid"], float(np.abs(resid_np[i] - r_ref.numpy()[..., 0]).max()))
        worst["grad"] = max(worst["grad"], float(np.abs(grad_np[i] - g_ref.numpy()[0, :, :, 0]).max()))
        worst["terms"] = max(worst["terms"], float(np.abs(terms[i] / t_ref - 1.0).max()))
    for k, v in worst.items():
        _report(f"{tag} max |{k} - oracle|" + (" (relative)" if k == "terms" else ""), v)
    for i in range(p.b):
        r_ref, g_ref = refs[i]
        t_ref = [float(t) for t in sr.loss_terms_tf(p.target(i), p.samples(i), p.rot[i], p.tr[i])[3:]]
        np.testing.assert_allclose(x0[i], p.x0_ref[i], rtol=0, atol=ATOL_X0)
        np.testing.assert_allclose(resid_np[i], r_ref.numpy()[..., 0], rtol=0, atol=ATOL_RESID)
        np.testing.assert_allclose(grad_np[i], g_ref.numpy()[0, :, :, 0], rtol=0, atol=ATOL_GRAD)
        np.testing.assert_allclose(terms[i], t_ref, rtol=RTOL_TERMS)
    return (yd, rot, tr, irot, itr), xd, resid, grad, refs


@pytest.mark.parametrize("kind", ["T0", "T1", "T2"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_forward_gradient_terms_match_oracle(dev, shape, kind):
    """All five shapes x {wide reference-like, projective rotation, general translate stage}, n = 5, two images with their own
    data and transforms: x0, residual, gradient and loss terms against the transform-level oracle, and two exact facts about
    the copy that lies wholly out of frame."""
    from asr_amd import ops
    p = _problem(shape, kind, 5, 50)
    (yd, rot, tr, irot, itr), xd, resid, grad, refs = _check_forward_and_gradient(p, f"{shape}/{kind}")
    k = OUT_OF_FRAME
    # forward value 0 -> the residual is -y, bit for bit
    assert torch.equal(resid[:, k], -yd[:, k])
    # no gradient comes back from it: the oracle's contribution of that copy is zero, and by linearity the kernel's gradient
    # of the stack without the copy differs from the full one by that contribution
    sr = p.oracle()
    keep = [i for i in range(p.n) if i != k]
    sel = lambda t: t[:, keep].contiguous()
    resid_wo = ops.sr_forward_residual(xd, sel(yd), sel(rot), sel(tr))
    assert torch.equal(resid_wo, sel(resid))
    _, grad_wo = ops.sr_backward_adam(xd, resid_wo, sel(irot), sel(itr), LAM, adam=None)
    for i in range(p.b):
        contrib = sr.data_grad_copies_tf(refs[i][0], p.irot[i], p.itr[i])[k, :, :, 0].numpy()
        assert not contrib.any()
        d = float(np.abs(grad[i].cpu().numpy() - grad_wo[i].cpu().numpy() - contrib).max())
        _report(f"{shape}/{kind} image {i} |grad - grad without the out-of-frame copy - its oracle contribution|", d)
        assert d <= ATOL_GRAD
    # ... whatever that copy's y holds: every one of its taps is structurally outside, so each is selected to 0
    y2 = yd.clone()
    y2[:, k] = ops.to_device(np.random.default_rng(60).uniform(-2.0, 1.0, tuple(y2[:, k].shape)).astype(np.float32))
    resid2 = ops.sr_forward_residual(xd, y2, rot, tr)
    assert torch.equal(resid2[:, k], -y2[:, k]) and torch.equal(sel(resid2), sel(resid))
    _, grad2 = ops.sr_backward_adam(xd, resid2, irot, itr, LAM, adam=None)
    assert torch.equal(grad2, grad)


def test_bilateral_tv_on_a_rectangle(dev):
    """The BTV window walks W-strided rows: shape A, wide transforms, gradient and the prior's value."""
    from asr_amd import ops
    p = _problem("A", "T0", 5, 50)
    yd, rot, tr, irot, itr = p.device()
    xd = ops.to_device(p.x)
    cfg = ops.sr_config(use_btv=True)
    resid = ops.sr_forward_residual(xd, yd, rot, tr)
    _, grad = ops.sr_backward(xd, resid, irot, itr, LAM, cfg, state=None)
    terms = ops.sr_loss_terms(xd, resid, cfg).cpu().numpy()
    sr = p.oracle(use_btv=True)
    for i in range(p.b):
        _, g_ref = sr.loss_and_grad_tf(p.target(i), p.samples(i), p.rot[i], p.tr[i], p.irot[i], p.itr[i])
        tv_ref = o_sr.bilateral_tv(p.target(i))
        _report(f"A/T0 BTV image {i} max |grad - oracle|", float(np.abs(grad[i].cpu().numpy() - g_ref.numpy()[0, :, :, 0]).max()))
        _report(f"A/T0 BTV image {i} relative |tv - oracle|", abs(terms[i][1] - tv_ref) / tv_ref)
        np.testing.assert_allclose(grad[i].cpu().numpy(), g_ref.numpy()[0, :, :, 0], rtol=0, atol=2e-5)
        assert abs(terms[i][1] - tv_ref) <= 1e-5 * terms[i][1]


@pytest.mark.parametrize("lr_hw,hr_hw", [((10, 18), (25, 50)), ((7, 5), (16, 12))])
def test_init_target_non_integer_ratio(dev, lr_hw, hr_hw):
    """asr_sr_init_target_f32 states no restriction on the shapes: half-pixel bilinear at any ratio."""
    from asr_amd import ops
    rng = np.random.default_rng(51)
    y = rng.standard_normal((2, 3) + lr_hw).astype(np.float32)
    got = ops.sr_init_target(ops.to_device(y), hr_hw).cpu().numpy()
    ref = tf_ops.resize_bilinear(torch.from_numpy(y[:, 0, :, :, None]), hr_hw).numpy()[..., 0]
    _report(f"init {lr_hw} -> {hr_hw} max |x0 - oracle|", float(np.abs(got - ref).max()))
    np.testing.assert_allclose(got, ref, rtol=0, atol=ATOL_X0)


@pytest.mark.parametrize("kind", ["T1", "T2"])
@pytest.mark.parametrize("shape", ["A", "D", "E"])
def test_solve_equals_explicit_steps_on_general_transforms(dev, shape, kind):
    """asr_sr_solve_f32 (bordered K_fwd, K_gt + gather) against 4 explicit unbordered-K_fwd + fused-backward steps, bit for
    bit, where K_fwd's rotation is projective, K_gt takes its generic branch and the gather its non-affine form."""
    p = _problem(shape, kind, 7, 52)
    d = p.device()
    x_solve = _solve(*d, (p.H, p.W), 4)
    x_steps = _explicit_steps(*d, (p.H, p.W), 4)
    assert torch.isfinite(x_solve).all()
    assert torch.equal(x_solve, x_steps), float((x_solve - x_steps).abs().max())


def test_affine_flag_is_per_image_and_sees_every_copy(dev):
    """n = 70: copy 67 is read on the flag kernel's second trip over the copies.  Image 0 is all affine, image 1 is affine but
    for the projective terms in copy 67's inverse rotation."""
    from asr_amd import ops, transforms as T
    H, h, n, b, iters = 64, 16, 70, 2, 3
    rng = np.random.default_rng(53)
    y = np.stack([_blob_masks(rng, n, h, h) for _ in range(b)])
    ang = rng.uniform(-0.15, 0.15, (b, n)).astype(np.float32)
    sh = rng.uniform(-0.15 * H, 0.15 * H, (b, n, 2)).astype(np.float32)
    ang[:, 0] = 0
    sh[:, 0] = 0
    rot = np.stack([T.rotation_transforms(ang[i], H, H) for i in range(b)])
    tr = np.stack([T.translation_transforms(sh[i]) for i in range(b)])
    rot[1, 67, 6:] = [1.0e-3, -0.7e-3]
    irot = np.stack([T.inverse_transforms(rot[i]) for i in range(b)])
    itr = np.stack([T.inverse_transforms(tr[i]) for i in range(b)])
    assert not irot[0, :, 6:].any() and not irot[1, :67, 6:].any() and not irot[1, 68:, 6:].any() and irot[1, 67, 6:].all()
    d = [ops.to_device(a) for a in (y, rot, tr, irot, itr)]
    x_solve = _solve(*d, (H, H), iters)
    x_steps = _explicit_steps(*d, (H, H), iters)
    assert torch.equal(x_solve[0], x_steps[0])
    assert torch.equal(x_solve[1], x_steps[1])
    # the flag is per image: image 0 alone (all affine) gives its batched result
    x_alone = _solve(*[t[:1].contiguous() for t in d], (H, H), iters)
    assert torch.equal(x_alone[0], x_solve[0])
    # and copy 67's projective terms are not ignored
    rot_aff = rot.copy()
    rot_aff[1, 67, 6:] = 0
    irot_aff = np.stack([T.inverse_transforms(rot_aff[i]) for i in range(b)])
    x_aff = _solve(d[0], ops.to_device(rot_aff), d[2], ops.to_device(irot_aff), d[4], (H, H), iters)
    assert torch.equal(x_aff[0], x_solve[0]) and not torch.equal(x_aff[1], x_solve[1])


@pytest.mark.parametrize("n", [1, 2, 9, 12])
def test_copy_count_edges(dev, n):
    """Shape B: a single identity copy, two copies, and the 8 / 4 / 1 unroll tails of the gather with the paired-copy loop of
    the fused kernel (n = 9, 12)."""
    p = _problem("B", "T0", n, 54)
    d, *_ = _check_forward_and_gradient(p, f"B/T0 n={n}")
    x_solve = _solve(*d, (p.H, p.W), 2)
    x_steps = _explicit_steps(*d, (p.H, p.W), 2)
    assert torch.equal(x_solve, x_steps), float((x_solve - x_steps).abs().max())


def test_translate_taps_that_do_not_abut(dev):
    """The rounding-edge fallbacks of the pure-translation fast paths, shape B (f = 2).  A shift of +2^-30 puts the first tap
    column of K_fwd at floor(0 - 2^-30) = -1 and the second at floor(1 - 2^-30 -> 1.0) = 1: not abutting, generic translate
    stage.  A shift of 1 - 2^-23 puts the inverse-translate taps of the HR positions 1 and 2 at floor(2 - 2^-23) = 1 and
    floor(3 - 2^-23 -> 3.0) = 3: the 4 taps {1, 2, 3, 4} span three LR cells, the fused backward's direct-gather branch."""
    H, W = SHAPES["B"][0]
    p = _Problem("B", "T0", 4, 55)
    tiny, edge = np.float32(2.0 ** -30), np.float32(1.0 - 2.0 ** -23)
    ang = np.array([0.0, 0.1, 0.0, -0.3], np.float32)
    sh = np.array([[0, 0], [tiny, tiny], [edge, edge], [edge, tiny]], np.float32)
    for i in range(p.b):
        p.rot[i] = tf_ops.angles_to_projective_transforms(ang * (1 + i), H, W)
        p.tr[i] = tf_ops.translations_to_projective_transforms(sh)
        p.irot[i], p.itr[i] = tf_ops.invert_transforms(p.rot[i]), tf_ops.invert_transforms(p.tr[i])
    assert np.array_equal(p.itr[0][:, [2, 5]], sh) and np.array_equal(p.itr[0][:, [0, 1, 3, 4, 6, 7]], p.tr[0][:, [0, 1, 3, 4, 6, 7]])
    assert np.float32(0.0) - tiny < 0 and np.float32(1.0) - tiny == 1 and np.float32(2.0) + edge == 3 and np.float32(1.0) + edge < 2
    d, *_ = _check_forward_and_gradient(p, "B/rounding edges")
    x_solve = _solve(*d, (H, W), 2)
    x_steps = _explicit_steps(*d, (H, W), 2)
    assert torch.equal(x_solve, x_steps), float((x_solve - x_steps).abs().max())


def _realign_case(p, case):
    """trans_tf / rot_tf of translate(-shifts) / rotate(-angles) for wide angles and shifts; "trans": a non-pure translate
    stage on two copies; "proj": projective terms in two copies' rotation."""
    rng = np.random.default_rng(56)
    tfs = []
    for i in range(p.b):
        ang = rng.uniform(-0.6, 0.6, p.n).astype(np.float32)
        sh = (rng.uniform(-0.3, 0.3, (p.n, 2)) * [p.W, p.H]).astype(np.float32)
        ang[0] = 0
        sh[0] = 0
        sh[1] = np.round(sh[1])
        tr = tf_ops.translations_to_projective_transforms(-sh)
        rot = tf_ops.angles_to_projective_transforms(-ang, p.H, p.W)
        if case == "trans":
            tr[2, :2] = [1.05, 0.03]
            tr[4, 6:] = [0.9e-3, -1.2e-3]
        elif case == "proj":
            rot[1, 6:] = [-1.1e-3, 0.8e-3]
            rot[3, 6:] = [0.6e-3, 1.4e-3]
        for t in (tr, rot):
            lo, hi = _proj_range(t, p.H, p.W)
            assert 0.5 <= lo and hi <= 1.5
        tfs.append((tr, rot))
    return np.stack([t[0] for t in tfs]), np.stack([t[1] for t in tfs])


@pytest.mark.parametrize("case", ["wide", "trans", "proj"])
@pytest.mark.parametrize("shape", ["A", "D", "E"])
def test_realign_on_rectangles_signed_inputs_and_general_transforms(dev, shape, case):
    """max / mean / both on signed inputs (slice_max class masks are raw logits): where every warped copy is negative or out
    of frame, the zero fill is the maximum."""
    from asr_amd import ops
    p = _problem(shape, "T0", 5, 57)
    rng = np.random.default_rng(58)
    y = rng.uniform(-1.0, 1.0, p.y.shape).astype(np.float32)
    y[:, 2] = -np.abs(y[:, 2]) - 0.01                      # one copy all negative
    y[:, 0] = -np.abs(y[:, 0]) - 0.01                      # and the identity copy, so that zero can win at all
    tr, rot = _realign_case(p, case)
    yd, trd, rotd = ops.to_device(y), ops.to_device(tr), ops.to_device(rot)
    mx = ops.realign(yd, trd, rotd, (p.H, p.W), "max")
    mn = ops.realign(yd, trd, rotd, (p.H, p.W), "mean")
    both = ops.realign(yd, trd, rotd, (p.H, p.W), "both")
    assert torch.equal(both[0], mx) and torch.equal(both[1], mn)
    sr = p.oracle()
    zero_is_max = 0
    for i in range(p.b):
        r = sr._realign_tf(y[i][..., None], tr[i], rot[i])
        ref_max, ref_mean = sr.max_of(r)[:, :, 0], sr.mean_of(r)[:, :, 0]
        _report(f"{shape}/{case} image {i} max |realign max - oracle|", float(np.abs(mx[i].cpu().numpy() - ref_max).max()))
        _report(f"{shape}/{case} image {i} max |realign mean - oracle|", float(np.abs(mn[i].cpu().numpy() - ref_mean).max()))
        np.testing.assert_allclose(mx[i].cpu().numpy(), ref_max, rtol=0, atol=ATOL_REALIGN)
        np.testing.assert_allclose(mn[i].cpu().numpy(), ref_mean, rtol=0, atol=ATOL_REALIGN)
        # pixels (taken from the oracle) where every warped copy is negative or exactly zero (out of frame), at least one of each
        r_np = r.numpy()[..., 0]
        where = np.argwhere((r_np <= 0).all(0) & (r_np == 0).any(0) & (r_np < -1e-3).any(0))
        zero_is_max += len(where)
        got = mx[i].cpu().numpy()
        assert all(got[yy, xx] == 0.0 for yy, xx in where)
    assert zero_is_max > 0


UNSUPPORTED = [((64, 96), (16, 16)),      # unequal factors on the two axes
               ((48, 48), (16, 16)),      # f = 3: odd
               ((50, 64), (16, 16)),      # not a multiple
               ((16, 16), (16, 16))]      # f = 1


@pytest.mark.parametrize("hr_hw,lr_hw", UNSUPPORTED)
def test_unsupported_shapes_are_refused(dev, hr_hw, lr_hw):
    """check_dims (csrc/sr.hip): the solver entry points take an even integer factor, the same on both axes, and nothing else;
    they refuse before anything is written.  asr_realign_* has no such restriction (include/asr_hip.h): it upsamples at any
    ratio, and is held to the oracle on the same shapes."""
    from asr_amd import _lib, ops
    (H, W), (h, w) = hr_hw, lr_hw
    b, n = 2, 3
    rng = np.random.default_rng(59)
    y = rng.random((b, n, h, w), dtype=np.float32)
    ang = np.array([0.0, 0.2, -0.4], np.float32)
    sh = np.array([[0, 0], [3.25, -2.5], [-5, 4]], np.float32)
    rot = np.stack([tf_ops.angles_to_projective_transforms(ang, H, W)] * b)
    tr = np.stack([tf_ops.translations_to_projective_transforms(sh)] * b)
    yd, rotd, trd = ops.to_device(y), ops.to_device(rot), ops.to_device(tr)
    irotd = ops.to_device(np.stack([tf_ops.invert_transforms(t) for t in rot]))
    itrd = ops.to_device(np.stack([tf_ops.invert_transforms(t) for t in tr]))
    fill = 7.25
    xd = torch.full((b, H, W), fill, dtype=torch.float32, device=yd.device)
    alphas = ops.to_device(_alphas(2, b))
    adam = lambda: dict(m=torch.zeros_like(xd), v=torch.zeros_like(xd), vhat=torch.zeros_like(xd), alphas=alphas[0].contiguous(),
                        one_minus_beta1=0.1, one_minus_beta2=0.001, epsilon=1e-7, amsgrad=True)
    with pytest.raises(_lib.AsrError):
        ops.sr_forward_residual(xd, yd, rotd, trd)
    with pytest.raises(_lib.AsrError):
        ops.sr_backward_adam(xd, yd, irotd, itrd, LAM, adam=None)
    with pytest.raises(_lib.AsrError):
        ops.sr_backward_adam(xd, yd, irotd, itrd, LAM, adam=adam())
    with pytest.raises(_lib.AsrError):
        ops.sr_solve(xd, yd, rotd, trd, irotd, itrd, alphas, LAM, 0.1, 0.001, 1e-7, True)
    assert torch.all(xd == fill)                                                 # the solver's in-place x
    # pre-filled outputs through the C ABI itself
    out_lr = torch.full_like(yd, fill)
    out_hr = [torch.full_like(xd, fill) for _ in range(5)]
    with pytest.raises(_lib.AsrError):
        _lib.call("asr_sr_forward_residual_f32", _lib.ptr(xd), _lib.ptr(yd), _lib.ptr(rotd), _lib.ptr(trd), _lib.ptr(out_lr),
                  b, n, H, W, h, w, _lib.stream_ptr())
    with pytest.raises(_lib.AsrError):
        _lib.call("asr_sr_backward_adam_f32", _lib.ptr(xd), _lib.ptr(out_hr[0]), _lib.ptr(yd), _lib.ptr(irotd), _lib.ptr(itrd),
                  _lib.ptr(out_hr[1]), _lib.ptr(out_hr[2]), _lib.ptr(out_hr[3]), _lib.ptr(alphas), _lib.ptr(out_hr[4]),
                  b, n, H, W, h, w, 1.0, 0.3, 0.7, 0.05, 0.1, 0.001, 1e-7, 1, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert torch.all(out_lr == fill) and all(torch.all(t == fill) for t in out_hr)
    # realign: any ratio
    sr = o_sr.Superresolution(1, 0, 0, 0, num_aug=n, feature_size=(h, w), output_size=(H, W))
    mx, mn = ops.realign(yd, trd, rotd, (H, W), "both")
    for i in range(b):
        r = sr._realign_tf(y[i][..., None], tr[i], rot[i])
        np.testing.assert_allclose(mx[i].cpu().numpy(), sr.max_of(r)[:, :, 0], rtol=0, atol=ATOL_REALIGN)
        np.testing.assert_allclose(mn[i].cpu().numpy(), sr.mean_of(r)[:, :, 0], rtol=0, atol=ATOL_REALIGN)
