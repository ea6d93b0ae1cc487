"""The exact-adjoint data gradient on the device (include/asr_hip.h, "exact adjoint"; adjoint="exact" through ops.sr_backward,
ops.sr_data_bound and ops.sr_solve) against its restatement tests/sr_adj_ref.py bit for bit, against the dense transpose of the
device's own forward operator within the float32 bound of tests/test_sr_adj_host.py, and on what a true gradient gives: a
symmetric map, a bound that is one, a loss that falls at step 1 / bound."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import sr as o_sr
from oracle import tf_ops
from test_gpu_sr_wtv import _adam_alphas, _adam_cfg
from test_sr_adj_host import make_transforms, transpose_bound

import sr_adj_ref as A
import sr_ml_ref as ML
import sr_pd_ref as P
import sr_rw_ref as RW

pytestmark = pytest.mark.gpu

SHAPES = [(8, 8, 4, 4), (8, 12, 4, 6), (12, 20, 3, 5), (16, 24, 2, 3), (32, 32, 8, 8)]
COPIES = (1, 5, 9, 13)              # the 8 / 4 / 1 tails of the registered unroll and the 4 / 1 tails of the exact one
BATCH = 2
LAM_DF = (1.0, 0.0, 0.0, 0.0)


@functools.lru_cache(maxsize=None)
def _case(H, W, h, w, n, b=BATCH, zero_angles=False):
    """Host arrays of a case: computed once, shared by the tests, never changed.  Image i's fixed angles are rolled by i."""
    rng = np.random.default_rng(1000 * H + 10 * W + n)
    tfs, angs, shs = [], [], []
    for i in range(b):
        angles, shifts = make_transforms(rng, n, H, W)
        k = min(n, 3)
        angles[:k] = np.roll(np.array([0.0, np.pi / 2, np.pi / 4], np.float32), i)[:k]
        if zero_angles:
            angles[:] = 0
        tfs.append(P.transforms(angles, shifts, (H, W)))
        angs.append(angles)
        shs.append(shifts)
    resid = rng.standard_normal((b, n, h, w)).astype(np.float32)
    x = rng.random((b, H, W), dtype=np.float32)
    y = rng.random((b, n, h, w), dtype=np.float32)
    return SimpleNamespace(H=H, W=W, h=h, w=w, n=n, b=b, tfs=tfs, angs=angs, shs=shs, resid=resid, x=x, y=y)


def _dev_tfs(tfs):
    from asr_amd import ops
    return [ops.to_device(np.stack([t[k] for t in tfs]).astype(np.float32)) for k in range(4)]


def _grad(x, resid, tf, adjoint, chunk=0, lam=LAM_DF):
    """grad_out of one gradient-only call -> host array [b, H, W]."""
    from asr_amd import ops
    _, g = ops.sr_backward(ops.to_device(x), ops.to_device(resid), tf[2], tf[3], lam, ops.sr_config(plane_chunk=chunk), state=None,
                           want_grad=True, rot_tf=tf[0], trans_tf=tf[1], adjoint=adjoint)
    return g.cpu().numpy()


def _report(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    bad = int((got != want).sum())
    print(f"{what}: {bad} of {got.size} values differ, max |diff| {float(np.abs(got.astype(np.float64) - want).max()):.3e}")
    return bad


# ---- 3. bit for bit against the restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", COPIES)
@pytest.mark.parametrize("H,W,h,w", SHAPES)
def test_exact_gradient_is_the_restatement_bit_for_bit(dev, H, W, h, w, n):
    c = _case(H, W, h, w, n)
    tf = _dev_tfs(c.tfs)
    want = np.stack([A.data_grad_from_resid(c.resid[i], c.tfs[i], (H, W), 1.0, "exact") for i in range(c.b)])
    whole = _grad(c.x, c.resid, tf, "exact")
    for i in range(c.b):
        _report(f"{H}x{W} n={n} image {i}", whole[i], want[i])
    assert np.array_equal(whole, want)
    assert _grad(c.x, c.resid, tf, "exact", chunk=3).tobytes() == whole.tobytes()
    for i in range(c.b):                                              # an image alone is the image in its batch
        alone = _grad(c.x[i:i + 1], c.resid[i:i + 1], _dev_tfs(c.tfs[i:i + 1]), "exact", chunk=3)
        assert alone.tobytes() == whole[i:i + 1].tobytes(), i
    if n > 1:
        assert not np.array_equal(whole, _grad(c.x, c.resid, tf, "registered"))


# ---- 4. the dense transpose of the device's own forward operator ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dense_forward(H, W, h, w, n, image=0):
    """A [n*h*w, H*W] float64: ops.sr_forward_residual on the H*W unit impulses (y = 0, one impulse per batch entry)."""
    from asr_amd import ops
    c = _case(H, W, h, w, n)
    P_ = H * W
    eye = ops.to_device(np.eye(P_, dtype=np.float32).reshape(P_, H, W))
    y0 = torch.zeros((P_, n, h, w), dtype=torch.float32, device=eye.device)
    rot, tr = (ops.to_device(np.tile(c.tfs[image][k][None], (P_, 1, 1)).astype(np.float32)) for k in (0, 1))
    r = ops.sr_forward_residual(eye, y0, rot, tr)
    return r.reshape(P_, n * h * w).cpu().numpy().astype(np.float64).T.copy()


@pytest.mark.parametrize("H,W,h,w,n", [(8, 8, 4, 4, 5), (12, 20, 3, 5, 13)])
def test_exact_gradient_is_the_dense_transpose_and_the_registered_one_is_not(dev, H, W, h, w, n):
    c = _case(H, W, h, w, n)
    Amat = _dense_forward(H, W, h, w, n)
    r = c.resid[0]
    want = 2.0 * (Amat.T @ r.reshape(-1).astype(np.float64))
    tol = transpose_bound(Amat, r, (H, W), n)
    tf = _dev_tfs(c.tfs[:1])
    exact = _grad(c.x[:1], c.resid[:1], tf, "exact")[0].reshape(-1).astype(np.float64)
    reg = _grad(c.x[:1], c.resid[:1], tf, None)[0].reshape(-1).astype(np.float64)       # the same call with the default
    used = np.abs(exact - want) / tol
    over = np.abs(reg - want) > tol
    print(f"{H}x{W} n={n}: exact uses at most {used.max():.3f} of the bound; registered exceeds it at {over.mean():.2%} of the pixels")
    assert (used <= 1.0).all()
    assert over.mean() >= 0.5


# ---- 5. symmetry ------------------------------------------------------------------------------------------------------------------------
def _apply_m(c, tf, v, adjoint):
    """M v for every image of the case: the forward residual at y = 0, then grad_out (lambda_df = 1)."""
    from asr_amd import ops
    vd = ops.to_device(v)
    q = ops.sr_forward_residual(vd, torch.zeros_like(ops.to_device(c.y)), tf[0], tf[1])
    return _grad(v, q.cpu().numpy(), tf, adjoint).astype(np.float64)


@pytest.mark.parametrize("H,W,h,w", SHAPES)
def test_the_exact_map_is_symmetric(dev, H, W, h, w):
    c = _case(H, W, h, w, 5)
    tf = _dev_tfs(c.tfs)
    rng = np.random.default_rng(5)
    u, v = (rng.standard_normal((c.b, H, W)).astype(np.float32) for _ in range(2))
    mu, mv, mabs = _apply_m(c, tf, u, "exact"), _apply_m(c, tf, v, "exact"), _apply_m(c, tf, np.abs(v), "exact")
    ru, rv = _apply_m(c, tf, u, "registered"), _apply_m(c, tf, v, "registered")
    for i in range(c.b):
        lhs, rhs = float((u[i] * mv[i]).sum()), float((mu[i] * v[i]).sum())
        tol = 2.0 ** -24 * 64 * float((np.abs(u[i]) * mabs[i]).sum())
        reg_gap = abs(float((u[i] * rv[i]).sum()) - float((ru[i] * v[i]).sum()))
        print(f"{H}x{W} image {i}: <u,Mv> {lhs:.6f} <Mu,v> {rhs:.6f} gap {abs(lhs - rhs):.3e} tol {tol:.3e}; registered gap {reg_gap:.3e}")
        assert abs(lhs - rhs) <= tol
        assert reg_gap > tol                                            # what the tolerance tells apart


# ---- 6. the bound is a bound ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,h,w", [(8, 8, 4, 4), (8, 12, 4, 6)])
def test_the_exact_bound_is_above_the_largest_eigenvalue(dev, H, W, h, w):
    from asr_amd import ops
    n = 5
    c = _case(H, W, h, w, n)
    tf = _dev_tfs(c.tfs)
    lam_max = [float(np.linalg.eigvalsh(2.0 * (Am.T @ Am))[-1]) for Am in (_dense_forward(H, W, h, w, n, i) for i in range(c.b))]
    last = None
    for k in (1, 6, 64):
        got = ops.sr_data_bound(*tf, (H, W), (h, w), 1.0, iters=k, adjoint="exact").cpu().numpy()
        print(f"{H}x{W} iters={k}: bound {got.tolist()} largest eigenvalue {lam_max}")
        for i in range(c.b):
            assert got[i] >= (1.0 - 1e-5) * lam_max[i]
        assert last is None or (got <= last).all()
        last = got
    chunked = ops.sr_data_bound(*tf, (H, W), (h, w), 1.0, iters=6, adjoint="exact", cfg=ops.sr_config(plane_chunk=3)).cpu().numpy()
    assert chunked.tobytes() == ops.sr_data_bound(*tf, (H, W), (h, w), 1.0, iters=6, adjoint="exact").cpu().numpy().tobytes()
    reg = ops.sr_data_bound(*tf, (H, W), (h, w), 1.0, iters=6, adjoint="registered").cpu().numpy()
    assert reg.tobytes() == ops.sr_data_bound(*tf, (H, W), (h, w), 1.0, iters=6).cpu().numpy().tobytes()


# ---- 7. pure translations ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,h,w", SHAPES)
def test_with_every_angle_zero_both_forms_are_equal(dev, H, W, h, w):
    c = _case(H, W, h, w, 9, zero_angles=True)
    tf = _dev_tfs(c.tfs)
    exact, reg = _grad(c.x, c.resid, tf, "exact"), _grad(c.x, c.resid, tf, "registered")
    assert (exact == reg).all() and (exact != 0).any()


# ---- 8. fallback -----------------------------------------------------------------------------------------------------------------------
def test_a_projective_rotation_takes_the_registered_statements(dev):
    from asr_amd import ops
    H, W, h, w, n = 12, 20, 3, 5, 5
    c = _case(H, W, h, w, n)
    tfs = [tuple(t.copy() for t in c.tfs[i]) for i in range(c.b)]
    tfs[0][0][2, 6] = 1e-3                                              # one projective rot_tf in image 0, and its inverse
    tfs[0][2][:] = tf_ops.invert_transforms(tfs[0][0])
    tf = _dev_tfs(tfs)
    flags = ops.sr_adjoint_flags(tf[0], tf[1], tf[2]).cpu().numpy()
    assert flags.dtype == np.int32 and flags.tolist() == [0, 1]
    for i in range(c.b):
        assert A.exact_applies(tfs[i][0], tfs[i][1], tfs[i][2]) == flags[i]
    exact, reg = _grad(c.x, c.resid, tf, "exact"), _grad(c.x, c.resid, tf, "registered")
    assert exact[0].tobytes() == reg[0].tobytes()
    assert not np.array_equal(exact[1], reg[1])
    assert np.array_equal(exact[1], A.data_grad_from_resid(c.resid[1], tfs[1], (H, W), 1.0, "exact"))
    tfs[1][1][0, 1] = 0.25                                              # a translate that is not pure: image 1 falls back too
    tf = _dev_tfs(tfs)
    assert ops.sr_adjoint_flags(tf[0], tf[1], tf[2]).cpu().numpy().tolist() == [0, 0]


# ---- 9. solves ---------------------------------------------------------------------------------------------------------------------------
SOLVE = (12, 20, 3, 5, 5)
LAM = (1.0, 0.3, 0.01, 0.0)


def _solve(c, tf, alphas, cfg, x0=None, lam=LAM, state=None, **kw):
    from asr_amd import ops
    st = {} if state is None else state
    out = ops.sr_solve(ops.to_device(c.x if x0 is None else x0), ops.to_device(c.y), *tf,
                       ops.to_device(np.ascontiguousarray(alphas, np.float32)), lam, cfg=cfg, state=st, want_loss=False, **kw)
    return out, st


def test_ten_iterations_are_ten_one_step_calls(dev):
    from asr_amd import ops
    c = _case(*SOLVE)
    tf = _dev_tfs(c.tfs)
    alphas = _adam_alphas(10, c.b, lr=1e-2)
    for chunk in (0, 3):
        (x, _), st = _solve(c, tf, alphas, _adam_cfg(chunk), adjoint="exact")
        xs = ops.to_device(c.x)
        yd = ops.to_device(c.y)
        slots = {k: torch.zeros_like(xs) for k in ("m", "v", "vhat")}
        for it in range(10):
            q = ops.sr_forward_residual(xs, yd, tf[0], tf[1])
            xs, _ = ops.sr_backward(xs, q, tf[2], tf[3], LAM, _adam_cfg(chunk), state=dict(slots, alphas=ops.to_device(alphas[it])),
                                    rot_tf=tf[0], trans_tf=tf[1], adjoint="exact")
        assert torch.equal(x, xs)
        for k in slots:
            assert torch.equal(st[k], slots[k]), k


def test_registered_is_the_call_without_the_keyword(dev):
    c = _case(*SOLVE)
    tf = _dev_tfs(c.tfs)
    alphas = _adam_alphas(10, c.b, lr=1e-2)
    (a, _), sa = _solve(c, tf, alphas, _adam_cfg())
    (b_, _), sb = _solve(c, tf, alphas, _adam_cfg(), adjoint="registered")
    (e, _), _ = _solve(c, tf, alphas, _adam_cfg(), adjoint="exact")
    assert torch.equal(a, b_) and all(torch.equal(sa[k], sb[k]) for k in ("m", "v", "vhat"))
    assert not torch.equal(a, e)


def _pd_cfg(chunk=0):
    from asr_amd import _lib, ops
    return ops.sr_config(_lib.OPT_PRIMAL_DUAL, c0=P.DUAL_RATIO, plane_chunk=chunk)


def _pd_taus(c, tf):
    from asr_amd import ops
    bound = ops.sr_data_bound(*tf, (c.H, c.W), (c.h, c.w), LAM[0], iters=6, adjoint="exact")
    return ops.pd_steps(bound, LAM[2], 1).cpu().numpy()[0]


def _pd_restated(c, taus, iters, group=None):
    srs = [P.make_sr(LAM, c.n, (c.h, c.w), (c.H, c.W)) for _ in range(c.b)]
    x, py, px = c.x.copy(), np.zeros_like(c.x), np.zeros_like(c.x)
    for _ in range(iters):
        new = [P.pd_update(srs[i], x[i], py[i], px[i], A.data_grad(srs[i], x[i], c.y[i], c.tfs[i], "exact"), taus[i]) for i in range(c.b)]
        x, py, px = (np.stack([s[k] for s in new]) for k in range(3))
        if group:
            x = ML.project_groups(x, group)
    return x, py, px


@pytest.mark.parametrize("coupling", [None, 2])
def test_primal_dual_and_the_coupling_against_the_restatement(dev, coupling):
    c = _case(*SOLVE)
    tf = _dev_tfs(c.tfs)
    taus = _pd_taus(c, tf)
    want = _pd_restated(c, taus, 3, coupling)
    for chunk in (0, 3):
        (x, _), st = _solve(c, tf, np.tile(taus[None], (3, 1)), _pd_cfg(chunk), adjoint="exact", coupling=coupling)
        for what, got, w_ in zip(("x", "p_y", "p_x"), (x, st["m"], st["v"]), want):
            _report(f"coupling={coupling} chunk={chunk} {what}", got.cpu().numpy(), w_)
            assert np.array_equal(got.cpu().numpy(), w_), (coupling, chunk, what)


def test_a_frozen_image_keeps_x_and_both_duals_under_the_exact_form(dev):
    c = _case(*SOLVE)
    tf = _dev_tfs(c.tfs)
    taus = _pd_taus(c, tf)
    iters = 6
    alphas = np.tile(np.array([1e-7, taus[1]], np.float32)[None], (iters, 1))
    mon = dict(every=1, rel_tol=1e-3, patience=2, min_iter=0, history=True)
    (x, _, trace), st = _solve(c, tf, alphas, _pd_cfg(), adjoint="exact", monitor=mon)
    done = trace.iters_done.cpu().numpy()
    print("iters_done", done.tolist())
    assert done[0] == 2 and done[0] < done[1] <= iters
    for i in range(c.b):
        (cx, _), cs = _solve(c, tf, alphas[:done[i]], _pd_cfg(), adjoint="exact")
        for what, got, w_ in zip(("x", "p_y", "p_x"), (x, st["m"], st["v"]), (cx, cs["m"], cs["v"])):
            assert torch.equal(got[i], w_[i]), (i, what)


class _ExactReweighted(RW.ReweightedSuperresolution, A.ExactAdjoint):
    """tests/sr_rw_ref's reweighted AMSGrad solve with the gradient swapped."""


def test_the_reweighted_amsgrad_solve_against_the_restatement(dev):
    c = _case(*SOLVE)
    tf = _dev_tfs(c.tfs)
    iters, lr = 8, 1e-2
    rw = dict(kind="cauchy", kappa=2.0, every=3, start=2, history=True)
    x0 = np.stack([tf_ops.resize_bilinear(torch.from_numpy(c.y[i, 0:1, :, :, None]), (c.H, c.W)).numpy()[0, :, :, 0] for i in range(c.b)])
    out, _ = _solve(c, tf, _adam_alphas(iters, c.b, lr=lr), _adam_cfg(), x0=x0, adjoint="exact", reweight=rw)
    for i in range(c.b):
        sr = _ExactReweighted(*LAM, num_iter=iters, num_aug=c.n, optimizer=o_sr.Optimizer("adam", lr, amsgrad=True),
                              feature_size=(c.h, c.w), output_size=(c.H, c.W), rw_kind="cauchy", rw_kappa=2.0, rw_every=3, rw_start=2)
        want, _ = sr.augmented_superresolution(c.y[i][..., None], c.angs[i], c.shs[i])
        _report(f"image {i} x", out[0][i].cpu().numpy(), want[:, :, 0])
        assert np.array_equal(out[0][i].cpu().numpy(), want[:, :, 0])
        assert np.array_equal(out[-1].weights[i].cpu().numpy(), sr.copy_weights)
        assert np.array_equal(out[-1].history[:, i].cpu().numpy(), sr.history)


def test_the_superresolution_object_hands_the_option_down(dev):
    from asr_amd import ops
    from asr_amd.superresolution_scripts.optimizer import Optimizer
    from asr_amd.superresolution_scripts.superresolution import Superresolution
    c = _case(*SOLVE)
    copies = ops.to_device(c.y)
    angs, shs = np.stack(c.angs), np.stack(c.shs)

    def run(rule, **kw):
        opt = Optimizer("adam", 1e-2, amsgrad=True) if rule == "adam" else Optimizer("primal_dual")
        sr = Superresolution(*LAM, num_iter=6, num_aug=c.n, optimizer=opt, feature_size=(c.h, c.w), output_size=(c.H, c.W), **kw)
        return sr, sr.augmented_superresolution_batch(copies, angs, shs)[0]

    for rule in ("adam", "pd"):
        sr, exact = run(rule, adjoint="exact")
        assert torch.equal(run(rule)[1], run(rule, adjoint="registered")[1])
        assert not torch.equal(exact, run(rule)[1])
        rot, tr = sr._transforms(angs, shs, dev)
        irot, itr = sr._transforms(angs, shs, dev, inverse=True)
        kw = {}
        if rule == "adam":                       # the object's own schedule: the global step counter advances image by image
            fresh = Optimizer("adam", 1e-2, amsgrad=True)
            alphas = ops.to_device(np.stack([fresh.schedule_alphas(6) for _ in range(c.b)], axis=1))
            cfg, kw = fresh.optimizer.config(use_btv=False), dict(slot_init=fresh.optimizer.slot_init)
        else:
            cfg = _pd_cfg()
            alphas = ops.pd_steps(ops.sr_data_bound(rot, tr, irot, itr, (c.H, c.W), (c.h, c.w), LAM[0], iters=6, adjoint="exact"), LAM[2], 6)
        want = ops.sr_solve(ops.sr_init_target(copies, (c.H, c.W)), copies, rot, tr, irot, itr, alphas, LAM, cfg=cfg, adjoint="exact",
                            **kw)[0]
        assert torch.equal(exact, want), rule


# ---- 10. descent ---------------------------------------------------------------------------------------------------------------------
def test_plain_gradient_descent_at_one_over_the_bound_never_raises_the_loss(dev):
    from asr_amd import _lib, ops
    H, W, h, w, n = 32, 32, 8, 8, 13
    c = _case(H, W, h, w, n)
    tf = _dev_tfs(c.tfs)
    lam = (1.0, 0.0, 0.01, 0.0)
    iters = 31                                                          # the losses before iterations 0 .. 30: thirty steps
    bound = ops.sr_data_bound(*tf, (H, W), (h, w), lam[0], iters=6, adjoint="exact")
    alphas = (1.0 / bound)[None].expand(iters, -1).contiguous().cpu().numpy()
    mon = dict(every=1, rel_tol=0.0, patience=0, min_iter=0, history=True)
    (_, _, trace), _ = _solve(c, tf, alphas, ops.sr_config(_lib.OPT_SGD), lam=lam, adjoint="exact", monitor=mon)
    losses = np.asarray(trace.losses(lam), dtype=np.float64)
    assert losses.shape == (iters, c.b) and np.isfinite(losses).all()
    rise = (losses[1:] - losses[:-1]) / losses[:-1]
    print("losses", losses[::5].tolist(), "largest relative rise", float(rise.max()))
    assert (rise <= 1e-6).all()
    assert (losses[-1] < 0.9 * losses[0]).all()
