"""The exact-adjoint gather on the device beyond rotations and on every instantiation (csrc/sr_adj_kernels.h; include/asr_hip.h,
"exact adjoint"): the transform families of tests/sr_adj_cases.py take the gather through its counted loop, the four clamps at
the plane border, the decision at 1.46875 and the fallbacks at half-width 8 and at |translation| 16384, in batches whose images
take different modes; the cases of its table launch the eight gather forms <WTV, MON> of both rules.  Everything is held bit
for bit against the restatement tests/sr_adj_ref.py, or within tests/test_sr_adj_host.transpose_bound against the dense
transpose of the device's own forward operator."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import tf_ops
from test_gpu_sr_adj import LAM, LAM_DF, _apply_m, _dev_tfs, _grad, _pd_cfg, _report, _solve
from test_gpu_sr_wtv import _adam_alphas, _adam_cfg
from test_sr_adj_host import transpose_bound

import sr_adj_cases as T
import sr_adj_ref as A
import sr_pd_ref as P
import sr_update_ref as RU
import sr_wtv_ref as WTV

pytestmark = pytest.mark.gpu

N = T.FORM_N
SHAPE = T.FORM_SHAPE                                            # (12, 20, 3, 5)
DENSE_SHAPES = [T.SHAPES[0], T.SHAPES[2]]                       # (12, 20, 3, 5) and (8, 8, 4, 4)


def _sid(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


@functools.lru_cache(maxsize=None)
def _want(shape, family, n, b=None):
    """The restated exact gradient of every image of a problem [b, H, W]: computed once, shared, never changed."""
    p = T.problem(shape, family, n, b)
    return np.stack([A.data_grad_from_resid(p.resid[i], p.tfs[i], shape[:2], 1.0, "exact") for i in range(p.b)])


def _flags(tf):
    from asr_amd import ops
    return ops.sr_adjoint_flags(tf[0], tf[1], tf[2]).cpu().numpy()


# ---- 1. bit for bit against the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", T.SHAPES, ids=_sid)
@pytest.mark.parametrize("family", list(T.FAMILIES))
def test_every_family_is_the_restatement_bit_for_bit(dev, family, shape):
    exact = T.FAMILIES[family][2]
    for n in T.COPIES:
        p = T.problem(shape, family, n)
        tf = _dev_tfs(p.tfs)
        want = _want(shape, family, n)
        whole = _grad(p.x, p.resid, tf, "exact")
        for i in range(p.b):
            _report(f"{family} {_sid(shape)} n={n} image {i}", whole[i], want[i])
        assert np.array_equal(whole, want)
        assert _flags(tf).tolist() == [A.exact_applies(*t[:3]) for t in p.tfs] == [int(exact)] * p.b
        for chunk in T.CHUNKS[1:]:
            assert _grad(p.x, p.resid, tf, "exact", chunk=chunk).tobytes() == whole.tobytes(), (n, chunk)
        for i in range(p.b):                                          # an image alone is the image in its batch
            alone = _grad(p.x[i:i + 1], p.resid[i:i + 1], _dev_tfs(p.tfs[i:i + 1]), "exact", chunk=3)
            assert alone.tobytes() == whole[i:i + 1].tobytes(), (n, i)
        reg = _grad(p.x, p.resid, tf, "registered")
        if not exact:
            assert whole.tobytes() == reg.tobytes()
        elif n > 1:
            assert whole.any() and not np.array_equal(whole, reg)


# ---- 2. the dense transpose of the device's own forward operator -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dense_forward(shape, family, n, image=0, b=None):
    """A [n*h*w, H*W] float64: ops.sr_forward_residual on the H*W unit impulses (y = 0, one impulse per batch entry)."""
    from asr_amd import ops
    H, W, h, w = shape
    p = T.problem(shape, family, n, b)
    P_ = H * W
    eye = ops.to_device(np.eye(P_, dtype=np.float32).reshape(P_, H, W))
    y0 = torch.zeros((P_, n, h, w), dtype=torch.float32, device=eye.device)
    rot, tr = (ops.to_device(np.tile(p.tfs[image][k][None], (P_, 1, 1)).astype(np.float32)) for k in (0, 1))
    r = ops.sr_forward_residual(eye, y0, rot, tr)
    return r.reshape(P_, n * h * w).cpu().numpy().astype(np.float64).T.copy()


@pytest.mark.parametrize("shape", DENSE_SHAPES, ids=_sid)
@pytest.mark.parametrize("family", ["zoom2", "zoom5", "aniso_shear"])
def test_the_counted_loop_is_the_dense_transpose_and_the_registered_gradient_is_not(dev, family, shape):
    p = T.problem(shape, family, N)
    Amat = _dense_forward(shape, family, N)
    r = p.resid[0]
    want = 2.0 * (Amat.T @ r.reshape(-1).astype(np.float64))
    tol = transpose_bound(Amat, r, shape[:2], N)
    tf = _dev_tfs(p.tfs[:1])
    exact = _grad(p.x[:1], p.resid[:1], tf, "exact")[0]
    reg = _grad(p.x[:1], p.resid[:1], tf, "registered")[0]
    used = np.abs(exact.reshape(-1).astype(np.float64) - want) / tol
    print(f"{family} {_sid(shape)} n={N}: halves up to {T.halves(p.tfs[0][2]).max():.4f}; exact uses at most {used.max():.4f} of the bound")
    assert want.any() and (used <= 1.0).all()
    assert not np.array_equal(exact, reg)


# ---- 3. symmetry ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["zoom2", "aniso_shear"])
def test_the_exact_map_is_symmetric_on_the_counted_loop(dev, family):
    H, W = SHAPE[:2]
    p = T.problem(SHAPE, family, N)
    tf = _dev_tfs(p.tfs)
    rng = np.random.default_rng(5)
    u, v = (rng.standard_normal((p.b, H, W)).astype(np.float32) for _ in range(2))
    mu, mv, mabs = _apply_m(p, tf, u, "exact"), _apply_m(p, tf, v, "exact"), _apply_m(p, tf, np.abs(v), "exact")
    for i in range(p.b):
        lhs, rhs = float((u[i] * mv[i]).sum()), float((mu[i] * v[i]).sum())
        tol = 2.0 ** -24 * 64 * float((np.abs(u[i]) * mabs[i]).sum())
        print(f"{family} image {i}: <u,Mv> {lhs:.6f} <Mu,v> {rhs:.6f} gap {abs(lhs - rhs):.3e} tol {tol:.3e}")
        assert mv[i].any() and abs(lhs - rhs) <= tol


# ---- 4. flags and modes ---------------------------------------------------------------------------------------------------------------
def _stack(images):
    """A batch from (problem, image index, transforms or None) triples: the images' own arrays, side by side."""
    tfs = [p.tfs[i] if t is None else t for p, i, t in images]
    pick = lambda key: np.stack([getattr(p, key)[i] for p, i, _ in images])
    p0 = images[0][0]
    return SimpleNamespace(H=p0.H, W=p0.W, h=p0.h, w=p0.w, n=p0.n, b=len(images), tfs=tfs, x=pick("x"), y=pick("y"), resid=pick("resid"))


@functools.lru_cache(maxsize=None)
def _mixed():
    """Four images that take four ways through the gather: the 3 x 3 form, the counted loop, a window too wide (registered), one
    projective rotation (registered, and the non-affine form of the registered gather)."""
    rotations = T.problem(SHAPE, "rotations", N)
    proj = tuple(t.copy() for t in rotations.tfs[1])
    proj[0][2, 6] = 1e-3
    proj[2][:] = tf_ops.invert_transforms(proj[0])
    return _stack([(rotations, 0, None), (T.problem(SHAPE, "just_loop", N), 0, None), (T.problem(SHAPE, "too_wide", N), 0, None),
                   (rotations, 1, proj)])


def test_a_batch_whose_images_take_different_modes(dev):
    c = _mixed()
    tf = _dev_tfs(c.tfs)
    flags = _flags(tf)
    assert flags.dtype == np.int32 and flags.tolist() == [1, 1, 0, 0] == [A.exact_applies(*t[:3]) for t in c.tfs]
    assert [T.side(t[2]) for t in c.tfs[:3]] == ["fixed", "loop", "wide"]
    want = [A.data_grad_from_resid(c.resid[i], c.tfs[i], SHAPE[:2], 1.0, "exact") for i in (0, 1)]
    for chunk in T.CHUNKS:                                          # the running sum carried between chunks, image by image
        exact, reg = _grad(c.x, c.resid, tf, "exact", chunk=chunk), _grad(c.x, c.resid, tf, "registered", chunk=chunk)
        for i in (2, 3):
            assert exact[i].tobytes() == reg[i].tobytes() and reg[i].any(), (chunk, i)
        for i in (0, 1):
            _report(f"chunk={chunk} image {i}", exact[i], want[i])
            assert np.array_equal(exact[i], want[i]) and not np.array_equal(exact[i], reg[i]), (chunk, i)


def test_a_far_inverse_translation_takes_the_registered_statements(dev):
    p = T.problem(SHAPE, "far_shift", N)
    tf = _dev_tfs(p.tfs)
    assert _flags(tf).tolist() == [0] * p.b == [A.exact_applies(*t[:3]) for t in p.tfs]
    reg = _grad(p.x, p.resid, tf, "registered")
    assert _grad(p.x, p.resid, tf, "exact").tobytes() == reg.tobytes() and reg.any()


def test_either_side_of_the_decision_in_one_batch(dev):
    c = _stack([(T.problem(SHAPE, "just_fixed", N), 0, None), (T.problem(SHAPE, "just_loop", N), 0, None)])
    assert [T.side(t[2]) for t in c.tfs] == ["fixed", "loop"]
    tf = _dev_tfs(c.tfs)
    assert _flags(tf).tolist() == [1, 1]
    got = _grad(c.x, c.resid, tf, "exact")
    for i, family in enumerate(("just_fixed", "just_loop")):
        assert np.array_equal(got[i], _want(SHAPE, family, N)[0]), family


# ---- 5. form equivalence on the device ---------------------------------------------------------------------------------------------
def test_the_counted_loop_gives_the_values_of_the_3x3_form(dev):
    """A rotations image with one more copy, a zoom2 one whose residual is all zero: the image then runs on the counted loop
    and every value stays what the 3 x 3 form gave."""
    p = T.problem(SHAPE, "rotations", N)
    fixed = _grad(p.x, p.resid, _dev_tfs(p.tfs), "exact")
    more = [T.with_zero_copy(p, i) for i in range(p.b)]
    assert all(T.side(t[2]) == "loop" for t, _ in more) and all(T.side(t[2]) == "fixed" for t in p.tfs)
    tf = _dev_tfs([t for t, _ in more])
    assert _flags(tf).tolist() == [1] * p.b
    for chunk in (0, 3):
        looped = _grad(p.x, np.stack([r for _, r in more]), tf, "exact", chunk=chunk)
        _report(f"chunk={chunk}", looped, fixed)
        assert np.array_equal(looped, fixed) and fixed.any()          # by value: a zero's sign may differ


@pytest.mark.parametrize("family", ["rotations", "zoom2", "zoom5"])
def test_the_windows_extent_changes_no_value_on_the_device(dev, family):
    p = T.problem(SHAPE, family, N)
    want = _grad(p.x, p.resid, _dev_tfs(p.tfs), "exact")
    moved = [T.perturbed_inverses(t[2]) for t in p.tfs]
    for k in range(3):
        tfs = [(t[0], t[1], moved[i][k], t[3]) for i, t in enumerate(p.tfs)]
        tf = _dev_tfs(tfs)
        assert _flags(tf).tolist() == [1] * p.b
        got = _grad(p.x, p.resid, tf, "exact")
        _report(f"{family} perturbation {k}", got, want)
        assert np.array_equal(got, want) and want.any()


# ---- 6. the instantiations no suite launched ---------------------------------------------------------------------------------------
ITERS = 3
B6 = 2


def _p6(family):
    return T.problem(SHAPE, family, N, B6)


def _edge(dev):
    wy, wx = T.edge_weights(SHAPE, B6)
    return (wy, wx), tuple(torch.as_tensor(w).to(dev) for w in (wy, wx))


class _ExactWeighted(WTV.WeightedSuperresolution, A.ExactAdjoint):
    """tests/sr_wtv_ref's weighted-TV gradient with the data-term gradient swapped for the exact one."""

    def loss_and_grad_tf(self, target, samples, rot_tf, trans_tf, inv_rot_tf, inv_trans_tf):
        self._adj_forward = (np.asarray(rot_tf, np.float32), np.asarray(trans_tf, np.float32))
        return super().loss_and_grad_tf(target, samples, rot_tf, trans_tf, inv_rot_tf, inv_trans_tf)


@functools.lru_cache(maxsize=None)
def _amsgrad_restated(family):
    """[(x, m, v, vhat)] after each of ITERS AMSGrad iterations under weighted TV, all [B6, H, W]: tests/sr_update_ref.step fed
    with the restated gradient."""
    p = _p6(family)
    wy, wx = T.edge_weights(SHAPE, B6)
    opt, flag, c0, c1, c2, _ = RU.RULES["amsgrad"]
    alphas = _adam_alphas(ITERS, B6, lr=1e-2)
    per_image = []
    for i in range(B6):
        sr = _ExactWeighted(*LAM, num_aug=N, feature_size=SHAPE[2:], output_size=SHAPE[:2], wy=wy[i], wx=wx[i])
        smp = torch.from_numpy(p.y[i][..., None])
        x = p.x[i:i + 1].copy()
        m, v, vhat = (np.zeros_like(x) for _ in range(3))
        traj = []
        for it in range(ITERS):
            _, g = sr.loss_and_grad_tf(torch.from_numpy(x[..., None]), smp, *p.tfs[i])
            x, m, v, vhat = RU.step(opt, flag, c0, c1, c2, x, g.numpy()[..., 0], m, v, vhat, alphas[it, i:i + 1])
            traj.append((x, m, v, vhat))
        per_image.append(traj)
    return [tuple(np.concatenate([per_image[i][it][k] for i in range(B6)]) for k in range(4)) for it in range(ITERS)]


@pytest.mark.parametrize("family", T.FORM_FAMILIES)
def test_weighted_tv_one_step_and_solve_under_amsgrad(dev, family):
    from asr_amd import ops
    p = _p6(family)
    tf = _dev_tfs(p.tfs)
    _, wd = _edge(dev)
    want = _amsgrad_restated(family)
    alphas = _adam_alphas(ITERS, B6, lr=1e-2)
    xd, yd = ops.to_device(p.x), ops.to_device(p.y)
    slots = {k: torch.zeros_like(xd) for k in ("m", "v", "vhat")}
    q = ops.sr_forward_residual(xd, yd, tf[0], tf[1])
    x1, _ = ops.sr_backward(xd, q, tf[2], tf[3], LAM, _adam_cfg(), state=dict(slots, alphas=ops.to_device(alphas[0])), tv_weights=wd,
                            rot_tf=tf[0], trans_tf=tf[1], adjoint="exact")
    for what, got, w_ in zip(("x", "m", "v", "vhat"), (x1, slots["m"], slots["v"], slots["vhat"]), want[0]):
        _report(f"{family} one step {what}", got.cpu().numpy(), w_)
        assert np.array_equal(got.cpu().numpy(), w_), what
    plain, _ = ops.sr_backward(xd, q, tf[2], tf[3], LAM, _adam_cfg(), state=dict({k: torch.zeros_like(xd) for k in slots},
                               alphas=ops.to_device(alphas[0])), rot_tf=tf[0], trans_tf=tf[1], adjoint="exact")
    assert not torch.equal(plain, x1)                                   # the weights are in force
    for chunk in (0, 3):
        (x, _), st = _solve(p, tf, alphas, _adam_cfg(chunk), adjoint="exact", tv_weights=wd)
        for what, got, w_ in zip(("x", "m", "v", "vhat"), (x, st["m"], st["v"], st["vhat"]), want[-1]):
            _report(f"{family} solve chunk={chunk} {what}", got.cpu().numpy(), w_)
            assert np.array_equal(got.cpu().numpy(), w_), (chunk, what)


def _pd_taus(p, tf):
    from asr_amd import ops
    bound = ops.sr_data_bound(*tf, SHAPE[:2], SHAPE[2:], LAM[0], iters=6, adjoint="exact")
    return ops.pd_steps(bound, LAM[2], 1).cpu().numpy()[0]


@pytest.mark.parametrize("wtv", [False, True])
@pytest.mark.parametrize("family", T.FORM_FAMILIES)
def test_primal_dual_with_and_without_weighted_tv(dev, family, wtv):
    p = _p6(family)
    tf = _dev_tfs(p.tfs)
    (wy, wx), wd = _edge(dev) if wtv else ((None, None), None)
    pick = lambda a, i: None if a is None else a[i]
    taus = _pd_taus(p, tf)
    srs = [P.make_sr(LAM, N, SHAPE[2:], SHAPE[:2]) for _ in range(B6)]
    x, py, px = p.x.copy(), np.zeros_like(p.x), np.zeros_like(p.x)
    for _ in range(ITERS):
        new = [P.pd_update(srs[i], x[i], py[i], px[i], A.data_grad(srs[i], x[i], p.y[i], p.tfs[i], "exact"), taus[i], wy=pick(wy, i),
                           wx=pick(wx, i)) for i in range(B6)]
        x, py, px = (np.stack([s[k] for s in new]) for k in range(3))
    for chunk in (0, 3):
        (gx, _), st = _solve(p, tf, np.tile(taus[None], (ITERS, 1)), _pd_cfg(chunk), adjoint="exact", tv_weights=wd)
        for what, got, w_ in zip(("x", "p_y", "p_x"), (gx, st["m"], st["v"]), (x, py, px)):
            _report(f"{family} chunk={chunk} {what}", got.cpu().numpy(), w_)
            assert np.array_equal(got.cpu().numpy(), w_), (chunk, what)
    (other, _), _ = _solve(p, tf, np.tile(taus[None], (ITERS, 1)), _pd_cfg(), adjoint="exact", tv_weights=None if wtv else _edge(dev)[1])
    assert not np.array_equal(other.cpu().numpy(), x)                   # the weights are in force, or are not


def _rule(rule, p, tf, iters):
    """(cfg, alphas [iters, B6]) of a monitored case's rule."""
    from asr_amd import _lib, ops
    if rule == "pd":
        return _pd_cfg(), np.tile(_pd_taus(p, tf)[None], (iters, 1))
    if rule == "sgd":
        return ops.sr_config(_lib.OPT_SGD), np.full((iters, B6), 1e-2, np.float32)
    return _adam_cfg(), _adam_alphas(iters, B6, lr=1e-2)


SLOTS = {"adam": ("m", "v", "vhat"), "sgd": (), "pd": ("m", "v")}


@pytest.mark.parametrize("case", [c for c in T.MONITORED if c.monitor == "trace"], ids=lambda c: f"{c.family}-{c.rule}-wtv{int(c.wtv)}")
def test_a_monitor_that_never_stops_returns_the_unmonitored_bytes(dev, case):
    p = _p6(case.family)
    tf = _dev_tfs(p.tfs)
    kw = dict(adjoint="exact", tv_weights=_edge(dev)[1] if case.wtv else None)
    iters = 4
    cfg, alphas = _rule(case.rule, p, tf, iters)
    mon = dict(every=1, rel_tol=0.0, patience=0, min_iter=0, history=True)
    (x, _, trace), st = _solve(p, tf, alphas, cfg, monitor=mon, **kw)
    (want, _), ws = _solve(p, tf, alphas, cfg, **kw)
    assert trace.iters_done.cpu().numpy().tolist() == [iters] * B6
    assert torch.equal(x, want) and not torch.equal(x, torch.as_tensor(p.x).to(x.device))
    for k in SLOTS[case.rule]:
        assert torch.equal(st[k], ws[k]) and bool(st[k].any()), k


@pytest.mark.parametrize("case", [c for c in T.MONITORED if c.monitor == "stop"], ids=lambda c: f"{c.family}-{c.rule}-wtv{int(c.wtv)}")
def test_a_frozen_image_is_the_solve_cut_there(dev, case):
    p = _p6(case.family)
    tf = _dev_tfs(p.tfs)
    kw = dict(adjoint="exact", tv_weights=_edge(dev)[1] if case.wtv else None)
    iters = 6
    cfg, alphas = _rule(case.rule, p, tf, iters)
    alphas = alphas.copy()
    alphas[:, 0] = 1e-7                                                 # image 0 all but stands still: it stalls at once
    mon = dict(every=1, rel_tol=1e-3, patience=2, min_iter=0, history=True)
    (x, _, trace), st = _solve(p, tf, alphas, cfg, monitor=mon, **kw)
    done = trace.iters_done.cpu().numpy()
    print(case, "iters_done", done.tolist())
    assert done[0] == 2 and done[0] < done[1] <= iters
    for i in range(B6):
        (cx, _), cs = _solve(p, tf, alphas[:done[i]], cfg, **kw)
        assert torch.equal(x[i], cx[i]), i
        for k in SLOTS[case.rule]:
            assert torch.equal(st[k][i], cs[k][i]), (i, k)


@pytest.mark.parametrize("family", T.FORM_FAMILIES)
def test_the_exact_bound_is_above_the_largest_eigenvalue_on_either_form(dev, family):
    from asr_amd import ops
    H, W, h, w = SHAPE
    p = _p6(family)
    tf = _dev_tfs(p.tfs)
    lam_max = [float(np.linalg.eigvalsh(2.0 * (Am.T @ Am))[-1]) for Am in (_dense_forward(SHAPE, family, N, i, B6) for i in range(B6))]
    last = None
    for k in (1, 6, 64):
        got = ops.sr_data_bound(*tf, (H, W), (h, w), 1.0, iters=k, adjoint="exact").cpu().numpy()
        print(f"{family} iters={k}: bound {got.tolist()} largest eigenvalue {lam_max}")
        for i in range(B6):
            assert got[i] >= (1.0 - 1e-5) * lam_max[i]
        assert last is None or (got <= last).all()
        last = got
    chunked = ops.sr_data_bound(*tf, (H, W), (h, w), 1.0, iters=6, adjoint="exact", cfg=ops.sr_config(plane_chunk=3)).cpu().numpy()
    assert chunked.tobytes() == ops.sr_data_bound(*tf, (H, W), (h, w), 1.0, iters=6, adjoint="exact").cpu().numpy().tobytes()


# ---- 7. Huber with per-measurement weights ------------------------------------------------------------------------------------------
def test_huber_with_weights_under_the_exact_form_on_sheared_copies(dev):
    from asr_amd import _lib, ops
    H, W, h, w = SHAPE
    p = _p6("aniso_shear")
    tf = _dev_tfs(p.tfs)
    rng = np.random.default_rng(7)
    wts = rng.random((B6, N, h, w), dtype=np.float32)
    wts[rng.random(wts.shape) < 0.05] = 0.0
    wts[rng.random(wts.shape) < 0.05] = 1.0
    delta = 0.1
    srs = [P.make_sr(LAM_DF, N, (h, w), (H, W), df_loss="huber", df_delta=delta, weights=wts[i]) for i in range(B6)]
    cfg = ops.sr_config(_lib.OPT_SGD)
    alpha = np.full(B6, 0.05, np.float32)
    x, yd, wd = p.x.copy(), ops.to_device(p.y), ops.to_device(wts)
    for it in range(3):
        xd = ops.to_device(x)
        q, raw = ops.sr_forward_residual(xd, yd, tf[0], tf[1], data_term=("huber", delta), weights=wd, want_raw=True)
        assert float((raw.abs() > delta).float().mean()) > 0.2 and float((raw.abs() < delta).float().mean()) > 0.02      # both branches
        x_new, g = ops.sr_backward(xd, q, tf[2], tf[3], LAM_DF, cfg, state=dict(m=None, v=None, vhat=None, alphas=ops.to_device(alpha)),
                                   want_grad=True, rot_tf=tf[0], trans_tf=tf[1], adjoint="exact")
        want_g = np.stack([A.data_grad(srs[i], x[i], p.y[i], p.tfs[i], "exact") for i in range(B6)])
        _report(f"step {it} gradient", g.cpu().numpy(), want_g)
        assert np.array_equal(g.cpu().numpy(), want_g) and want_g.any()
        x = RU.step(RU.OPT_SGD, 0, 0, 0, 0, x, want_g, None, None, None, alpha)[0]
        assert np.array_equal(x_new.cpu().numpy(), x), it
    plain = np.stack([A.data_grad(P.make_sr(LAM_DF, N, (h, w), (H, W)), p.x[i], p.y[i], p.tfs[i], "exact") for i in range(B6)])
    first = np.stack([A.data_grad(srs[i], p.x[i], p.y[i], p.tfs[i], "exact") for i in range(B6)])
    assert not np.array_equal(plain, first)                                 # the data term is in force
