"""GPU: the SR solver's data term (include/asr_hip.h, "data term": L1, Huber, per-measurement weights) and the confidence
kernel that makes its weights, against the restatement of tests/sr_dt_ref.py and against the kernels that were there before."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import sr as o_sr
from test_gpu_sr_wtv import _adam_alphas, _adam_cfg, _problem, _random_weights, _tfs, B1, B2, EPS

import sr_dt_ref as R

pytestmark = pytest.mark.gpu

DELTA = 0.1
D32 = np.float32(DELTA)
TERMS = ("l2", "l1", ("huber", DELTA))
SHAPES = [(64, 64, 16, 16, 5), (64, 64, 32, 32, 3), (48, 80, 12, 20, 4), (2, 2, 1, 1, 2), (128, 128, 32, 32, 4)]
BATCH = 2


def _name(dt):
    return dt if isinstance(dt, str) else dt[0]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _neighbours(v):
    return np.nextafter(v, np.float32(np.inf), dtype=np.float32), np.nextafter(v, np.float32(-np.inf), dtype=np.float32)


def _weights_for(mode, shape, dev, seed=31):
    """None / [n,h,w] shared / [b,n,h,w], in [0, 1] with exact zeros and ones -> (numpy broadcastable to [b,n,h,w] | None, device)."""
    if mode == "none":
        return None, None
    full = shape if mode == "batch" else shape[1:]
    (w, _), (wd, _) = _random_weights(seed, full, dev)
    assert (w == 0).any() and (w == 1).any() or w.size < 8
    return w, wd.contiguous()


def _arranged(dev, H, W, h, w, n):
    """x, y, transforms of one shape with y arranged so that the residual r = D - y holds +0, +-delta and the float32
    neighbours of +-delta exactly (where D, the forward model's output, allows it: y = D - t is tried with its two float32
    neighbours and kept where D - y IS t), on top of an ordinary residual everywhere else.  -0 needs D = -0, which the
    forward model's last statement top + (bot - top) * 0.5 yields only for tl = -0 and trv = bl = br = the negative
    denormal: the 2 x 2 shape carries exactly that x for image 0 (identity transforms there)."""
    from asr_amd import ops, transforms as T
    tiny = (H, W) == (2, 2)
    y0, angs, shs = _problem(41, BATCH, n, H, W, h, w)
    if tiny:
        angs, shs = np.zeros_like(angs), np.zeros_like(shs)
    rot, tr, irot, itr = _tfs(angs, shs, H, W)
    if (H, W) == (128, 128):                     # one genuinely projective rotation: the generic path of the kernel
        r = T.rotation_transforms(angs.reshape(-1), H, W).reshape(BATCH, n, 8)
        r[1, 2, 6:] = [1e-4, -2e-4]
        rot = ops.to_device(r)
        irot = ops.to_device(np.stack([T.inverse_transforms(r[i]) for i in range(BATCH)]))
    rng = np.random.default_rng(42)
    x = ops.sr_init_target(ops.to_device(y0), (H, W)).cpu().numpy()
    x[:, :, : W // 2] += 0.05 * rng.standard_normal((BATCH, H, W // 2)).astype(np.float32)      # the right half keeps exact zeros
    if tiny:
        d = np.float32(-1e-45)
        x[0] = np.array([[-0.0, d], [d, d]], np.float32)
    xd = ops.to_device(x)
    D = ops.sr_forward_residual(xd, torch.zeros((BATCH, n, h, w), device=dev), rot, tr).cpu().numpy()   # r = D - 0 = D
    y = y0.copy()
    flat_D, flat_y = D.reshape(-1), y.reshape(-1)
    up, dn = _neighbours(D32)
    nup, ndn = _neighbours(-D32)
    targets = [np.float32(0.0), D32, -D32, up, dn, nup, ndn]
    made = set()
    if tiny:
        flat_y[0] = 0.0                                       # image 0, copy 0: r = (-0) - (+0) = -0
        flat_y[1] = flat_D[1]                                 # image 0, copy 1: r = D - D = +0
        return xd, ops.to_device(y), (rot, tr, irot, itr), made, targets
    order = np.argsort(np.abs(flat_D), kind="stable")        # D = 0 first: there y = -t is exact
    pos = 0
    for t in targets:                                         # three elements per target, each element used once
        hits = 0
        while hits < 3 and pos < flat_D.size:
            p = order[pos]
            pos += 1
            c0 = np.float32(flat_D[p] - t)
            for c in (c0,) + _neighbours(c0):
                if np.float32(flat_D[p] - c) == t:
                    flat_y[p] = c
                    hits += 1
                    made.add(float(t))
                    break
    return xd, ops.to_device(y), (rot, tr, irot, itr), made, targets


@pytest.fixture(scope="module")
def cases(dev):
    return {}


def _case(cases, dev, shape):
    if shape not in cases:
        cases[shape] = _arranged(dev, *shape)
    return cases[shape]


# ---- 1. + 2. the forward kernel's two outputs and the loss term ---------------------------------------------------------------------
@pytest.mark.parametrize("H,W,h,w,n", SHAPES)
def test_q_and_r_and_the_loss_term(dev, cases, H, W, h, w, n):
    from asr_amd import ops
    xd, yd, (rot, tr, _, _), made, targets = _case(cases, dev, (H, W, h, w, n))
    r_plain = ops.sr_forward_residual(xd, yd, rot, tr)
    r_np = r_plain.cpu().numpy()
    if (H, W) == (2, 2):
        assert r_np.reshape(-1)[0] == 0 and np.signbit(r_np.reshape(-1)[0]), "the arrangement must give r = -0"
        assert ((r_np == 0) & ~np.signbit(r_np)).any()
    else:
        assert made == {float(t) for t in targets}, made
        for t in targets:
            assert (r_np == t).any(), t
        assert ((r_np == 0) & ~np.signbit(r_np)).any()
    t_plain = ops.sr_loss_terms(xd, r_plain).cpu().numpy()
    for mode in ("none", "shared", "batch"):
        w_np, w_dev = _weights_for(mode, (BATCH, n, h, w), dev)
        for dt in TERMS:
            loss = _name(dt)
            q, r = ops.sr_forward_residual(xd, yd, rot, tr, data_term=dt, weights=w_dev, want_raw=True)
            if mode == "none" and loss == "l2":
                assert q is r                                                  # the call that ran before: nothing new launched
            assert np.array_equal(_bits(r.cpu().numpy()), _bits(r_np)), (mode, loss)
            want = R.weighted_psi(r_np, loss, DELTA, w_np)
            assert np.array_equal(_bits(q.cpu().numpy()), _bits(want)), (mode, loss)
            q_only = ops.sr_forward_residual(xd, yd, rot, tr, data_term=dt, weights=w_dev)
            assert torch.equal(q_only, q)
            # 2. the loss term: <= 4 float32 roundings per non-negative term, 4 * 2^-24 = 2.4e-7 relative
            terms = ops.sr_loss_terms(xd, r, data_term=dt, weights=w_dev).cpu().numpy()
            wb = None if w_np is None else np.broadcast_to(w_np, r_np.shape)
            for b in range(BATCH):
                ref = R.data_term64(r_np[b], loss, DELTA, None if wb is None else wb[b])
                print(f"{(H, W, h, w, n)} {mode:6s} {loss:5s} image {b}: df {terms[b, 0]:.9g} ref {ref:.9g}")
                assert abs(terms[b, 0] - ref) <= 1e-6 * abs(ref), (mode, loss, b, terms[b, 0], ref)
            np.testing.assert_allclose(terms[:, 1:], t_plain[:, 1:], rtol=1e-12)


def test_huber_at_least_as_wide_as_the_residual_and_unit_weights_are_l2(dev, cases):
    from asr_amd import ops
    H, W, h, w, n = SHAPES[0]
    xd, yd, (rot, tr, _, _), _, _ = _case(cases, dev, SHAPES[0])
    r = ops.sr_forward_residual(xd, yd, rot, tr)
    big = float(r.abs().max())
    ones = torch.ones((n, h, w), device=dev)
    for dt, wts in ((("huber", big), None), ("l2", ones), (("huber", big), ones), (("huber", 1e30), ones[None].repeat(BATCH, 1, 1, 1))):
        q = ops.sr_forward_residual(xd, yd, rot, tr, data_term=dt, weights=wts)
        assert np.array_equal(_bits(q.cpu().numpy()), _bits(r.cpu().numpy())), dt
        np.testing.assert_allclose(ops.sr_loss_terms(xd, r, data_term=dt, weights=wts).cpu().numpy(),
                                   ops.sr_loss_terms(xd, r).cpu().numpy(), rtol=1e-12)
    assert not torch.equal(ops.sr_forward_residual(xd, yd, rot, tr, data_term=("huber", 0.5 * big)), r)


# ---- 3. the gradient ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,h,w,n", SHAPES[:3])
def test_gradient_matches_the_restatement_on_the_devices_own_residual(dev, cases, H, W, h, w, n):
    """psi and w in numpy on the device's r (a 1-ulp difference in r may flip a sign under L1), then the oracle's
    data_grad_copies_tf summed in copy order, against the existing backward kernel fed q; lambda_tv = l2 = l1 = 0, so the
    gradient is the data term's alone.  atol 2e-5: test_sr_forward_and_gradient_match_oracle's."""
    from asr_amd import ops
    xd, yd, (rot, tr, irot, itr), _, _ = _case(cases, dev, (H, W, h, w, n))
    lam = (1.3, 0.0, 0.0, 0.0)
    sr = o_sr.Superresolution(*lam, num_aug=n, feature_size=(h, w), output_size=(H, W))
    w_np, w_dev = _weights_for("batch", (BATCH, n, h, w), dev)
    for dt, (wn, wd) in ((("huber", DELTA), (w_np, w_dev)), ("l1", (None, None)), ("l1", (w_np, w_dev)), (("huber", DELTA), (None, None))):
        q, r = ops.sr_forward_residual(xd, yd, rot, tr, data_term=dt, weights=wd, want_raw=True)
        grad = ops.sr_backward(xd, q, irot, itr, lam, _adam_cfg())[1].cpu().numpy()
        q_np = R.weighted_psi(r.cpu().numpy(), _name(dt), DELTA, wn)
        for b in range(BATCH):
            g = sr.data_grad_copies_tf(torch.from_numpy(np.ascontiguousarray(q_np[b][..., None])), irot[b].cpu().numpy(),
                                       itr[b].cpu().numpy())
            ref = torch.zeros_like(g[0])
            for i in range(n):
                ref += g[i]
            err = float(np.abs(grad[b] - ref.numpy()[:, :, 0]).max())
            print(f"{(H, W, h, w, n)} {_name(dt)} weights={wn is not None} image {b}: max |grad - ref| = {err:.3e}")
            np.testing.assert_allclose(grad[b], ref.numpy()[:, :, 0], rtol=0, atol=2e-5)


# ---- 4. the solve is its explicit steps ---------------------------------------------------------------------------------------------------
def _solve_dt_raw(x, y, tfs, alphas, lam, cfg, dt, state):
    """asr_sr_solve_dt_f32 itself (ops.sr_solve routes L2 without weights to the call that ran before)."""
    from asr_amd import _lib, ops
    from asr_amd._lib import call, ptr, stream_ptr
    b, n, H, W, h, w = ops._sr_dims(x, y)
    nbytes = _lib.load().asr_sr_solve_workspace_bytes_dt(b, n, H, W, h, w, C.byref(cfg))
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=x.device)
    terms = torch.zeros((b, 4), dtype=torch.float64, device=x.device)
    call("asr_sr_solve_dt_f32", ptr(x), ptr(y), *(ptr(t) for t in tfs), ptr(state["m"]), ptr(state["v"]), ptr(state["vhat"]),
         ptr(alphas), alphas.shape[0], ptr(terms, torch.float64), ptr(ws), C.c_size_t(nbytes), b, n, H, W, h, w,
         *(float(v) for v in lam), C.byref(cfg), C.byref(dt), stream_ptr())
    return x, terms


@pytest.mark.parametrize("kind", ["amsgrad", "adagrad"])
def test_three_iterations_are_three_explicit_steps(dev, kind):
    from asr_amd import _lib, ops
    H, h, n, b, iters = 64, 16, 5, 2, 3
    y, angs, shs = _problem(51, b, n, H, H, h, h)
    rot, tr, irot, itr = _tfs(angs, shs, H, H)
    yd = ops.to_device(y)
    lam = (1.0, 0.3, 0.7, 0.05)
    if kind == "amsgrad":
        make_cfg, init, alphas = _adam_cfg, {}, _adam_alphas(iters, b, lr=1e-2)
    else:
        make_cfg = lambda chunk=0: ops.sr_config(_lib.OPT_ADAGRAD, c2=1e-7, plane_chunk=chunk)
        init, alphas = {"v": 0.1}, np.full((iters, b), 1e-2, np.float32)
    ad = ops.to_device(alphas)
    slots = ("m", "v", "vhat") if kind == "amsgrad" else ("v",)
    _, w_shared = _weights_for("shared", (b, n, h, h), dev)
    _, w_batch = _weights_for("batch", (b, n, h, h), dev, seed=33)
    _, tvw = _random_weights(35, (H, H), dev)
    for dt, wts in (("l1", w_shared), (("huber", DELTA), w_batch), ("l1", None), ("l2", w_batch)):
        for tv in (None, tvw):
            # the explicit steps: forward under the data term, the backward kernel that was there before
            xd = ops.sr_init_target(yd, (H, H))
            st = {k: torch.full_like(xd, float(init.get(k, 0.0))) for k in ("m", "v", "vhat")}
            for it in range(iters):
                q = ops.sr_forward_residual(xd, yd, rot, tr, data_term=dt, weights=wts)
                xd, _ = ops.sr_backward(xd, q, irot, itr, lam, make_cfg(), state=dict(st, alphas=ops.to_device(alphas[it])),
                                        tv_weights=tv)
            for chunk in (0, 1, 2):
                for cuts in ((iters,), (1, 2)):
                    state, x, first = {}, ops.sr_init_target(yd, (H, H)), 0
                    for c in cuts:
                        x, terms = ops.sr_solve(x, yd, rot, tr, irot, itr, ad[first:first + c].contiguous(), lam, cfg=make_cfg(chunk),
                                                slot_init=init, state=state, tv_weights=tv, data_term=dt, weights=wts)
                        first += c
                    tag = (kind, _name(dt), wts is not None, tv is not None, chunk, cuts)
                    assert torch.equal(x, xd), tag
                    for k in slots:
                        assert torch.equal(state[k], st[k]), tag + (k,)
            # the loss terms of the last iteration: evaluated before its update, on the raw residual
            x2 = ops.sr_init_target(yd, (H, H))
            state = {}
            ops.sr_solve(x2, yd, rot, tr, irot, itr, ad[:iters - 1].contiguous(), lam, cfg=make_cfg(), slot_init=init, state=state,
                         tv_weights=tv, data_term=dt, weights=wts)
            _, r = ops.sr_forward_residual(x2, yd, rot, tr, data_term=dt, weights=wts, want_raw=True)
            want = ops.sr_loss_terms(x2, r, make_cfg(), tv_weights=tv, data_term=dt, weights=wts).cpu().numpy()
            np.testing.assert_allclose(terms.cpu().numpy(), want, rtol=1e-12)


def test_l2_without_weights_through_the_new_entry_point_is_the_old_solve(dev):
    from asr_amd import _lib, ops
    H, h, n, b, iters = 64, 16, 5, 2, 3
    y, angs, shs = _problem(53, b, n, H, H, h, h)
    tfs = _tfs(angs, shs, H, H)
    yd = ops.to_device(y)
    lam = (1.0, 0.3, 0.7, 0.05)
    ad = ops.to_device(_adam_alphas(iters, b, lr=1e-2))
    for chunk in (0, 2):
        cfg = _adam_cfg(chunk)
        old_state = {}
        x_old, t_old = ops.sr_solve(ops.sr_init_target(yd, (H, H)), yd, *tfs, ad, lam, cfg=cfg, state=old_state)
        x = ops.sr_init_target(yd, (H, H))
        st = {k: torch.zeros_like(x) for k in ("m", "v", "vhat")}
        x_new, t_new = _solve_dt_raw(x, yd, tfs, ad, lam, cfg, _lib.SrDataTerm(_lib.DF_L2, 0.0, None, 0, None, None, 0), st)
        assert torch.equal(x_new, x_old)
        for k in ("m", "v", "vhat"):
            assert torch.equal(st[k], old_state[k]), k
        np.testing.assert_allclose(t_new.cpu().numpy(), t_old.cpu().numpy(), rtol=1e-12)
    # and ops makes the old call for it
    same, _ = ops.sr_solve(ops.sr_init_target(yd, (H, H)), yd, *tfs, ad, lam, cfg=_adam_cfg(), data_term="l2", weights=None)
    assert torch.equal(same, x_old)


# ---- 5. trajectory ------------------------------------------------------------------------------------------------------------
def test_huber_trajectory_matches_the_restatement(dev):
    """test_sr_solve_trajectory_matches_oracle under Huber (delta 0.1) with shared weights: 10 AMSGrad iterations, two images
    under the persistent step counter, the same bounds.  (L1's sign makes single pixels chaotic: no trajectory bound.)"""
    from asr_amd import ops, transforms as T
    from oracle import augment as o_aug
    H, h, n, b, iters = 128, 32, 6, 2, 10
    y, angs, shs = _problem(5, b, n, H, H, h, h)
    lam = (1.0, 0.3, 0.7, 0.0)
    rot, tr, irot, itr = _tfs(angs, shs, H, H)
    yd = ops.to_device(y)
    w_np, w_dev = _weights_for("shared", (b, n, h, h), dev, seed=37)
    alphas = np.zeros((iters, b), np.float32)
    for i in range(b):
        for it in range(iters):
            alphas[it, i] = T.adam_alpha(T.exponential_decay_lr(1e-3, 60, 0.3, it), B1, B2, i * iters + it + 1)
    xd, terms = ops.sr_solve(ops.sr_init_target(yd, (H, H)), yd, rot, tr, irot, itr, ops.to_device(alphas), lam,
                             np.float32(1) - B1, np.float32(1) - B2, EPS, True, data_term=("huber", DELTA), weights=w_dev)
    got = xd.cpu().numpy()
    opt = o_sr.Optimizer("adam", 1e-3, amsgrad=True, lr_scheduler=True, decay_steps=60, decay_rate=0.3)
    for i in range(b):
        ref_sr = R.DataTermSuperresolution(*lam, num_iter=iters, num_aug=n, optimizer=opt, feature_size=(h, h), output_size=(H, H),
                                           df_loss="huber", df_delta=DELTA, weights=w_np)
        ref, loss = ref_sr.augmented_superresolution(y[i][..., None], angs[i], shs[i])
        d = np.abs(got[i] - ref[:, :, 0])
        m_got = o_sr.threshold_image(got[i], 1, th_factor=0.2)
        m_ref = o_sr.threshold_image(ref[:, :, 0], 1, th_factor=0.2)
        iou = o_aug.single_class_IOU(m_ref, m_got, 1, False)
        print(f"image {i}: mean |d| {d.mean():.3e}  max |d| {d.max():.3e}  mask IoU {iou:.6f}")
        assert d.mean() < 1e-5, d.mean()
        assert d.max() < 5e-3, d.max()
        assert iou >= 0.999
        t = terms[i].cpu().numpy()
        assert abs(lam[0] * t[0] + lam[1] * t[1] + lam[2] * t[2] - loss) <= 1e-4 * abs(loss)


# ---- 6. what it is for --------------------------------------------------------------------------------------------------------
def test_the_construction_huber_and_l1_beat_l2_on_every_seed(dev):
    """sr_dt_ref.make_case on seeds 0..7, solved on the device: 150 AMSGrad iterations, lr 1e-2, lambda = (1, 0.05, 0, 0)."""
    from asr_amd import ops, transforms as T
    seeds = list(range(8))
    made = [R.make_case(s) for s in seeds]
    H, h = R.H_HR, R.H_LR
    y = np.stack([c["copies"] for c in made])
    angs, shs = np.stack([c["angles"] for c in made]), np.stack([c["shifts"] for c in made])
    rot, tr, irot, itr = _tfs(angs, shs, H, H)
    yd = ops.to_device(y)
    alphas = np.zeros((R.ITERS, len(seeds)), np.float32)
    for it in range(R.ITERS):
        alphas[it, :] = T.adam_alpha(np.float32(R.LR), B1, B2, it + 1)
    ad = ops.to_device(alphas)
    ious = {}
    for dt in TERMS:
        x, _ = ops.sr_solve(ops.sr_init_target(yd, (H, H)), yd, rot, tr, irot, itr, ad, R.LAMBDAS, np.float32(1) - B1,
                            np.float32(1) - B2, EPS, True, want_loss=False, data_term=dt)
        ious[_name(dt)] = [R.iou(x[i].cpu().numpy(), made[i]["truth"]) for i in range(len(seeds))]
    for i, s in enumerate(seeds):
        print(f"seed {s}: IoU L2 {ious['l2'][i]:.3f}  Huber(0.1) {ious['huber'][i]:.3f}  L1 {ious['l1'][i]:.3f}")
    for i, s in enumerate(seeds):
        assert ious["huber"][i] > ious["l2"][i], (s, ious["l2"][i], ious["huber"][i])
        assert ious["l1"][i] > ious["l2"][i], (s, ious["l2"][i], ious["l1"][i])


# ---- 7. the confidence kernel -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("classes", [1, 2, 21, 40])                           # 40 > kMaxStageClasses = 32: rows straight from memory
@pytest.mark.parametrize("pixels", [1, 255, 257, 2048 * 256 + 1])             # one beyond a grid stride of 2048 workgroups
def test_confidence_is_the_softmax_kernels_top_entries(dev, classes, pixels):
    from asr_amd import ops
    g = torch.Generator(dev).manual_seed(100 * classes + pixels % 97)
    logits = 4.0 * torch.randn((pixels, classes), device=dev, generator=g)
    ties = torch.randint(-2, 3, (pixels, classes), device=dev, generator=g).to(torch.float32)      # few values: ties for the maximum
    pick = torch.rand((pixels, 1), device=dev, generator=g) < 0.5
    logits = torch.where(pick, ties, logits).contiguous()
    sm = ops.class_activation(logits, "softmax")
    maxprob = ops.opm_confidence(logits, "maxprob")
    margin = ops.opm_confidence(logits, "margin")
    assert maxprob.shape == (pixels,) and margin.shape == (pixels,)
    if classes == 1:
        assert torch.equal(maxprob, torch.ones_like(maxprob)) and torch.equal(margin, torch.ones_like(margin))
        return
    top = torch.topk(sm, 2, dim=-1).values
    assert torch.equal(maxprob, top[:, 0].contiguous())
    assert torch.equal(margin, (top[:, 0] - top[:, 1]).contiguous())
    tied = (torch.topk(logits, 2, dim=-1).values.diff(dim=-1)[:, 0] == 0)
    assert torch.equal(margin[tied], torch.zeros_like(margin[tied]))
    if pixels > 1:
        assert bool(tied.any()) and not bool(tied.all())
    # leading dimensions and an out= slice, as the label-map path calls it
    if pixels == 257:
        out = torch.full((3, pixels), -1.0, device=dev)
        ops.opm_confidence(logits.view(1, pixels, classes), "margin", out=out[1:2])
        assert torch.equal(out[1], margin) and bool((out[0] == -1).all()) and bool((out[2] == -1).all())
