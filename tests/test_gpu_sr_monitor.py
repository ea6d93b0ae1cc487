"""The convergence monitor on the device (include/asr_hip.h, "convergence monitor"; asr_sr_solve_mon_f32 through
ops.sr_solve(monitor=...)): every loss term against an exact host sum of its float32 summands, the trace's reproducibility
(call to call, alone or in a batch, for any plane chunking), trace-only solves against the unmonitored solve bit for bit, and
the stop rule against its restatement tests/sr_mon_ref.py, with every stopped image compared bit for bit with the plain solve cut
at its iteration."""
import numpy as np
import pytest
import torch

from oracle import sr as o_sr
from oracle import tf_ops
from test_gpu_warp_sr import _angles_shifts, _blob_masks
from test_gpu_sr_wtv import LAM, B1, B2, EPS, _adam_alphas, _adam_cfg, _problem, _random_weights, _tfs

import sr_mon_ref as M

pytestmark = pytest.mark.gpu

SHAPES = [(64, 64, 16, 16, 5), (48, 80, 12, 20, 4), (2, 2, 1, 1, 2)]
BATCH = 3
TRACE_ONLY = dict(every=1, rel_tol=0.0, patience=0, min_iter=0, history=True)
# two float64 sums of the same N summands >= 0, each in some order: each within (N - 1) * 2^-53 of the exact sum, so within
# twice that of each other; N <= 64 * 64 * 15, the bilateral-TV summands of the largest image here
TWO_ORDERS = 2 * (64 * 64 * 15) * 2.0 ** -53


def _setup(seed, H, W, h, w, n, b=BATCH, noise=0.05):
    """A batch of problems on the device with a perturbed start, so that no term is trivial."""
    from asr_amd import ops
    y, angs, shs = _problem(seed, b, n, H, W, h, w)
    y = (y + 0.1 * np.random.default_rng(seed + 1).random(y.shape, dtype=np.float32)).astype(np.float32)
    tfs = _tfs(angs, shs, H, W)
    yd = ops.to_device(y)
    x0 = ops.sr_init_target(yd, (H, W)).cpu().numpy() + noise * np.random.default_rng(seed + 2).standard_normal((b, H, W)).astype(np.float32)
    return y, yd, x0.astype(np.float32), tfs


def _solve(x0, yd, tfs, alphas, lam=LAM, cfg=None, monitor=None, sel=None, **kw):
    """ops.sr_solve from the host start x0 -> (x, m, v, vhat, terms, trace) as host arrays / the trace; sel: the images."""
    from asr_amd import ops
    pick = (lambda t: t) if sel is None else (lambda t: t[sel].contiguous())
    for k in ("weights",):
        if kw.get(k) is not None and kw[k].dim() == 4:
            kw[k] = pick(kw[k])
    if kw.get("tv_weights") is not None and kw["tv_weights"][0].dim() == 3:
        kw["tv_weights"] = tuple(pick(t) for t in kw["tv_weights"])
    a = alphas if sel is None else alphas[:, sel]
    state = {}
    out = ops.sr_solve(pick(ops.to_device(x0)), pick(yd), *[pick(t) for t in tfs], ops.to_device(np.ascontiguousarray(a)), lam,
                       cfg=cfg if cfg is not None else _adam_cfg(), state=state, monitor=monitor, **kw)
    arrs = [out[0].cpu().numpy()] + [state[k].cpu().numpy() for k in ("m", "v", "vhat")]
    return arrs, out[1].cpu().numpy(), (out[2] if monitor is not None else None)


# ---- 1. the loss terms against an exact sum of their float32 summands -------------------------------------------------------------
def _check_terms(got, x, r, loss, delta, wts, prior, lam_case):
    """got [4] against math.fsum of the summands; every summand is >= 0, so ANY order of adding N of them in float64 is within
    (N - 1) * 2^-53 relative of the exact sum."""
    if prior[0] == "btv":
        tv = M.btv_summands(x, prior[1], prior[2])
    elif prior[0] == "wtv":
        tv = M.tv_summands(x, prior[1], prior[2])
    else:
        tv = M.tv_summands(x)
    for k, summands in enumerate((M.rho32(r, loss, delta, wts), tv, M.l2_summands(x), M.l1_summands(x))):
        want, count = M.exact_sum(summands)
        assert np.all(np.asarray(summands) >= 0)
        tol = (count - 1) * 2.0 ** -53 * want
        print(f"{lam_case} term {k}: got {got[k]!r} exact {want!r} |diff| {abs(got[k] - want):.3e} tol {tol:.3e} (N = {count})")
        assert abs(got[k] - want) <= tol, (lam_case, k, got[k], want, tol)


@pytest.mark.parametrize("H,W,h,w,n", SHAPES)
def test_loss_terms_match_an_exact_host_sum(dev, H, W, h, w, n):
    from asr_amd import ops
    y, yd, x0, tfs = _setup(7, H, W, h, w, n)
    rot, tr = tfs[0], tfs[1]
    alphas = _adam_alphas(1, BATCH)
    wts_np = np.random.default_rng(8).random((BATCH, n, h, w), dtype=np.float32)
    wts_np[0, 0] = 0.0
    wts = torch.as_tensor(wts_np).to(dev)
    (wy, wx), tvw = _random_weights(9, (BATCH, H, W), dev)
    big = np.float32(np.abs(ops.sr_forward_residual(ops.to_device(x0), yd, rot, tr).cpu().numpy()).max())
    cases = []
    for loss, delta in (("l2", 0.1), ("l1", 0.1), ("huber", float(0.3 * big))):
        for weighted in (False, True):
            cases.append((loss, delta, weighted, ("tv",)))
    cases += [("l2", 0.1, False, ("btv", 0.6, 2)), ("huber", float(0.3 * big), True, ("wtv",)), ("l1", 0.1, False, ("wtv",)),
              ("l2", 0.1, True, ("btv", 0.7, 1))]
    for loss, delta, weighted, prior in cases:
        from asr_amd import _lib
        cfg = ops.sr_config(_lib.OPT_ADAM, True, np.float32(1) - B1, np.float32(1) - B2, EPS, use_btv=prior[0] == "btv",
                            btv_alpha=prior[1] if prior[0] == "btv" else 0.6, btv_shift=prior[2] if prior[0] == "btv" else 2)
        kw = dict(data_term=(loss, delta), weights=wts if weighted else None, tv_weights=tvw if prior[0] == "wtv" else None)
        _, terms, trace = _solve(x0, yd, tfs, alphas, cfg=cfg, monitor=TRACE_ONLY, **kw)
        hist = trace.history.cpu().numpy()
        assert hist.shape == (1, BATCH, 4) and np.array_equal(hist[0], terms)          # one iteration: it is also the last
        _, r = ops.sr_forward_residual(ops.to_device(x0), yd, rot, tr, data_term=(loss, delta), weights=wts if weighted else None,
                                       want_raw=True)
        r = r.cpu().numpy()
        if loss == "huber":
            assert (np.abs(r) > np.float32(delta)).any() and (np.abs(r) <= np.float32(delta)).any()      # both branches
        for b in range(BATCH):
            p = prior if prior[0] != "wtv" else ("wtv", wy[b], wx[b])
            _check_terms(hist[0, b], x0[b], r[b], loss, delta, wts_np[b] if weighted else None, p, (loss, weighted, prior[0], b))
        # and against the library's own (atomic) terms, which agree to rounding
        np.testing.assert_allclose(terms, ops.sr_loss_terms(ops.to_device(x0), ops.to_device(r), cfg, data_term=(loss, delta),
                                                            weights=wts if weighted else None,
                                                            tv_weights=tvw if prior[0] == "wtv" else None).cpu().numpy(), rtol=TWO_ORDERS)


# ---- 2. reproducibility ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,h,w,n", SHAPES)
def test_the_trace_is_the_same_bytes_every_time(dev, H, W, h, w, n):
    iters = 6
    y, yd, x0, tfs = _setup(11, H, W, h, w, n)
    alphas = _adam_alphas(iters, BATCH, lr=1e-2)
    mon = dict(TRACE_ONLY, every=2)
    (xs, _, tr0) = _solve(x0, yd, tfs, alphas, monitor=mon)
    h0 = tr0.history.cpu().numpy()
    assert h0.shape == (3, BATCH, 4) and not np.isnan(h0).any()
    for _ in range(2):                                                               # the same call again
        _, _, t = _solve(x0, yd, tfs, alphas, monitor=mon)
        assert t.history.cpu().numpy().tobytes() == h0.tobytes()
    for b in range(BATCH):                                                           # image b alone
        _, _, t = _solve(x0, yd, tfs, alphas, monitor=mon, sel=[b])
        assert t.history.cpu().numpy().tobytes() == h0[:, b:b + 1].tobytes(), b
    _, _, t = _solve(x0, yd, tfs, alphas, monitor=mon, sel=[2, 0])                   # another batch, another place in it
    assert t.history.cpu().numpy().tobytes() == np.ascontiguousarray(h0[:, [2, 0]]).tobytes()
    (xc, _, t) = _solve(x0, yd, tfs, alphas, cfg=_adam_cfg(chunk=1), monitor=mon)     # one copy's planes at a time
    assert t.history.cpu().numpy().tobytes() == h0.tobytes()
    for a, c in zip(xs, xc):
        assert np.array_equal(a, c)


# ---- 3. trace only: the unmonitored solve bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("every", [1, 3, 7])
@pytest.mark.parametrize("H,W,h,w,n", SHAPES)
def test_trace_only_is_the_unmonitored_solve(dev, H, W, h, w, n, every):
    iters = 10
    y, yd, x0, tfs = _setup(13, H, W, h, w, n)
    alphas = _adam_alphas(iters, BATCH, lr=1e-2)
    plain, terms_plain, _ = _solve(x0, yd, tfs, alphas)
    got, terms, trace = _solve(x0, yd, tfs, alphas, monitor=dict(TRACE_ONLY, every=every))
    for a, c in zip(plain, got):
        assert np.array_equal(a, c)
    hist = trace.history.cpu().numpy()
    assert hist.shape == (-(-iters // every), BATCH, 4) and not np.isnan(hist).any()
    assert trace.eval_iters == list(range(0, iters, every))
    assert np.array_equal(trace.iters_done.cpu().numpy(), np.full(BATCH, iters, np.int32))
    np.testing.assert_allclose(terms, terms_plain, rtol=TWO_ORDERS)           # the last iteration's terms: the atomic sums to rounding
    if (iters - 1) % every == 0:
        assert np.array_equal(hist[-1], terms)
    assert trace.losses(LAM).shape == hist.shape[:2] and np.array_equal(trace.losses(LAM), M.scalar_loss(hist, LAM))
    _, _, no_hist = _solve(x0, yd, tfs, alphas, monitor=dict(TRACE_ONLY, every=every, history=False))
    assert no_hist.history is None and np.array_equal(no_hist.iters_done.cpu().numpy(), np.full(BATCH, iters, np.int32))


# ---- 4. stopping -----------------------------------------------------------------------------------------------------------------
STOP_ITERS, STOP_TOL, STOP_PATIENCE = 40, 1e-2, 2
STOP_LR = (1e-2, 3e-2, 1e-2)               # per image: the step scalars are per image


def _stop_batch(H=64, W=64, h=16, w=16, n=5):
    """Image 0: all-zero copies (loss 0 from the start); images 1 and 2: ordinary problems, image 1 with the larger learning
    rate, so that its loss flattens while image 2's still falls."""
    rng = np.random.default_rng(21)
    ys, angs, shs = [], [], []
    for i in range(3):
        ys.append(_blob_masks(rng, n, h, w) if i else np.zeros((n, h, w), np.float32))
        a, s = _angles_shifts(rng, n, 0.15, 0.15 * min(H, W))
        angs.append(a)
        shs.append(s)
    alphas = np.stack([_adam_alphas(STOP_ITERS, 1, lr=lr)[:, 0] for lr in STOP_LR], axis=1)
    return np.stack(ys), np.stack(angs), np.stack(shs), alphas


def _oracle_trace(y, angles, shifts, lr, lam, H, W, iters):
    """The CPU oracle's own loss at every iteration (before that iteration's update), float64 [iters]."""
    n, h, w = y.shape
    sr = o_sr.Superresolution(*lam, num_iter=iters, num_aug=n, optimizer=o_sr.Optimizer("adam", lr, amsgrad=True),
                              feature_size=(h, w), output_size=(H, W))
    smp = torch.from_numpy(y[..., None])
    _, _, traj = sr.augmented_superresolution(smp, angles, shifts, return_trajectory=True)
    xs = [tf_ops.resize_bilinear(smp[0:1], (H, W))] + [torch.from_numpy(t[None]) for t in traj[:-1]]
    return np.array([float(sr.loss_function(t, smp, angles, shifts)) for t in xs], dtype=np.float64)


@pytest.fixture(scope="module")
def stop_case(dev):
    """The batch, its oracle traces (which must themselves give distinct stops, one of them mid-way), and the monitored solve."""
    from asr_amd import ops
    y, angs, shs, alphas = _stop_batch()
    oracle = np.stack([_oracle_trace(y[i], angs[i], shs[i], STOP_LR[i], LAM, 64, 64, STOP_ITERS) for i in range(3)], axis=1)
    want = M.stop_iterations(oracle, 1, STOP_TOL, STOP_PATIENCE, 0)
    print("oracle stops:", want)
    assert want[0] == STOP_PATIENCE and STOP_PATIENCE < want[1] < STOP_ITERS and want[2] == STOP_ITERS, want
    tfs = _tfs(angs, shs, 64, 64)
    yd = ops.to_device(y)
    x0 = ops.sr_init_target(yd, (64, 64)).cpu().numpy()
    return dict(y=y, yd=yd, x0=x0, tfs=tfs, alphas=alphas, oracle_stops=want)


def _assert_stops(case, mon, **kw):
    """The monitored solve of the stop batch under `mon`: iters_done against the restatement applied to the returned history,
    NaN rows after each stop, last terms, and every group of images against the plain solve cut at its iteration."""
    got, terms, trace = _solve(case["x0"], case["yd"], case["tfs"], case["alphas"], monitor=mon, **kw)
    hist = trace.history.cpu().numpy()
    done = trace.iters_done.cpu().numpy()
    lam = kw.get("lam", LAM)
    losses = M.scalar_loss(hist, lam)
    assert np.array_equal(losses, trace.losses(lam), equal_nan=True)
    want = M.stop_iterations(losses, mon["every"], mon["rel_tol"], mon["patience"], mon["min_iter"], num_iter=STOP_ITERS)
    print("iters_done", done, "restatement", want)
    assert np.array_equal(done, want)
    assert len(set(done.tolist())) >= 2 and done.min() < STOP_ITERS                  # not vacuous
    for b, k in enumerate(done):
        rows = [e for e, it in enumerate(trace.eval_iters) if it <= k and it < STOP_ITERS]
        after = [e for e, it in enumerate(trace.eval_iters) if it > k]
        assert not np.isnan(hist[rows, b]).any() and np.isnan(hist[after, b]).all(), (b, k)
        if k < STOP_ITERS:
            assert np.array_equal(terms[b], hist[k // mon["every"], b])               # the loss of the x that is returned
    for k in sorted(set(done.tolist())):
        plain, _, _ = _solve(case["x0"], case["yd"], case["tfs"], case["alphas"][:k], **kw)
        for b in np.flatnonzero(done == k):
            for name, a, c in zip("x m v vhat".split(), plain, got):
                assert np.array_equal(a[b], c[b]), (k, b, name)
    return done


def test_each_image_stops_by_itself(dev, stop_case):
    mon = dict(every=1, rel_tol=STOP_TOL, patience=STOP_PATIENCE, min_iter=0, history=True)
    done = _assert_stops(stop_case, mon)
    assert done[0] == STOP_PATIENCE and STOP_PATIENCE < done[1] < STOP_ITERS and done[2] == STOP_ITERS
    assert np.array_equal(done, stop_case["oracle_stops"])


def test_min_iter_delays_a_stop(dev, stop_case):
    mon = dict(every=1, rel_tol=STOP_TOL, patience=STOP_PATIENCE, min_iter=7, history=True)
    done = _assert_stops(stop_case, mon)
    assert done[0] == 7
    done = _assert_stops(stop_case, dict(mon, every=3, min_iter=7))
    assert done[0] == 9                                                               # the first evaluation >= 7


# ---- 5. combinations ---------------------------------------------------------------------------------------------------------------
def test_stop_with_every_4(dev, stop_case):
    done = _assert_stops(stop_case, dict(every=4, rel_tol=STOP_TOL, patience=STOP_PATIENCE, min_iter=0, history=True))
    assert done[0] == 8


def test_stop_under_huber_weights_and_edge_weighted_tv(dev, stop_case):
    n, h, w = stop_case["y"].shape[1:]
    wts = torch.as_tensor(np.random.default_rng(31).random((3, n, h, w), dtype=np.float32)).to(dev)
    _, tvw = _random_weights(32, (3, 64, 64), dev)
    _assert_stops(stop_case, dict(every=1, rel_tol=STOP_TOL, patience=STOP_PATIENCE, min_iter=0, history=True),
                  data_term=("huber", 0.2), weights=wts, tv_weights=tvw)


def test_stop_under_bilateral_tv(dev, stop_case):
    from asr_amd import _lib, ops
    cfg = ops.sr_config(_lib.OPT_ADAM, True, np.float32(1) - B1, np.float32(1) - B2, EPS, use_btv=True, btv_alpha=0.6, btv_shift=2)
    _assert_stops(stop_case, dict(every=2, rel_tol=STOP_TOL, patience=STOP_PATIENCE, min_iter=0, history=True), cfg=cfg)


def test_stop_under_a_projective_transform(dev):
    """The (128, 128, 32, 32, 4) problem with genuinely projective rotation vectors (the kernels' generic branches), image 0
    with all-zero copies: it stops, the others do not, and each equals the plain solve cut at its iteration."""
    from asr_amd import ops, transforms as T
    H, h, n, iters = 128, 32, 4, 12
    y, angs, shs = _problem(41, 3, n, H, H, h, h)
    y[0] = 0.0
    rot = np.stack([T.rotation_transforms(angs[i], H, H) for i in range(3)])
    rot[:, 1:, 6] = 2e-5
    rot[:, 1:, 7] = -3e-5
    tr = np.stack([T.translation_transforms(shs[i]) for i in range(3)])
    tr[:, 2, 0] = 1.01                                                                # affine, not a pure translation
    irot = np.stack([T.inverse_transforms(rot[i]) for i in range(3)])
    itr = np.stack([T.inverse_transforms(tr[i]) for i in range(3)])
    tfs = [ops.to_device(t) for t in (rot, tr, irot, itr)]
    yd = ops.to_device(y)
    x0 = ops.sr_init_target(yd, (H, H)).cpu().numpy()
    alphas = _adam_alphas(iters, 3, lr=1e-2)
    mon = dict(every=1, rel_tol=1e-6, patience=2, min_iter=0, history=True)
    got, terms, trace = _solve(x0, yd, tfs, alphas, monitor=mon)
    done = trace.iters_done.cpu().numpy()
    hist = trace.history.cpu().numpy()
    assert np.array_equal(done, M.stop_iterations(M.scalar_loss(hist, LAM), 1, 1e-6, 2, 0, num_iter=iters))
    assert done[0] == 2 and len(set(done.tolist())) >= 2
    for k in sorted(set(done.tolist())):
        plain, _, _ = _solve(x0, yd, tfs, alphas[:k])
        for b in np.flatnonzero(done == k):
            for a, c in zip(plain, got):
                assert np.array_equal(a[b], c[b]), (k, b)


# ---- 6. the upper layer ------------------------------------------------------------------------------------------------------------
def test_superresolution_keywords(dev, stop_case):
    """Superresolution(stop_rel_tol=...): last_trace holds the trace, the counter advances by num_iter per image whether it
    stops or not, and without the keywords nothing changes."""
    from asr_amd.superresolution_scripts.optimizer import Optimizer
    from asr_amd.superresolution_scripts.superresolution import Superresolution
    y, (rot, tr, irot, itr) = stop_case["y"], stop_case["tfs"]
    angs = np.zeros(y.shape[:2], np.float32)
    shs = np.zeros(y.shape[:2] + (2,), np.float32)
    kw = dict(num_iter=12, num_aug=y.shape[1], feature_size=y.shape[2:], output_size=(64, 64))
    def run(**extra):
        opt = Optimizer("adam", 1e-2, amsgrad=True)
        sr = Superresolution(*LAM, optimizer=opt, **kw, **extra)
        x, terms = sr.augmented_superresolution_batch(stop_case["yd"], angs, shs)
        return sr, x.cpu().numpy(), terms.cpu().numpy(), opt.optimizer.iterations
    sr0, x0, t0, it0 = run()
    assert sr0.last_trace is None
    sr1, x1, t1, it1 = run(keep_history=True, stop_every=5)
    assert np.array_equal(x0, x1) and it0 == it1 and sr1.last_trace.history.shape == (3, 3, 4)
    sr2, x2, t2, it2 = run(stop_rel_tol=1e-3, stop_patience=2)
    done = sr2.last_trace.iters_done.cpu().numpy()
    assert it2 == it0 and sr2.last_trace.history is None and done[0] == 2 and done.max() <= 12
    assert np.array_equal(x2[0], np.zeros((64, 64), np.float32))
