"""The primal-dual rule on the device (include/asr_hip.h, "primal-dual"; ASR_OPT_PRIMAL_DUAL through ops.sr_solve, the step
bound through ops.sr_data_bound) against its restatement tests/sr_pd_ref.py, bit for bit: x and both dual planes after 1, 2
and 3 iterations, for any plane chunking; the update statements alone on the device's own data-term gradient; plain SGD under
the same step sizes when there is no TV term (a check that owes nothing to the restatement); the bound after 1, 3 and 6
repetitions with and without weights; and the monitor's frozen image against the unmonitored solve cut at its iteration.
No tolerance anywhere: sr.hip is built without contraction and the restatement rounds every operation by itself."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import tf_ops
from test_gpu_sr_wtv import _problem

import sr_pd_ref as P

pytestmark = pytest.mark.gpu

# name -> (H, W), (h, w), copies, batch, lambdas, data term, weighted data term, edge-weighted TV
CASES = {
    "16x16": ((16, 16), (8, 8), 3, 1, (1.0, 0.3, 0.7, 0.0), ("l2", 0.1), False, False),
    # three 64 x 4 gather workgroups each way, the last ones partial; batch 2 with different transforms
    "12x136": ((12, 136), (6, 68), 5, 2, (1.0, 0.3, 0.7, 0.0), ("l2", 0.1), False, False),
    # f = 4; edge weights in [0, 1] with exact zeros, Huber, a weight plane, lambda_l1 > 0
    "32x32": ((32, 32), (8, 8), 4, 1, (1.0, 0.3, 0.7, 0.05), ("huber", 0.1), True, True),
}
ITERS = 3
DUAL_RATIO = 1.0 / 16.0


@functools.lru_cache(maxsize=None)
def _case(name):
    """Host arrays of a case and its restated trajectory: computed once, shared by the tests, never changed."""
    (H, W), (h, w), n, b, lam, (loss, delta), weighted, wtv = CASES[name]
    seed = 40 + list(CASES).index(name)
    y, angs, shs = _problem(seed, b, n, H, W, h, w)
    rng = np.random.default_rng(seed + 100)
    y = (y + 0.1 * rng.random(y.shape, dtype=np.float32)).astype(np.float32)
    tfs = [P.transforms(angs[i], shs[i], (H, W)) for i in range(b)]
    x0 = np.stack([tf_ops.resize_bilinear(torch.from_numpy(y[i, 0:1, :, :, None]), (H, W)).numpy()[0, :, :, 0] for i in range(b)])
    x0 = (x0 + 0.05 * rng.standard_normal(x0.shape).astype(np.float32)).astype(np.float32)
    wts = None
    if weighted:
        wts = rng.random((b, n, h, w), dtype=np.float32)
        wts[:, 0, :2] = 0.0
    wy = wx = None
    if wtv:
        wy, wx = (rng.random((b, H, W), dtype=np.float32) for _ in range(2))
        for plane in (wy, wx):
            plane[rng.random(plane.shape) < 0.1] = 0.0
            plane[rng.random(plane.shape) < 0.1] = 1.0
    srs = [P.make_sr(lam, n, (h, w), (H, W), loss, delta, None if wts is None else wts[i]) for i in range(b)]
    # the bound is taken under L2 with the same weights; the step of image i is its own
    bound_srs = [P.make_sr((lam[0], 0, 0, 0), n, (h, w), (H, W), weights=None if wts is None else wts[i]) for i in range(b)]
    bounds = np.array([[P.data_bound(bound_srs[i], tfs[i], 6, all_iters=True)[k - 1] for i in range(b)] for k in (1, 3, 6)], np.float32)
    plain_srs = [P.make_sr((lam[0], 0, 0, 0), n, (h, w), (H, W)) for i in range(b)]
    bounds_plain = np.array([[P.data_bound(plain_srs[i], tfs[i], 6, all_iters=True)[k - 1] for i in range(b)] for k in (1, 3, 6)],
                            np.float32)
    taus = np.array([P.pd_tau(bounds[2, i], lam[2]) for i in range(b)], np.float32)
    traj = [P.pd_solve(srs[i], x0[i], y[i], tfs[i], [taus[i]] * ITERS, DUAL_RATIO, None if wy is None else wy[i],
                       None if wx is None else wx[i], trajectory=True) for i in range(b)]
    return SimpleNamespace(H=H, W=W, h=h, w=w, n=n, b=b, lam=lam, dt=(loss, delta), y=y, tfs=tfs, x0=x0, wts=wts, wy=wy, wx=wx,
                           srs=srs, bounds=bounds, bounds_plain=bounds_plain, taus=taus, traj=traj)


def _device(c, dev):
    """The case on the device: y, the four transform stacks (the oracle's own vectors), weights and edge weights."""
    from asr_amd import ops
    tf = [ops.to_device(np.stack([c.tfs[i][k] for i in range(c.b)]).astype(np.float32)) for k in range(4)]
    wts = None if c.wts is None else torch.as_tensor(c.wts).to(dev)
    tvw = None if c.wy is None else (torch.as_tensor(c.wy).to(dev), torch.as_tensor(c.wx).to(dev))
    return ops.to_device(c.y), tf, wts, tvw


def _cfg(chunk=0, c0=DUAL_RATIO):
    from asr_amd import _lib, ops
    return ops.sr_config(_lib.OPT_PRIMAL_DUAL, c0=c0, plane_chunk=chunk)


def _solve(c, dev, alphas, x0=None, lam=None, cfg=None, monitor=None, state=None, plain=False):
    """ops.sr_solve of the case -> (x, p_y, p_x) host arrays (+ the trace with a monitor); plain: no data term, no edge weights."""
    from asr_amd import ops
    yd, tf, wts, tvw = _device(c, dev)
    kw = {}
    if not plain:
        if c.dt[0] != "l2" or wts is not None:
            kw.update(data_term=c.dt, weights=wts)
        if tvw is not None:
            kw["tv_weights"] = tvw
    st = {} if state is None else state
    out = ops.sr_solve(ops.to_device(c.x0 if x0 is None else x0), yd, *tf, ops.to_device(np.ascontiguousarray(alphas, np.float32)),
                       c.lam if lam is None else lam, cfg=cfg if cfg is not None else _cfg(), state=st, want_loss=False,
                       monitor=monitor, **kw)
    arrs = (out[0].cpu().numpy(), st["m"].cpu().numpy(), st["v"].cpu().numpy())
    return arrs + ((out[2],) if monitor is not None else ())


def _report(what, got, want):
    """Print how far apart two float32 arrays are before any assertion on them."""
    got, want = np.asarray(got), np.asarray(want)
    bad = int((got != want).sum())
    print(f"{what}: {bad} of {got.size} values differ, max |diff| {float(np.abs(got.astype(np.float64) - want).max()):.3e}")
    return bad


# ---- 1. the iteration against the restatement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_one_two_and_three_iterations_are_the_restatement_bit_for_bit(dev, name):
    c = _case(name)
    alphas = np.tile(c.taus[None], (ITERS, 1))
    for k in (1, 2, 3):
        got = _solve(c, dev, alphas[:k])
        for i in range(c.b):
            for what, g, want in zip(("x", "p_y", "p_x"), got, c.traj[i][k - 1]):
                _report(f"{name} image {i} after {k}: {what}", g[i], want)
        for i in range(c.b):
            for what, g, want in zip(("x", "p_y", "p_x"), got, c.traj[i][k - 1]):
                assert np.array_equal(g[i], want), (name, i, k, what)
    # the duals did something: they are neither all zero nor all at a bound
    py = got[1]
    assert (py != 0).any() and (np.abs(py) < np.float32(c.lam[1])).any()


def test_the_result_does_not_depend_on_plane_chunk(dev):
    c = _case("12x136")
    alphas = np.tile(c.taus[None], (ITERS, 1))
    whole = _solve(c, dev, alphas)
    for chunk in (2, 1):
        for a, r in zip(_solve(c, dev, alphas, cfg=_cfg(chunk=chunk)), whole):
            assert a.tobytes() == r.tobytes(), chunk
    for i in range(c.b):                                              # and an image alone is the image in its batch
        one = SimpleNamespace(**{**vars(c), "b": 1, "y": c.y[i:i + 1], "tfs": c.tfs[i:i + 1], "x0": c.x0[i:i + 1]})
        for a, r in zip(_solve(one, dev, alphas[:, i:i + 1]), whole):
            assert a.tobytes() == r[i:i + 1].tobytes(), i


# ---- 2. the update statements on the device's own data-term gradient -------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_the_update_statements_on_the_device_gradient(dev, name):
    """Two solves of one iteration, the second starting from the duals of the first: each equals the restated statements
    applied to the gradient the device itself returns for that x (a gradient-only launch with every prior off)."""
    from asr_amd import ops
    c = _case(name)
    yd, tf, wts, tvw = _device(c, dev)
    state = {}
    x, py, px = c.x0, np.zeros_like(c.x0), np.zeros_like(c.x0)
    for step in range(2):
        xd = ops.to_device(x)
        q = ops.sr_forward_residual(xd, yd, tf[0], tf[1], data_term=c.dt, weights=wts)
        _, g_df = ops.sr_backward(xd, q, tf[2], tf[3], (c.lam[0], 0.0, 0.0, 0.0), ops.sr_config(), state=None)
        g_df = g_df.cpu().numpy()
        got = _solve(c, dev, c.taus[None], x0=x, state=state)
        for i in range(c.b):
            want = P.pd_update(c.srs[i], x[i], py[i], px[i], g_df[i], c.taus[i], DUAL_RATIO, None if c.wy is None else c.wy[i],
                               None if c.wx is None else c.wx[i])[:3]
            for what, g, w_ in zip(("x", "p_y", "p_x"), got, want):
                assert np.array_equal(g[i], w_), (name, step, i, what)
        x, py, px = got


# ---- 3. no TV term: plain gradient descent ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_without_tv_and_l1_the_solve_is_sgd_without_momentum(dev, name):
    from asr_amd import _lib, ops
    c = _case(name)
    lam = (c.lam[0], 0.0, c.lam[2], 0.0)
    alphas = np.tile(c.taus[None], (ITERS, 1))
    pd = _solve(c, dev, alphas, lam=lam, plain=True)
    sgd = _solve(c, dev, alphas, lam=lam, plain=True, cfg=ops.sr_config(_lib.OPT_SGD))
    assert np.array_equal(pd[0], sgd[0])
    assert not pd[1].any() and not pd[2].any()                       # a box of width 0: the duals stay 0
    assert not np.array_equal(pd[0], c.x0)


# ---- 4. the bound -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name", list(CASES))
def test_the_bound_is_the_restatement_bit_for_bit(dev, name, weighted):
    from asr_amd import ops
    c = _case(name)
    if weighted and c.wts is None:
        rng = np.random.default_rng(7)
        wts_np = rng.random((c.b, c.n, c.h, c.w), dtype=np.float32)
        srs = [P.make_sr((c.lam[0], 0, 0, 0), c.n, (c.h, c.w), (c.H, c.W), weights=wts_np[i]) for i in range(c.b)]
        want = np.array([[P.data_bound(srs[i], c.tfs[i], 6, all_iters=True)[k - 1] for i in range(c.b)] for k in (1, 3, 6)], np.float32)
    else:
        wts_np, want = (c.wts, c.bounds) if weighted else (None, c.bounds_plain)
    _, tf, _, _ = _device(c, dev)
    wd = None if wts_np is None else torch.as_tensor(wts_np).to(dev)
    for row, iters in enumerate((1, 3, 6)):
        got = ops.sr_data_bound(*tf, (c.H, c.W), (c.h, c.w), c.lam[0], weights=wd, iters=iters).cpu().numpy()
        print(f"{name} weighted={weighted} iters={iters}: device {got.tolist()} restatement {want[row].tolist()}")
        assert got.dtype == np.float32 and got.shape == (c.b,)
        assert np.array_equal(got, want[row]), (name, weighted, iters)
        assert (got > 0).all()
    # the same bits again, for another chunking, and with one stack of weights shared by the batch
    again = ops.sr_data_bound(*tf, (c.H, c.W), (c.h, c.w), c.lam[0], weights=wd, iters=6).cpu().numpy()
    chunked = ops.sr_data_bound(*tf, (c.H, c.W), (c.h, c.w), c.lam[0], weights=wd, iters=6, cfg=ops.sr_config(plane_chunk=2)).cpu().numpy()
    assert again.tobytes() == got.tobytes() == chunked.tobytes()
    if wd is not None:
        shared = ops.sr_data_bound(*tf, (c.H, c.W), (c.h, c.w), c.lam[0], weights=wd[0].contiguous(), iters=6).cpu().numpy()
        assert shared[0] == got[0]


def test_pd_steps_are_built_on_the_device(dev):
    from asr_amd import ops
    c = _case("12x136")
    bound = torch.as_tensor(np.array([c.bounds[2, 0], 0.0], np.float32)).to(dev)
    steps = ops.pd_steps(bound, c.lam[2], 4)
    assert steps.is_cuda and steps.shape == (4, 2) and steps.is_contiguous()
    want = np.array([P.pd_tau(c.bounds[2, 0], c.lam[2]), P.pd_tau(0.0, c.lam[2])], np.float32)
    assert np.array_equal(steps.cpu().numpy(), np.tile(want[None], (4, 1)))
    assert ops.pd_steps(bound, 0.0, 1).cpu().numpy()[0, 1] == 0.0                 # a denominator of 0: a step of 0


# ---- 5. the monitor -----------------------------------------------------------------------------------------------------------------
def test_a_frozen_image_keeps_x_and_both_duals(dev):
    """Batch 2: image 0 gets a step so short that its loss stalls and it stops at the second stalled evaluation; image 1 runs
    on.  Each equals the unmonitored solve cut at its own iteration, x and both dual planes, bit for bit."""
    c = _case("12x136")
    iters = 6
    alphas = np.tile(np.array([1e-7, c.taus[1]], np.float32)[None], (iters, 1))
    mon = dict(every=1, rel_tol=1e-3, patience=2, min_iter=0, history=True)
    x, py, px, trace = _solve(c, dev, alphas, monitor=mon)
    done = trace.iters_done.cpu().numpy()
    print("iters_done", done.tolist(), "losses", trace.losses(c.lam).T.tolist())
    assert done[0] == 2 and done[0] < done[1] <= iters
    for i in range(c.b):
        cut = _solve(c, dev, alphas[:done[i]])
        for what, got, want in zip(("x", "p_y", "p_x"), (x, py, px), cut):
            assert np.array_equal(got[i], want[i]), (i, what)
    full = _solve(c, dev, alphas)
    assert not np.array_equal(full[0][0], x[0])                                  # the stop did cut image 0 short
    if done[1] == iters:
        assert all(np.array_equal(a[1], b_[1]) for a, b_ in zip((x, py, px), full))
