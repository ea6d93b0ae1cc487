"""The option kernels of the SR solver (csrc/sr.hip: the DT, MON and WTV instantiations, the primal-dual gather, the step bound) on
the geometries of tests/test_gpu_sr_shapes.py -- f = 8 and the generic factor 6, planes narrower than a tile, an out-of-frame
copy, the affine-but-not-pure and projective translate stages, a projective rotation, a short last plane chunk -- where the
feature suites (test_gpu_sr_dt / _monitor / _wtv / _pd) do not go.  The cases and the instantiations each one launches are in
tests/sr_option_cases.py.

Every check is a chain of exact equalities anchored on a kernel form that test_gpu_sr_shapes.py and test_gpu_sr_update.py
already hold against the oracle (the plain solve, the unbordered forward kernel and the fused backward without options):
  a. an option that is on in the instantiation and neutral in value returns the plain solve;
  b. with the options in effect, the split solve is the loop of single steps, q is psi applied to the device's own r, and the
     loss terms are those of sr_loss_terms on the same state;
  c. the primal-dual solve is its own single iterations, each of them the restated update on the device's own gradient;
  d. a monitored image that stops equals the plain solve cut at its iteration;
  e. the step bound is the maximum of the device's own gradient, repeated on the host.
x, the optimiser slots, the duals, q, r and the bound are compared bit for bit (sr.hip is built without contraction).  The
loss terms are the one exception: the unmonitored kernels add their float64 partial sums with atomics, in the order of
arrival, so two runs of the SAME solve need not return the same bits.  They are held to the bound that
test_gpu_sr_monitor.py derives (two orders of adding N summands >= 0: 2 N 2^-53 relative) and, against sr_loss_terms, to the
1e-12 of test_gpu_sr_dt.py; the monitor's own terms, which have a fixed order, are compared bit for bit with its history.
The number of differing values and the largest difference of every comparison are printed before it is asserted."""
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_gpu_sr_wtv import B1, B2, EPS, _adam_alphas, _adam_cfg

import sr_dt_ref as RD
import sr_mon_ref as M
import sr_option_cases as T
import sr_pd_ref as P

pytestmark = pytest.mark.gpu

LAM = (1.0, 0.3, 0.7, 0.05)
ITERS = 3
DUAL_RATIO = 1.0 / 16.0
TRACE_ONLY = dict(every=1, rel_tol=0.0, patience=0, min_iter=0, history=True)
PD_SR = SimpleNamespace(lambda_tv=LAM[1], lambda_L2=LAM[2], lambda_L1=LAM[3])     # what sr_pd_ref.pd_update reads of its `sr`


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t0 = time.perf_counter()
    yield
    print(f"\n[sr_option_shapes] wall time of the file: {time.perf_counter() - t0:.1f} s")


# ---- helpers -------------------------------------------------------------------------------------------------------------------------
def _report(what, got, want):
    """Print how far apart two arrays are before any assertion on them; -> the number of differing values (+0 == -0)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = int((got != want).sum())
    diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print(f"[sr_option_shapes] {what}: {bad} of {got.size} values differ, max |diff| {float(np.nanmax(diff)) if diff.size else 0.0:.3e}")
    return bad


def _same(tag, got, want, names):
    """Report every named array of two results, then assert that none differs."""
    bad = {k: _report(f"{tag} {k}", getattr(got, k), getattr(want, k)) for k in names}
    assert not any(bad.values()), (tag, bad)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _cfg(rule, chunk=0):
    from asr_amd import _lib, ops
    if rule == "adam":
        return _adam_cfg(chunk)
    if rule == "sgd":
        return ops.sr_config(_lib.OPT_SGD, plane_chunk=chunk)
    assert rule == "pd"
    return ops.sr_config(_lib.OPT_PRIMAL_DUAL, c0=DUAL_RATIO, plane_chunk=chunk)


def _alphas(rule, iters):
    """[iters, B] step scalars, another one for each image."""
    a = _adam_alphas(iters, T.BATCH, lr=1e-2) if rule == "adam" else np.full((iters, T.BATCH), 2e-3, np.float32)
    a[:, 1] *= np.float32(1.25)
    return a


class _Inputs:
    """A problem of the table on the device, and the option values of a case for it."""

    def __init__(self, dev, shape, kind, y=None):
        from asr_amd import ops
        self.p = T.problem(shape, kind)
        self.dev = dev
        self.y_np = self.p.y if y is None else y
        _, self.rot, self.tr, self.irot, self.itr = self.p.device()
        self.yd = ops.to_device(self.y_np)
        self.x0 = self.p.x                                          # the resized copy 0 plus noise: no term is trivial
        self.hw = (self.p.H, self.p.W)

    def options(self, case, neutral=False, delta=None):
        """-> (keywords of ops.sr_solve / sr_forward_residual / sr_loss_terms, host weights, host (wy, wx))."""
        w_np, tv_np = T.data_weights(case, neutral), T.edge_weights(case, neutral)
        kw = {}
        if case.loss != "l2" or w_np is not None:
            kw["data_term"] = (case.loss, delta) if case.loss == "huber" else case.loss
            kw["weights"] = None if w_np is None else torch.as_tensor(w_np).to(self.dev)
        if tv_np is not None:
            kw["tv_weights"] = tuple(torch.as_tensor(t).to(self.dev) for t in tv_np)
        return kw, w_np, tv_np

    def residual(self, x, **kw):
        from asr_amd import ops
        return ops.sr_forward_residual(x if isinstance(x, torch.Tensor) else ops.to_device(x), self.yd, self.rot, self.tr, **kw)

    def clip(self, x=None, share=0.3):
        """A Huber delta that clips a share of the residuals of x (the start by default): some, not all."""
        r = np.abs(self.residual(self.x0 if x is None else x).cpu().numpy())
        delta = float(np.float32(share) * r.max())
        assert (r > np.float32(delta)).any() and not (r > np.float32(delta)).all()
        return delta

    def solve(self, case, alphas, kw=None, x0=None, state=None, monitor=None, want_loss=True, lam=LAM):
        """ops.sr_solve of the case -> host arrays x, m, v, vhat, terms (+ trace).  The plain AMSGrad solve with all copies at
        once is the very call of test_gpu_sr_shapes._solve (asr_sr_solve_f32); everything else goes through a config."""
        from asr_amd import ops
        kw = kw or {}
        st = {} if state is None else state
        args = (ops.to_device(self.x0 if x0 is None else x0), self.yd, self.rot, self.tr, self.irot, self.itr,
                ops.to_device(np.ascontiguousarray(alphas, np.float32)), lam)
        if case.rule == "adam" and not kw and monitor is None and case.chunk == 0:
            out = ops.sr_solve(*args, np.float32(1) - B1, np.float32(1) - B2, EPS, True, want_loss=want_loss, state=st)
        else:
            out = ops.sr_solve(*args, cfg=_cfg(case.rule, case.chunk), want_loss=want_loss, state=st, monitor=monitor, **kw)
        return SimpleNamespace(x=out[0].cpu().numpy(), m=st["m"].cpu().numpy(), v=st["v"].cpu().numpy(), vhat=st["vhat"].cpu().numpy(),
                               terms=None if out[1] is None else out[1].cpu().numpy(), trace=out[2] if monitor is not None else None)


@pytest.fixture(scope="module")
def inputs(dev):
    made = {}

    def get(shape, kind):
        if (shape, kind) not in made:
            made[(shape, kind)] = _Inputs(dev, shape, kind)
        return made[(shape, kind)]
    return get


def _terms_close(tag, got, want, p):
    """Loss terms of two summation orders (module docstring): 2 N 2^-53 relative, N the larger count of summands."""
    n_sum = max(p.n * p.h * p.w, p.H * p.W)
    assert (want > 0).all()
    rel = np.abs(got - want) / np.abs(want)
    print(f"[sr_option_shapes] {tag} loss terms: {int((got != want).sum())} of {got.size} values differ, max relative |diff| "
          f"{float(rel.max()):.3e} (bound {2 * n_sum * 2.0 ** -53:.3e})")
    np.testing.assert_allclose(got, want, rtol=2 * n_sum * 2.0 ** -53, atol=0)


def _cid(case):
    return "-".join(str(v) for v in case)


# ---- a. on in the instantiation, off in value ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,kind", T.NEUTRAL_GEOMETRIES)
def test_a_neutral_options_return_the_plain_solve(dev, inputs, shape, kind):
    """A Huber delta above every residual of the trajectory, all-one weights (per image and shared), all-one edge weights (per
    image and shared) and a monitor that never stops, alone and all together, under AMSGrad, SGD and a last chunk of one copy:
    x, m, v and vhat of the plain solve bit for bit, its last loss terms to the order of their sums."""
    from asr_amd import ops
    inp = inputs(shape, kind)
    cases = T.neutral_variants(shape, kind)
    plain, big = {}, 0.0
    for rule in ("adam", "sgd"):
        c = T.plain(cases[0])._replace(rule=rule)
        alphas = _alphas(rule, ITERS)
        plain[rule] = inp.solve(c, alphas)
        assert np.isfinite(plain[rule].x).all() and not np.array_equal(plain[rule].x, inp.x0)
        # the plain run once more, one iteration per call, for the residual of every iterate
        st, x = {}, inp.x0
        for it in range(ITERS):
            big = max(big, float(inp.residual(x).abs().max()))
            x = inp.solve(c, alphas[it:it + 1], x0=x, state=st, want_loss=False).x
        assert _report(f"{shape}/{kind} {rule}: one call against {ITERS} calls of one iteration, x", x, plain[rule].x) == 0
    # plain SGD has no solver test of its own: three fused steps (test_gpu_sr_update holds the fused step to its restatement)
    alphas, x = _alphas("sgd", ITERS), ops.to_device(inp.x0)
    for it in range(ITERS):
        x, _ = ops.sr_backward(x, inp.residual(x), inp.irot, inp.itr, LAM, _cfg("sgd"), state=dict(alphas=ops.to_device(alphas[it])))
    assert _report(f"{shape}/{kind} sgd: the plain solve against {ITERS} fused steps, x", plain["sgd"].x, x.cpu().numpy()) == 0
    delta = 2.0 * big
    assert np.isfinite(np.float32(delta)) and np.float32(delta) > np.float32(big)
    for case in cases:
        kw, w_np, tv_np = inp.options(case, neutral=True, delta=delta)
        assert all((a == 1).all() for a in ([] if w_np is None else [w_np]) + list(tv_np or ()))
        mon = TRACE_ONLY if case.monitor == "trace" else None
        got = inp.solve(case, _alphas(case.rule, ITERS), kw, monitor=mon)
        tag = f"{_cid(case)}:"
        print(f"[sr_option_shapes] {tag} {sorted(T.instantiations(case) - T.SOLVER_HELPERS)}")
        _same(tag, got, plain[case.rule], ("x", "m", "v", "vhat"))
        _terms_close(tag, got.terms, plain[case.rule].terms, inp.p)
        if mon is not None:
            done, hist = got.trace.iters_done.cpu().numpy(), got.trace.history.cpu().numpy()
            assert np.array_equal(done, np.full(T.BATCH, ITERS, np.int32)), done
            assert hist.shape == (ITERS, T.BATCH, 4) and not np.isnan(hist).any()
            assert hist[-1].tobytes() == got.terms.tobytes()              # the monitor's own sums have one order


# ---- b. options with effect ------------------------------------------------------------------------------------------------------------
def _in_frame(inp):
    """bool [B, N, h, w]: measurements that see the frame -- the forward model of an all-one x is > 0 there and exactly 0
    where every tap is outside."""
    from asr_amd import ops
    ones = torch.ones((T.BATCH,) + inp.hw, device=inp.dev)
    d1 = ops.sr_forward_residual(ones, torch.zeros_like(inp.yd), inp.rot, inp.tr).cpu().numpy()
    assert not d1[:, T.OUT_OF_FRAME].any() and (d1[:, 0] > 0).all()     # the out-of-frame copy; the identity copy
    return d1 > 0


@pytest.mark.parametrize("opt", T.B_OPTIONS, ids=lambda o: "-".join(o))
def test_b_split_solve_is_the_loop_of_single_steps(dev, inputs, opt):
    """asr_sr_solve_dt_f32 (bordered DT forward kernel, K_gt + the WTV gather) for plane_chunk 0, 2 and 1 against
    3 x (asr_sr_forward_residual_dt_f32 + the fused asr_sr_backward_wtv_f32), AMSGrad: x, m, v, vhat bit for bit; and the
    solve's loss terms against sr_loss_terms on the state they are taken from."""
    from asr_amd import ops
    base = T.Case(*opt, "adam", "off", 0)
    inp = inputs(base.shape, base.kind)
    delta = inp.clip() if base.loss == "huber" else None
    kw, w_np, tv_np = inp.options(base, delta=delta)
    if w_np is not None:
        zero_in_frame = (np.broadcast_to(w_np, inp.y_np.shape) == 0) & _in_frame(inp)
        assert zero_in_frame.any() and (w_np == 1).any() and ((w_np > 0) & (w_np < 1)).any()
    assert all((t == 0).any() and (t == 1).any() for t in tv_np)
    fwd_kw = {k: v for k, v in kw.items() if k != "tv_weights"}
    alphas = _alphas("adam", ITERS)
    x = ops.to_device(inp.x0)
    slots = {k: torch.zeros_like(x) for k in ("m", "v", "vhat")}
    for it in range(ITERS):
        q = inp.residual(x, **fwd_kw)
        x, _ = ops.sr_backward(x, q, inp.irot, inp.itr, LAM, _adam_cfg(), state=dict(slots, alphas=ops.to_device(alphas[it])),
                               tv_weights=kw.get("tv_weights"))
    want = SimpleNamespace(x=x.cpu().numpy(), **{k: t.cpu().numpy() for k, t in slots.items()})
    assert np.isfinite(want.x).all() and not np.array_equal(want.x, inp.x0)
    print(f"[sr_option_shapes] steps: {sorted(T.instantiations(T.steps_of(base)))}")
    for chunk in (0, 2, 1):
        case = base._replace(chunk=chunk)
        assert case in T.B_CASES
        got = inp.solve(case, alphas, kw)
        print(f"[sr_option_shapes] {_cid(case)}: {sorted(T.instantiations(case) - T.SOLVER_HELPERS)}")
        _same(_cid(case), got, want, ("x", "m", "v", "vhat"))
        if chunk == 0:
            terms = got.terms
    # the options did something: the plain loop of the same steps ends elsewhere
    assert not np.array_equal(inp.solve(T.plain(base), alphas).x, want.x)
    # the loss terms: those of the last iteration, before its update, on the raw residual
    before = inp.solve(base, alphas[:ITERS - 1], kw, want_loss=False)
    x2 = ops.to_device(before.x)
    _, r = inp.residual(x2, want_raw=True, **fwd_kw)
    ref = ops.sr_loss_terms(x2, r, _adam_cfg(), tv_weights=kw.get("tv_weights"), **fwd_kw).cpu().numpy()
    print(f"[sr_option_shapes] {_cid(base)} loss terms: solve {terms.tolist()} sr_loss_terms {ref.tolist()}")
    np.testing.assert_allclose(terms, ref, rtol=1e-12)


@pytest.mark.parametrize("shape,kind", T.B_FORWARD_GEOMETRIES)
def test_b_q_is_psi_of_the_devices_own_residual(dev, inputs, shape, kind):
    """want_raw: r is the plain kernel's residual and q = w * psi(r), both bit for bit (signed zeros included), for L2, L1 and
    Huber with per-image and with shared weights.  Six measurements are arranged to give r = +0 exactly."""
    from asr_amd import ops
    base = inputs(shape, kind)
    xd = ops.to_device(base.x0)
    d = ops.sr_forward_residual(xd, torch.zeros_like(base.yd), base.rot, base.tr).cpu().numpy()        # r = D - 0
    y = base.p.y.copy()
    for i in range(T.BATCH):
        y[i, 0, 0, :3] = d[i, 0, 0, :3]                               # r = D - D = +0
    inp = _Inputs(dev, shape, kind, y=y)
    r_plain = inp.residual(xd).cpu().numpy()
    assert int((r_plain == 0).sum()) >= 3 * T.BATCH and np.array_equal(r_plain[:, T.OUT_OF_FRAME], -y[:, T.OUT_OF_FRAME])
    delta = inp.clip(share=0.3)
    in_frame = _in_frame(inp)
    for case in [c for c in T.B_FORWARD if (c.shape, c.kind) == (shape, kind)]:
        kw, w_np, _ = inp.options(case, delta=delta)
        assert ((np.broadcast_to(w_np, y.shape) == 0) & in_frame).any()
        q, r = inp.residual(xd, want_raw=True, **kw)
        want = RD.weighted_psi(r_plain, case.loss, delta, w_np)
        tag = _cid(case)
        r_np, q_np = r.cpu().numpy(), q.cpu().numpy()
        bad_r, bad_q = _report(f"{tag} r", r_np, r_plain), _report(f"{tag} q", q_np, want)
        assert bad_r == 0 and bad_q == 0, (tag, bad_r, bad_q)
        assert np.array_equal(_bits(r_np), _bits(r_plain)) and np.array_equal(_bits(q_np), _bits(want)), tag    # the zeros' signs
        assert torch.equal(inp.residual(xd, **kw), q)                  # the same q without the second output
        if case.loss != "l2":
            assert not np.array_equal(RD.psi(r_plain, case.loss, delta), r_plain)


# ---- c. primal-dual --------------------------------------------------------------------------------------------------------------------
def _pd_steps(inp, kw, iters):
    """[iters, B] float32: the steps of the rule from the device's own bound (6 repetitions, under the case's weights)."""
    from asr_amd import ops
    p = inp.p
    bound = ops.sr_data_bound(inp.rot, inp.tr, inp.irot, inp.itr, inp.hw, (p.h, p.w), LAM[0], weights=kw.get("weights"), iters=6)
    taus = ops.pd_steps(bound, LAM[2], iters).cpu().numpy()
    assert taus.shape == (iters, T.BATCH) and (taus > 0).all() and np.isfinite(taus).all()
    return taus


@pytest.mark.parametrize("case", T.C_CASES, ids=_cid)
def test_c_primal_dual_is_its_single_iterations_and_each_is_the_restated_update(dev, inputs, case):
    """One call of 3 iterations against three calls of 1 iteration threaded through `state` (the duals carried in m and v),
    and each of those against sr_pd_ref.pd_update on the gradient the device itself returns for that x (a gradient-only
    launch of the fused backward with every prior off): x, p_y and p_x bit for bit."""
    from asr_amd import ops
    inp = inputs(case.shape, case.kind)
    kw, _, tv_np = inp.options(case, delta=inp.clip() if case.loss == "huber" else None)
    fwd_kw = {k: v for k, v in kw.items() if k != "tv_weights"}
    taus = _pd_steps(inp, kw, ITERS)
    whole = inp.solve(case, taus, kw, want_loss=False)
    print(f"[sr_option_shapes] {_cid(case)}: {sorted(T.instantiations(case, want_loss=False) - T.SOLVER_HELPERS)}")
    st = {}
    x, py, px = inp.x0, np.zeros_like(inp.x0), np.zeros_like(inp.x0)
    for it in range(ITERS):
        xd = ops.to_device(x)
        _, g_df = ops.sr_backward(xd, inp.residual(xd, **fwd_kw), inp.irot, inp.itr, (LAM[0], 0.0, 0.0, 0.0), ops.sr_config(), state=None)
        g_df = g_df.cpu().numpy()
        one = inp.solve(case, taus[it:it + 1], kw, x0=x, state=st, want_loss=False)
        bad = {}
        for i in range(T.BATCH):
            wy, wx = (None, None) if tv_np is None else (tv_np[0][i], tv_np[1][i])
            want = P.pd_update(PD_SR, x[i], py[i], px[i], g_df[i], taus[it, i], DUAL_RATIO, wy, wx)[:3]
            for what, g, w_ in zip(("x", "p_y", "p_x"), (one.x[i], one.m[i], one.v[i]), want):
                bad[(i, what)] = _report(f"{_cid(case)} iteration {it} image {i} {what} against the restated update", g, w_)
        assert not any(bad.values()), bad
        x, py, px = one.x, one.m, one.v
    _same(f"{_cid(case)} one call against {ITERS} calls:", whole, SimpleNamespace(x=x, m=py, v=px), ("x", "m", "v"))
    assert (py != 0).any() and (np.abs(py) < np.float32(LAM[1])).any()       # the duals: neither all zero nor all at a bound


@pytest.mark.parametrize("case", T.C_MONITORED, ids=_cid)
def test_c_primal_dual_under_a_monitor_that_never_stops(dev, inputs, case):
    """sr_backward_gather_pd_kernel<WTV, true> (with K_fwd<true,true,true> and K_gt<LOG2F, true>) against <WTV>: the same
    call without the monitor, x and both dual planes bit for bit."""
    inp = inputs(case.shape, case.kind)
    kw, _, _ = inp.options(case, delta=inp.clip() if case.loss == "huber" else None)
    taus = _pd_steps(inp, kw, ITERS)
    want = inp.solve(case._replace(monitor="off"), taus, kw)
    got = inp.solve(case, taus, kw, monitor=TRACE_ONLY)
    print(f"[sr_option_shapes] {_cid(case)}: {sorted(T.instantiations(case) - T.SOLVER_HELPERS)}")
    _same(_cid(case), got, want, ("x", "m", "v"))
    _terms_close(_cid(case), got.terms, want.terms, inp.p)
    assert np.array_equal(got.trace.iters_done.cpu().numpy(), np.full(T.BATCH, ITERS, np.int32))
    assert not np.array_equal(got.x, inp.x0) and got.m.any() and got.v.any()


@pytest.mark.parametrize("case", T.C_FROZEN, ids=_cid)
def test_c_a_frozen_image_keeps_x_and_both_duals_under_edge_weights(dev, inputs, case):
    """test_gpu_sr_pd's frozen image with edge weights on and a last chunk of one copy: image 0 gets a step so short that its
    loss stalls and it stops at the second stalled evaluation; image 1 runs on.  Each equals the unmonitored solve cut at its
    own iteration: x, p_y and p_x bit for bit."""
    inp = inputs(case.shape, case.kind)
    kw, _, _ = inp.options(case)
    iters = 6
    taus = _pd_steps(inp, kw, iters)
    taus[:, 0] = np.float32(1e-7)
    mon = dict(every=1, rel_tol=1e-3, patience=2, min_iter=0, history=True)
    got = inp.solve(case, taus, kw, monitor=mon, want_loss=False)
    done = got.trace.iters_done.cpu().numpy()
    losses = got.trace.losses(LAM)
    print(f"[sr_option_shapes] {_cid(case)}: iters_done {done.tolist()} losses {losses.T.tolist()}")
    assert np.array_equal(done, M.stop_iterations(losses, 1, 1e-3, 2, 0, num_iter=iters))
    assert done[0] == 2 and done[0] < done[1] <= iters
    plain = case._replace(monitor="off")
    for i in range(T.BATCH):
        cut = inp.solve(plain, taus[:done[i]], kw, want_loss=False)
        bad = {k: _report(f"{_cid(case)} image {i} cut at {done[i]}: {k}", getattr(got, k)[i], getattr(cut, k)[i]) for k in ("x", "m", "v")}
        assert not any(bad.values()), (i, bad)
    full = inp.solve(plain, taus, kw, want_loss=False)
    assert not np.array_equal(full.x[0], got.x[0])                               # the stop did cut image 0 short


# ---- d. the monitor with a real stop ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.D_CASES, ids=_cid)
def test_d_a_stopped_image_is_the_plain_solve_cut_at_its_iteration(dev, case):
    """f = 8 and f = 6, general transforms, a last chunk of one copy: image 0 (all-zero copies, loss 0 from the start) stops at
    its second stalled evaluation, image 1 runs on.  iters_done is the restated rule on the returned history; each image equals
    the unmonitored solve cut at its iteration (x, m, v, vhat, bit for bit); the history rows after a stop are NaN."""
    from asr_amd import ops
    inp = _Inputs(dev, case.shape, case.kind, y=T.stop_copies(case))
    x0 = ops.sr_init_target(inp.yd, inp.hw).cpu().numpy()
    assert not x0[0].any() and x0[1].any()
    inp.x0 = x0
    iters, tol, patience = 6, 1e-6, 2
    kw, _, _ = inp.options(case, delta=inp.clip() if case.loss == "huber" else None)
    alphas = _alphas("adam", iters)
    mon = dict(every=1, rel_tol=tol, patience=patience, min_iter=0, history=True)
    got = inp.solve(case, alphas, kw, monitor=mon)
    print(f"[sr_option_shapes] {_cid(case)}: {sorted(T.instantiations(case) - T.SOLVER_HELPERS)}")
    done, hist = got.trace.iters_done.cpu().numpy(), got.trace.history.cpu().numpy()
    losses = M.scalar_loss(hist, LAM)
    print(f"[sr_option_shapes] {_cid(case)}: iters_done {done.tolist()} losses {losses.T.tolist()}")
    assert np.array_equal(done, M.stop_iterations(losses, 1, tol, patience, 0, num_iter=iters))
    assert done[0] == 2 < done[1] <= iters
    assert not hist[:3, 0].any() and np.isnan(hist[3:, 0]).all()                 # evaluations 0, 1, 2: a loss of 0; then NaN
    assert not np.isnan(hist[:min(done[1] + 1, iters), 1]).any() and np.isnan(hist[done[1] + 1:, 1]).all()
    assert got.terms[0].tobytes() == hist[2, 0].tobytes()                        # the terms of the x that is returned
    plain = case._replace(monitor="off")
    for i in range(T.BATCH):
        cut = inp.solve(plain, alphas[:done[i]], kw, want_loss=False)
        bad = {k: _report(f"{_cid(case)} image {i} cut at {done[i]}: {k}", getattr(got, k)[i], getattr(cut, k)[i])
               for k in ("x", "m", "v", "vhat")}
        assert not any(bad.values()), (i, bad)
    assert not got.x[0].any() and not np.array_equal(got.x[1], x0[1])


# ---- e. the step bound -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", ["none", "batch"])
@pytest.mark.parametrize("kind", ["T0", "T2"])
@pytest.mark.parametrize("shape", ["C", "D", "A"])
def test_e_the_bound_is_the_maximum_of_the_devices_own_gradient(dev, inputs, shape, kind, weights):
    """asr_sr_data_bound_f32 (K_fwd<true,true> under L2, K_gt, the gather without a prior, the three sr_bound_* kernels) after 1
    and 3 repetitions against the same repetitions on the host in float32, the device supplying every M v through the
    unbordered forward kernel and the fused backward in gradient-only mode: bit for bit, for plane_chunk 0 and 2."""
    from asr_amd import ops
    lam_df = 1.3
    case = T.Case(shape, kind, "l2", weights, "none", "bound", "off", 0)
    assert case in T.E_CASES and case._replace(chunk=2) in T.E_CASES
    inp = inputs(shape, kind)
    p = inp.p
    kw, w_np, _ = inp.options(case)
    wd = kw.get("weights")
    zero_y = torch.zeros_like(inp.yd)

    def m_times(v):
        vd = ops.to_device(v)
        q = ops.sr_forward_residual(vd, zero_y, inp.rot, inp.tr, weights=wd)
        return ops.sr_backward(vd, q, inp.irot, inp.itr, (lam_df, 0.0, 0.0, 0.0), ops.sr_config(), state=None)[1].cpu().numpy()

    want = []
    v = np.ones((T.BATCH,) + inp.hw, np.float32)
    for _ in range(3):
        w = m_times(v)
        row = []
        for i in range(T.BATCH):                                      # sr_pd_ref.data_bound, image by image
            pos = v[i] > 0
            ratio = (w[i][pos] / v[i][pos]).max() if pos.any() else np.float32(0.0)
            row.append(np.float32(max(ratio, np.float32(0.0))))
            s = np.float32(w[i].max())
            if s > 0:
                v[i] = (w[i] / s).astype(np.float32)
        want.append(np.array(row, np.float32))
    for iters in (1, 3):
        for chunk in (0, 2):
            got = ops.sr_data_bound(inp.rot, inp.tr, inp.irot, inp.itr, inp.hw, (p.h, p.w), lam_df, weights=wd, iters=iters,
                                    cfg=ops.sr_config(plane_chunk=chunk)).cpu().numpy()
            tag = f"{_cid(case._replace(chunk=chunk))} iters={iters}: device {got.tolist()} host {want[iters - 1].tolist()};"
            assert _report(tag, got, want[iters - 1]) == 0
            assert got.dtype == np.float32 and (got > 0).all()
