"""GPU: copy reweighting (include/asr_hip.h, "copy reweighting") bit for bit against tests/sr_rw_ref.py -- the three stand-alone
entry points at every size at which the energy kernel takes another path, the weights at every copy count around a wave and a
pass of the ranking, and the reweighted solve against its host-driven segments, the CPU restatement, the monitor and the
coupling.  No tolerance anywhere."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import sr as o_sr
from test_gpu_sr_wtv import B1, B2, EPS, _adam_alphas, _problem, _tfs

import sr_dt_ref as RD
import sr_rw_ref as RW

pytestmark = pytest.mark.gpu

DELTA = 0.1
LOSSES = ("l2", "l1", ("huber", DELTA))


def _name(dt):
    return dt if isinstance(dt, str) else dt[0]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same_bits(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = int((_bits(got) != _bits(want)).sum())
    print(f"{what}: {bad} of {got.size} values differ")
    assert bad == 0, what


# ---- 1. energy, mass and apply, stand-alone ----------------------------------------------------------------------------------------
# h*w = 1, 63, 64, 255, 256, 257, 1000: one lane, one wave -+ 1, one pass -+ 1, several ragged passes
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("h,w", [(1, 1), (7, 9), (8, 8), (15, 17), (16, 16), (1, 257), (25, 40)])
def test_energy_mass_and_apply_are_the_restatement(dev, h, w, n):
    from asr_amd import ops
    b, H, W = 2, 2 * h, 2 * w
    rng = np.random.default_rng(1000 * h + 10 * w + n)
    y, angs, shs = _problem(7, b, n, H, W, h, w)
    rot, tr, _, _ = _tfs(angs, shs, H, W)
    yd = ops.to_device(y)
    xd = ops.to_device(rng.random((b, H, W), dtype=np.float32))
    u_batch = rng.random((b, n, h, w), dtype=np.float32) * 2
    u_batch[rng.random(u_batch.shape) < 0.1] = 0.0
    u_batch[1, n - 1] = 0.0                                   # one copy of all-zero weights: mass 0, inactive
    modes = {"none": None, "shared": u_batch[0], "batch": u_batch}
    for dt in LOSSES:
        _, r = ops.sr_forward_residual(xd, yd, rot, tr, data_term=("huber", DELTA), want_raw=True)
        r_np = r.cpu().numpy()
        assert (np.abs(r_np) > DELTA).any() or h * w == 1
        for mode, u in modes.items():
            ud = None if u is None else ops.to_device(u)
            tag = f"{h}x{w} n={n} {_name(dt)} {mode}"
            e, a = ops.sr_copy_energy(r, data_term=dt, weights=ud)
            e_np, a_np = RW.copy_energy(r_np, _name(dt), DELTA, u)
            _same_bits(e, e_np, tag + " energy")
            _same_bits(a, a_np, tag + " mass")
            if mode == "batch":
                assert a_np[1, n - 1] == 0.0 and e_np[1, n - 1] == 0.0
            c_np, _ = RW.copy_weights(e_np, a_np, "cauchy", 2.0)
            c_np[0, 0] = np.float32(0.37)                      # never exactly 1 everywhere, also for n = 1
            w_np, q_np = RW.apply_copy_weights(r_np, c_np, _name(dt), DELTA, u)
            w_eff, q = ops.sr_apply_copy_weights(r, ops.to_device(c_np), data_term=dt, weights=ud)
            _same_bits(w_eff, w_np, tag + " w_eff")
            _same_bits(q, q_np, tag + " q")
            q_fwd = ops.sr_forward_residual(xd, yd, rot, tr, data_term=dt, weights=w_eff)
            assert torch.equal(_as_int(q), _as_int(q_fwd)), tag + " q against the forward launch with weights = w_eff"


def _as_int(t):
    return t.view(torch.int32)


# ---- 2. the weights ---------------------------------------------------------------------------------------------------------------
def _energy_rows(n, seed):
    """Six images of n copies: distinct energies; ties, exact zeros and inactive copies (mass 0, NaN, inf) among them; more than
    half zeros (s = 0); all inactive; uneven masses; one huge energy (t*t overflows towards c = 0)."""
    rng = np.random.default_rng(seed)
    e = rng.uniform(0.01, 50.0, (6, n))
    a = np.full((6, n), 64.0)
    e[1] = rng.integers(0, 4, n).astype(np.float64)                   # ties and zeros
    for j, (ev, av) in enumerate(((3.0, 0.0), (np.nan, 64.0), (np.inf, 64.0), (0.0, 0.0))):
        if n > 4:
            e[1, (5 * j + 2) % n], a[1, (5 * j + 2) % n] = ev, av
    e[2, :n // 2 + 1] = 0.0
    a[3] = 0.0
    a[4] = rng.uniform(0.5, 200.0, n)
    if n > 1:
        a[4, n - 1] = 0.0
    e[5, 0] = 1e300
    return e, a


@pytest.mark.parametrize("n", [1, 2, 3, 4, 63, 64, 65, 257, 640])
def test_copy_weights_are_the_restatement(dev, n):
    from asr_amd import ops
    e, a = _energy_rows(n, 40 + n)
    ed, ad = ops.to_device(e, torch.float64), ops.to_device(a, torch.float64)
    for kind in RW.KINDS:
        for kappa in (0.5, 2.0, 1e30):
            c, s = ops.sr_copy_weights(ed, ad, kind, kappa, want_scale=True)
            c_np, s_np = RW.copy_weights(e, a, kind, kappa)
            _same_bits(c, c_np, f"n={n} {kind} kappa={kappa} c")
            _same_bits(s, s_np, f"n={n} {kind} kappa={kappa} scale")
            if kappa == 1e30:                                     # every active copy but the one whose t*t overflows
                act = (a[:5] > 0) & np.isfinite(e[:5] / np.where(a[:5] > 0, a[:5], 1.0))
                assert (c_np[:5][act] == 1.0).all() and (c_np[:5][~act] == 0.0).all() and c_np[5, 0] == (1.0 if n == 1 else 0.0)
    assert (RW.copy_weights(e, a, "hard", 0.5)[0][0] == 0.0).any() or n == 1
    assert (RW.copy_weights(e, a, "cauchy", 2.0)[0][3] == 0.0).all() and s_np[2] == 0.0


# ---- 3. the solve ---------------------------------------------------------------------------------------------------------------
ITERS = 6
RW_PARAMS = dict(kappa=2.0, every=2, start=1, history=True)
POINTS = [1, 3, 5]
LR = 1e-2
# name -> (H, W), (h, w), n, batch, lambdas, data term, base weights, edge weights
CASES = {
    "16x16": ((16, 16), (8, 8), 4, 2, (1.0, 0.05, 0.0, 0.0), "l2", False, False),
    "12x136": ((12, 136), (6, 68), 5, 2, (1.0, 0.3, 0.7, 0.0), "l2", False, False),
    "32x32": ((32, 32), (8, 8), 4, 2, (1.0, 0.3, 0.7, 0.05), ("huber", DELTA), True, True),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """Host arrays of a case: computed once, shared by the tests, never changed.  The last copy of every image is replaced by
    another image's blob, so that the copy weights differ from 1."""
    (H, W), (h, w), n, b, lam, dt, weighted, wtv = CASES[name]
    seed = 90 + list(CASES).index(name)
    y, angs, shs = _problem(seed, b, n, H, W, h, w)
    rng = np.random.default_rng(seed + 100)
    y = (y + 0.1 * rng.random(y.shape, dtype=np.float32)).astype(np.float32)
    y[:, n - 1] = (rng.random((b, h, w)) < 0.5).astype(np.float32)
    wts = None
    if weighted:
        wts = rng.random((b, n, h, w), dtype=np.float32)
        wts[:, 0, :2] = 0.0
    wy = wx = None
    if wtv:
        wy, wx = (rng.random((b, H, W), dtype=np.float32) for _ in range(2))
    return SimpleNamespace(name=name, H=H, W=W, h=h, w=w, n=n, b=b, lam=lam, dt=dt, y=y, angs=angs, shs=shs, wts=wts, wy=wy, wx=wx)


def _device(c):
    from asr_amd import ops
    tfs = _tfs(c.angs, c.shs, c.H, c.W)
    dev = tfs[0].device
    d = SimpleNamespace(tfs=tfs, y=ops.to_device(c.y), u=None if c.wts is None else ops.to_device(c.wts), tvw=None)
    if c.wy is not None:
        d.tvw = (ops.to_device(c.wy), ops.to_device(c.wx))
    d.x0 = ops.sr_init_target(d.y, (c.H, c.W))
    d.dev = dev
    return d


def _rule(c, d, rule, chunk=0):
    """(cfg, alphas [ITERS, b] on the device) of AMSGrad (lr 1e-2) or the primal-dual rule (its own step, from the base weights)."""
    from asr_amd import _lib, ops
    if rule == "amsgrad":
        return (ops.sr_config(_lib.OPT_ADAM, True, np.float32(1) - B1, np.float32(1) - B2, EPS, plane_chunk=chunk),
                ops.to_device(_adam_alphas(ITERS, c.b, lr=LR)))
    cfg = ops.sr_config(_lib.OPT_PRIMAL_DUAL, c0=ops.PD_DUAL_RATIO, plane_chunk=chunk)
    bound = ops.sr_data_bound(*d.tfs, (c.H, c.W), (c.h, c.w), c.lam[0], weights=d.u, iters=6, cfg=cfg)
    return cfg, ops.pd_steps(bound, c.lam[2], ITERS)


def _solve(c, d, cfg, alphas, x=None, weights="base", state=None, **kw):
    """ops.sr_solve on a copy of x (default: the start) -> its return value; the optimiser slots end up in `state`."""
    from asr_amd import ops
    x = (d.x0 if x is None else x).clone()
    w = d.u if isinstance(weights, str) else weights
    return ops.sr_solve(x, d.y, *d.tfs, alphas.contiguous(), c.lam, cfg=cfg, state={} if state is None else state, want_loss=False,
                        tv_weights=d.tvw, data_term=c.dt, weights=w, **kw)


def _reweigh(c, d, x, w_cur, kind):
    """The host-driven reweighting at x: the forward call with the raw residual, then the three stand-alone entry points."""
    from asr_amd import ops
    _, r = ops.sr_forward_residual(x, d.y, d.tfs[0], d.tfs[1], data_term=c.dt, weights=w_cur, want_raw=True)
    e, a = ops.sr_copy_energy(r, data_term=c.dt, weights=d.u)
    cw = ops.sr_copy_weights(e, a, kind, RW_PARAMS["kappa"])
    w_eff, _ = ops.sr_apply_copy_weights(r, cw, data_term=c.dt, weights=d.u)
    return cw, w_eff


def _equal(got, want, what):
    for k, (p, q) in enumerate(zip(got, want)):
        assert p.shape == q.shape and torch.equal(p.view(torch.int32), q.view(torch.int32)), (what, k)


SLOTS = {"amsgrad": ("m", "v", "vhat"), "pd": ("m", "v")}


@pytest.mark.parametrize("kind", RW.KINDS)
@pytest.mark.parametrize("rule", ["amsgrad", "pd"])
@pytest.mark.parametrize("name", list(CASES))
def test_the_solve_is_its_host_driven_segments(dev, name, rule, kind):
    c = _case(name)
    d = _device(c)
    cfg, alphas = _rule(c, d, rule)
    # the segments: [0, 1) under the base weights, then [1, 3), [3, 5), [5, 6), each after a reweighting at its first iteration
    x, st, w_cur, hist = d.x0, {}, d.u, []
    cw = torch.ones((c.b, c.n), device=d.dev)
    for first, last in zip([0] + POINTS, POINTS + [ITERS]):
        if first in POINTS:
            cw, w_cur = _reweigh(c, d, x, w_cur, kind)
            hist.append(cw)
        x = _solve(c, d, cfg, alphas[first:last], x=x, weights=w_cur, state=st)[0]
    want = [x] + [st[k] for k in SLOTS[rule]] + [cw, torch.stack(hist)]
    assert not bool((cw == 1).all()), "the replaced copy did not move the weights"
    for chunk in (0, 1, 2):
        cfg_c, _ = _rule(c, d, rule, chunk)
        st2 = {}
        out = _solve(c, d, cfg_c, alphas, state=st2, reweight=dict(RW_PARAMS, kind=kind))
        assert len(out) == 3 and out[2].iters == POINTS
        got = [out[0]] + [st2[k] for k in SLOTS[rule]] + [out[2].weights, out[2].history]
        _equal(got, want, f"{name} {rule} {kind} chunk {chunk}")
    # and the reweighting did something: the plain solve is another one
    assert not torch.equal(_solve(c, d, cfg, alphas)[0], x)


@pytest.mark.parametrize("kind", RW.KINDS)
def test_the_16x16_case_is_the_restatements_trajectory(dev, kind):
    c = _case("16x16")
    d = _device(c)
    cfg, alphas = _rule(c, d, "amsgrad")
    for k in (2, 4, ITERS):
        out = _solve(c, d, cfg, alphas[:k], reweight=dict(RW_PARAMS, kind=kind))
        for i in range(c.b):
            ref = _restated(c.name, i, kind, k)
            _same_bits(out[0][i], ref.trajectory[k - 1][:, :, 0], f"{kind} image {i} x after {k}")
            _same_bits(out[2].weights[i], ref.copy_weights, f"{kind} image {i} copy weights after {k}")
            _same_bits(out[2].history[:, i], ref.history, f"{kind} image {i} history after {k}")


@functools.lru_cache(maxsize=None)
def _restated(name, i, kind, iters):
    """The CPU restatement's reweighted AMSGrad solve of image i of a case: computed once, shared, never changed."""
    c = _case(name)
    opt = o_sr.Optimizer("adam", LR, amsgrad=True)
    sr = RW.ReweightedSuperresolution(*c.lam, num_iter=iters, num_aug=c.n, optimizer=opt, feature_size=(c.h, c.w),
                                      output_size=(c.H, c.W), df_loss=_name(c.dt), df_delta=DELTA,
                                      weights=None if c.wts is None else c.wts[i], rw_kind=kind, rw_kappa=RW_PARAMS["kappa"],
                                      rw_every=RW_PARAMS["every"], rw_start=RW_PARAMS["start"])
    sr.augmented_superresolution(c.y[i][..., None], c.angs[i], c.shs[i], return_trajectory=True)
    return sr


@pytest.mark.parametrize("name", list(CASES))
def test_a_start_beyond_the_last_iteration_is_the_unreweighted_solve(dev, name):
    c = _case(name)
    d = _device(c)
    for rule in ("amsgrad", "pd"):
        cfg, alphas = _rule(c, d, rule)
        st0, st1 = {}, {}
        plain = _solve(c, d, cfg, alphas, state=st0)
        for start in (ITERS, ITERS + 7):
            out = _solve(c, d, cfg, alphas, state=st1, reweight=dict(kind="cauchy", kappa=2.0, every=1, start=start, history=True))
            _equal([out[0]] + [st1[k] for k in SLOTS[rule]], [plain[0]] + [st0[k] for k in SLOTS[rule]], f"{name} {rule} start {start}")
            assert bool((out[2].weights == 1).all()) and out[2].iters == [] and tuple(out[2].history.shape) == (0, c.b, c.n)
            st1 = {}


@pytest.mark.parametrize("kind", RW.KINDS)
def test_the_monitors_term_0_is_the_weighted_data_term(dev, kind):
    """Trace only (patience 0): the solve is the unmonitored reweighted solve, and term 0 of every evaluation is the data term
    under the weights in force at that iteration -- after its reweighting, where there was one."""
    c = _case("16x16")
    d = _device(c)
    cfg, alphas = _rule(c, d, "amsgrad")
    rw = dict(RW_PARAMS, kind=kind)
    plain = _solve(c, d, cfg, alphas, reweight=rw)
    out = _solve(c, d, cfg, alphas, reweight=rw, monitor=dict(every=1, rel_tol=0.0, patience=0, min_iter=0, history=True))
    assert len(out) == 4
    _equal([out[0], out[3].weights, out[3].history], [plain[0], plain[2].weights, plain[2].history], "trace only")
    assert out[2].iters_done.cpu().numpy().tolist() == [ITERS] * c.b
    hist = out[2].history.cpu().numpy()
    for i in range(c.b):
        ref = _restated(c.name, i, kind, ITERS)
        want = np.array([ref.data_terms[it] for it in range(ITERS)], dtype=np.float64)
        _same_bits(hist[:, i, 0].copy(), want, f"{kind} image {i} term 0")
        # the reweighting changed the term at its iteration: under the weights of before it is another number
    assert not np.array_equal(hist[:, :, 0], _solve(c, d, cfg, alphas, monitor=dict(every=1, rel_tol=0.0, patience=0, min_iter=0,
                                                                                  history=True))[2].history.cpu().numpy()[:, :, 0])


@pytest.mark.parametrize("rule", ["amsgrad", "pd"])
@pytest.mark.parametrize("name", list(CASES))
def test_a_stopped_image_is_the_reweighted_solve_cut_there(dev, name, rule):
    """Image 0 gets steps so short that its loss stalls: with patience 1 it stops at iteration 2 -- the evaluation at the
    reweighting iteration 1 re-armed the rule and counts as an improvement.  It equals the same reweighted solve cut there and
    is never reweighted again; image 1 runs on."""
    c = _case(name)
    d = _device(c)
    cfg, alphas = _rule(c, d, rule)
    alphas = alphas.clone()
    alphas[:, 0] = 1e-9
    rw = dict(RW_PARAMS, kind="cauchy")
    mon = dict(every=1, rel_tol=1e-3, patience=1, min_iter=0, history=True)
    st = {}
    out = _solve(c, d, cfg, alphas, state=st, reweight=rw, monitor=mon)
    done = out[2].iters_done.cpu().numpy().tolist()
    print(name, rule, "iters_done", done, "losses", out[2].losses(c.lam).T.tolist())
    assert done[0] == 2, done
    hist = out[3].history.cpu().numpy()
    for i in range(c.b):
        k = done[i]
        stc = {}
        cut = _solve(c, d, cfg, alphas[:k], state=stc, reweight=rw)
        _equal([out[0][i]] + [st[s][i] for s in SLOTS[rule]] + [out[3].weights[i]],
               [cut[0][i]] + [stc[s][i] for s in SLOTS[rule]] + [cut[2].weights[i]], f"{name} {rule} image {i} cut at {k}")
        rows = len([p for p in POINTS if p < k])
        assert np.array_equal(_bits(hist[:rows, i].copy()), _bits(cut[2].history.cpu().numpy()[:, i].copy()))
        assert np.isnan(hist[rows:, i]).all()


@pytest.mark.parametrize("kind", RW.KINDS)
@pytest.mark.parametrize("name", list(CASES))
def test_the_coupled_solve_is_a_loop_of_single_iterations(dev, name, kind):
    """coupling = 2: one-iteration uncoupled solves carrying the duals, the reweighting launches before the iterations that
    reweight, the projection after every one."""
    from asr_amd import ops
    c = _case(name)
    d = _device(c)
    cfg, alphas = _rule(c, d, "pd")
    x, st, w_cur, hist = d.x0 * 2.0, {}, d.u, []                  # from twice the start the two planes' sum exceeds 1 somewhere
    x0 = x.clone()
    cw = torch.ones((c.b, c.n), device=d.dev)
    projected = 0
    for it in range(ITERS):
        if it in POINTS:
            cw, w_cur = _reweigh(c, d, x, w_cur, kind)
            hist.append(cw)
        x = _solve(c, d, cfg, alphas[it:it + 1], x=x, weights=w_cur, state=st)[0]
        projected += int((x.reshape(c.b // 2, 2, -1).clamp(min=0).sum(1) > 1).sum())
        x = ops.simplex_project(x, 2)
    assert projected > 0
    want = [x, st["m"], st["v"], cw, torch.stack(hist)]
    for chunk in (0, 1):
        cfg_c, _ = _rule(c, d, "pd", chunk)
        st2 = {}
        out = _solve(c, d, cfg_c, alphas, x=x0, state=st2, reweight=dict(RW_PARAMS, kind=kind), coupling=2)
        _equal([out[0], st2["m"], st2["v"], out[2].weights, out[2].history], want, f"{name} coupled {kind} chunk {chunk}")


def test_rw_null_is_the_wrapped_entry_point(dev, lib):
    """asr_sr_solve_rw_f32 with rw == NULL against ops.sr_solve without the keyword (asr_sr_solve_dt_f32 / _mon_f32)."""
    import ctypes as C
    from asr_amd import _lib, ops
    c = _case("32x32")
    d = _device(c)
    cfg, alphas = _rule(c, d, "amsgrad")
    st = {}
    plain = _solve(c, d, cfg, alphas, state=st)
    x = d.x0.clone()
    m, v, vhat = (torch.zeros_like(x) for _ in range(3))
    dt = ops._data_term(c.dt, d.u, d.y, ops._tv_weights(d.tvw, x, "test"), "test", always=True)
    nbytes = lib.asr_sr_solve_workspace_bytes_ml(c.b, c.n, c.H, c.W, c.h, c.w, C.byref(cfg), 0)
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=x.device)
    _lib.call("asr_sr_solve_rw_f32", x.data_ptr(), d.y.data_ptr(), *[t.data_ptr() for t in d.tfs], m.data_ptr(), v.data_ptr(),
              vhat.data_ptr(), alphas.data_ptr(), ITERS, None, ws.data_ptr(), C.c_size_t(nbytes), c.b, c.n, c.H, c.W, c.h, c.w,
              *[float(t) for t in c.lam], C.byref(cfg), C.byref(dt), None, 0, None, _lib.stream_ptr())
    _equal([x, m, v, vhat], [plain[0], st["m"], st["v"], st["vhat"]], "rw NULL")
