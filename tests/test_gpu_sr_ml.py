"""GPU: the coupled primal-dual solve (ops.sr_solve's coupling, asr_sr_solve_ml_f32; include/asr_hip.h, "multi-label coupling")
on the three cases of tests/test_gpu_sr_pd.py, the batch made of groups of G = 3 planes that share one image's transforms, and
two cases of two groups (plain L2; Huber, weights, edge weights and L1).  Bit for bit: coupling None / 0 against the solve without the keyword; T coupled iterations against T
rounds of {one uncoupled iteration, ops.simplex_project} (owes nothing to the restatement; catches a projection that missed the
bordered copy); x and both duals against tests/sr_ml_ref.py for any plane chunking; the monitor per group.  No tolerance."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import tf_ops
from test_gpu_sr_pd import CASES as PD_CASES, DUAL_RATIO, ITERS
from test_gpu_sr_wtv import _problem

import sr_ml_ref as M
import sr_pd_ref as P

pytestmark = pytest.mark.gpu

G = 3
# the geometry, lambdas and data terms of test_gpu_sr_pd.py's cases; groups of G planes instead of its batch
CASES = {name: PD_CASES[name] + (1,) for name in PD_CASES}
CASES["16x16 two groups"] = PD_CASES["16x16"] + (2,)
CASES["32x32 two groups"] = PD_CASES["32x32"] + (2,)        # the monitor per group under Huber, weights, edge weights and L1
TWO_GROUPS = [name for name in CASES if CASES[name][-1] == 2]
# The Huber / weights / L1 cases start from 3 * x0: their x decays (from x0 itself the largest sum over a group is 0.91 after one
# iteration and 0.08 after three), and from the larger start the first iterations still end above a sum of 1, so that the sort
# branch of the projection runs -- and writes the bordered copy -- under those options too.
X0_SCALE = {"32x32": 3.0, "32x32 two groups": 3.0}


@functools.lru_cache(maxsize=None)
def _case(name):
    """Host arrays of a case and its restated coupled trajectory: computed once, shared by the tests, never changed."""
    (H, W), (h, w), n, _, lam, (loss, delta), weighted, wtv, groups = CASES[name]
    b = G * groups
    seed = 70 + list(CASES).index(name)
    y, angs, shs = _problem(seed, b, n, H, W, h, w)
    rng = np.random.default_rng(seed + 100)
    y = (y + 0.1 * rng.random(y.shape, dtype=np.float32)).astype(np.float32)
    # the members of a group are classes of ONE image: the transforms of the group's first plane
    tfs = [P.transforms(angs[i - i % G], shs[i - i % G], (H, W)) for i in range(b)]
    x0 = np.stack([tf_ops.resize_bilinear(torch.from_numpy(y[i, 0:1, :, :, None]), (H, W)).numpy()[0, :, :, 0] for i in range(b)])
    x0 = (x0 + 0.05 * rng.standard_normal(x0.shape).astype(np.float32)).astype(np.float32)
    x0 = (np.float32(X0_SCALE.get(name, 1.0)) * x0).astype(np.float32)
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
    bound_srs = [P.make_sr((lam[0], 0, 0, 0), n, (h, w), (H, W), weights=None if wts is None else wts[i]) for i in range(b)]
    taus = np.array([P.pd_tau(P.data_bound(bound_srs[i], tfs[i], 6), lam[2]) for i in range(b)], np.float32)
    traj = M.pd_solve(srs, x0, y, tfs, [taus] * ITERS, G, DUAL_RATIO, wy, wx, trajectory=True)
    return SimpleNamespace(H=H, W=W, h=h, w=w, n=n, b=b, groups=groups, lam=lam, dt=(loss, delta), y=y, tfs=tfs, x0=x0, wts=wts,
                           wy=wy, wx=wx, srs=srs, taus=taus, traj=traj)


def _cfg(chunk=0):
    from asr_amd import _lib, ops
    return ops.sr_config(_lib.OPT_PRIMAL_DUAL, c0=DUAL_RATIO, plane_chunk=chunk)


def _solve(c, alphas, x0=None, cfg=None, monitor=None, state=None, planes=None, **kw):
    """ops.sr_solve of the case (planes: a slice of its batch) -> (x, p_y, p_x) host arrays (+ the trace with a monitor); kw goes
    to ops.sr_solve as it is, so a call without `coupling` never names the keyword."""
    from asr_amd import ops
    sl = slice(None) if planes is None else planes
    tf = [ops.to_device(np.stack([t[k] for t in c.tfs[sl]]).astype(np.float32)) for k in range(4)]
    dev = tf[0].device
    if c.dt[0] != "l2" or c.wts is not None:
        kw.update(data_term=c.dt, weights=None if c.wts is None else torch.as_tensor(c.wts[sl]).to(dev).contiguous())
    if c.wy is not None:
        kw["tv_weights"] = (torch.as_tensor(c.wy[sl]).to(dev).contiguous(), torch.as_tensor(c.wx[sl]).to(dev).contiguous())
    st = {} if state is None else state
    out = ops.sr_solve(ops.to_device((c.x0 if x0 is None else x0)[sl]), ops.to_device(c.y[sl]), *tf,
                       ops.to_device(np.ascontiguousarray(alphas, np.float32)), c.lam, cfg=cfg if cfg is not None else _cfg(),
                       state=st, want_loss=False, monitor=monitor, **kw)
    arrs = (out[0].cpu().numpy(), st["m"].cpu().numpy(), st["v"].cpu().numpy())
    return arrs + ((out[2],) if monitor is not None else ())


def _same(a, b, what, zero_sign=True):
    """Two device results: the same bytes.  zero_sign=False, against the restatement: the same bytes of x, and the same values
    of the duals -- a dual clamped into a box of width 0 is +0 or -0 by fminf / fmaxf's choice between equal operands, as in
    tests/test_gpu_sr_pd.py; the projection always writes +0, so x needs no such allowance."""
    for name, p, q in zip(("x", "p_y", "p_x"), a, b):
        bad = int((p != q).sum())
        print(f"{what}: {name}: {bad} of {p.size} values differ, max |diff| {float(np.abs(p.astype(np.float64) - q).max()):.3e}")
    for name, p, q in zip(("x", "p_y", "p_x"), a, b):
        assert np.array_equal(p, q), (what, name)
        assert not (zero_sign or name == "x") or p.tobytes() == q.tobytes(), (what, name)


# ---- (a) group 0 is the solve that was there ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_coupling_none_and_zero_are_the_solve_without_the_keyword(dev, name):
    c = _case(name)
    alphas = np.tile(c.taus[None], (ITERS, 1))
    plain = _solve(c, alphas)
    _same(_solve(c, alphas, coupling=None), plain, f"{name} coupling=None")
    _same(_solve(c, alphas, coupling=0), plain, f"{name} coupling=0")
    mon = dict(every=1, rel_tol=1e-3, patience=2, min_iter=0, history=True)
    base = _solve(c, alphas, monitor=mon)
    for coupling in (None, 0):
        got = _solve(c, alphas, monitor=mon, coupling=coupling)
        _same(got[:3], base[:3], f"{name} monitored coupling={coupling}")
        assert torch.equal(got[3].iters_done, base[3].iters_done)
        assert got[3].history.cpu().numpy().tobytes() == base[3].history.cpu().numpy().tobytes()
    # and the coupling does something on this case: the coupled solve is another one
    assert not np.array_equal(_solve(c, alphas, coupling=G)[0], plain[0])


# ---- (b) chaining: owes nothing to the restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_coupled_iterations_are_rounds_of_one_iteration_and_a_projection(dev, name):
    from asr_amd import ops
    c = _case(name)
    alphas = np.tile(c.taus[None], (ITERS, 1))
    whole = _solve(c, alphas, coupling=G)
    carry = {}
    x = c.x0
    for it in range(ITERS):
        x, py, px = _solve(c, alphas[it:it + 1], x0=x, state=carry)
        x = ops.simplex_project(ops.to_device(x), G).cpu().numpy()
    _same((x, py, px), whole, f"{name} chained")
    # a projection that missed the bordered copy would leave the FIRST iteration right and the second wrong
    one = _solve(c, alphas[:1], coupling=G)
    first = ops.simplex_project(ops.to_device(_solve(c, alphas[:1])[0]), G).cpu().numpy()
    assert one[0].tobytes() == first.tobytes()


# ---- (c) the restatement, for any chunking; (e) the result is a partition --------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_one_two_and_three_coupled_iterations_are_the_restatement(dev, name):
    c = _case(name)
    alphas = np.tile(c.taus[None], (ITERS, 1))
    projected = 0
    for k in (1, 2, 3):
        for chunk in (0, 2, 1):
            got = _solve(c, alphas[:k], cfg=_cfg(chunk), coupling=G)
            _same(got, c.traj[k - 1], f"{name} after {k} chunk {chunk}", zero_sign=False)
        x = got[0].reshape(c.groups, G, c.H, c.W)
        s32 = x[:, 0].copy()
        for j in range(1, G):
            s32 = (s32 + x[:, j]).astype(np.float32)
        s64 = x.astype(np.float64).sum(axis=1)
        print(f"{name} after {k}: min {float(x.min()):.3e}, max float32 sum {float(s32.max()):.9f}, max exact sum {float(s64.max()):.9f}")
        assert float(x.min()) >= 0.0 and not np.signbit(x).any()
        assert float(s32.max()) <= 1.0 + 2e-6 and float(s64.max()) <= 1.0 + 2e-6
        projected += int((s64 > 0.999999).sum())
    assert projected > 0                                           # some pixel sat on the face sum = 1: the branch s > 1 ran
    assert (c.traj[-1][1] != 0).any()                              # and the duals did something


# ---- (d) the monitor per group --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_with_patience_zero_the_monitored_coupled_solve_is_the_unmonitored_one(dev, name):
    c = _case(name)
    alphas = np.tile(c.taus[None], (ITERS, 1))
    whole = _solve(c, alphas, coupling=G)
    got = _solve(c, alphas, coupling=G, monitor=dict(every=1, rel_tol=0.0, patience=0, min_iter=0, history=True))
    _same(got[:3], whole, f"{name} patience 0")
    assert got[3].iters_done.cpu().numpy().tolist() == [ITERS] * c.b
    hist = got[3].history.cpu().numpy()
    assert hist.shape == (ITERS, c.b, 4) and np.isfinite(hist).all()


@pytest.mark.parametrize("name", TWO_GROUPS)
def test_a_stopped_group_stops_together_and_the_other_runs_on(dev, name):
    """Two groups: the members of group 0 get steps so short that the group's loss stalls and it stops; group 1 runs on.  Every
    member of group 0 has the group's iters_done and equals the unmonitored coupled solve cut there; group 1 equals its own
    solve alone in the batch, under the same monitor."""
    c = _case(name)
    iters = 6
    taus = c.taus.copy()
    taus[:G] = 1e-7
    alphas = np.tile(taus[None], (iters, 1))
    mon = dict(every=1, rel_tol=1e-3, patience=2, min_iter=0, history=True)
    x, py, px, trace = _solve(c, alphas, coupling=G, monitor=mon)
    done = trace.iters_done.cpu().numpy()
    hist = trace.history.cpu().numpy()
    print("iters_done", done.tolist(), "losses", trace.losses(c.lam).T.tolist())
    assert len(set(done[:G].tolist())) == 1 and len(set(done[G:].tolist())) == 1
    assert 2 <= done[0] < iters and done[0] < done[G] <= iters
    # the rule, replayed on the members' own losses: the group's loss is their sum in index order
    losses = trace.losses(c.lam)
    assert M.group_stop(losses[:done[0] + 1, :G], 1e-3, 2) == done[0]
    assert np.isfinite(hist[:done[0] + 1, :G]).all() and np.isnan(hist[done[0] + 1:, :G]).all()
    cut = _solve(c, alphas[:done[0]], coupling=G)
    _same([a[:G] for a in (x, py, px)], [a[:G] for a in cut], "group 0 cut at its stop")
    full = _solve(c, alphas, coupling=G)
    assert not np.array_equal(full[0][:G], x[:G])                               # the stop did cut group 0 short
    alone = _solve(c, alphas[:, G:], coupling=G, monitor=mon, planes=slice(G, 2 * G))
    _same([a[G:] for a in (x, py, px)], alone[:3], "group 1 alone in its batch")
    assert alone[3].iters_done.cpu().numpy().tolist() == done[G:].tolist()


# ---- the C refusals ---------------------------------------------------------------------------------------------------------------
def test_the_c_entry_point_refuses_before_any_launch(dev, lib):
    import ctypes as C
    from asr_amd import _lib, ops
    c = _case("16x16")
    x = ops.to_device(c.x0)
    y = ops.to_device(c.y)
    tf = [ops.to_device(np.stack([t[k] for t in c.tfs]).astype(np.float32)) for k in range(4)]
    alphas = ops.to_device(np.tile(c.taus[None], (2, 1)))
    m, v, vhat = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x)
    dt =_lib.SrDataTerm(_lib.DF_L2, 0.1, None, 0, None, None, 0)

    def call(cfg, group, batch=c.b):
        ws_bytes = lib.asr_sr_solve_workspace_bytes_ml(batch, c.n, c.H, c.W, c.h, c.w, C.byref(cfg), 0)
        ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.float32, device=x.device)
        rc = lib.asr_sr_solve_ml_f32(x.data_ptr(), y.data_ptr(), *[t.data_ptr() for t in tf], m.data_ptr(), v.data_ptr(),
                                     vhat.data_ptr(), alphas.data_ptr(), 2, None, ws.data_ptr(), C.c_size_t(ws_bytes), batch, c.n, c.H, c.W, c.h,
                                     c.w, *c.lam, C.byref(cfg), C.byref(dt), None, group, _lib.stream_ptr())
        return rc, lib.asr_last_error()

    for group in (-1, 33):
        rc, msg = call(_cfg(), group)
        assert rc == -1 and b"group" in msg, (group, msg)
    rc, msg = call(_cfg(), 2)                                                  # 3 planes are no multiple of 2
    assert rc == -1 and b"multiple" in msg, msg
    rc, msg = call(ops.sr_config(_lib.OPT_SGD), G)
    assert rc == -2 and b"ASR_OPT_PRIMAL_DUAL" in msg, (rc, msg)                # ASR_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert np.array_equal(x.cpu().numpy(), c.x0) and not m.any() and not v.any()
    # the workspace query is the wrapped entry points'
    cfg = _cfg()
    args = (c.b, c.n, c.H, c.W, c.h, c.w, C.byref(cfg))
    assert lib.asr_sr_solve_workspace_bytes_ml(*args, 0) == lib.asr_sr_solve_workspace_bytes_dt(*args)
    assert lib.asr_sr_solve_workspace_bytes_ml(*args, 1) == lib.asr_sr_solve_workspace_bytes_mon(*args)
