"""The primal-dual rule without a device (include/asr_hip.h, "primal-dual"): its restatement tests/sr_pd_ref.py on what the
rule rests on -- the data-gradient map is entrywise non-negative and the bound is one on its spectral radius, from above and
tightening -- and on what it is for (a lower loss in 60 iterations than AMSGrad reaches in 150); every refusal of the C entry
points through ctypes (null or fake device pointers: refused before any launch); the host checks of the upper layers."""
import ctypes as C

import numpy as np
import pytest

from asr_amd.ops import check_pd                   # the feature itself: nothing below runs without it
import sr_dt_ref as RD
import sr_pd_ref as P

FAKE = 1 << 20                      # non-null, never dereferenced on the host: every call below is refused before a launch
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
DIMS = (1, 2, 8, 8, 4, 4)
LAM = (1.0, 0.05, 0.0, 0.0)


# ---- 1. the map and its bound ------------------------------------------------------------------------------------------------
def test_the_data_gradient_map_is_nonnegative_and_the_bound_is_one_from_above():
    H, h, n = 8, 4, 3
    rng = np.random.default_rng(0)
    angles = rng.uniform(-0.3, 0.3, n).astype(np.float32)
    shifts = rng.uniform(-1.0, 1.0, (n, 2)).astype(np.float32)
    angles[0], shifts[0] = 0, 0
    tfs = P.transforms(angles, shifts, (H, H))
    for weights in (None, rng.random((n, h, h), dtype=np.float32)):
        sr = P.make_sr((1.0, 0, 0, 0), n, (h, h), (H, H), weights=weights)
        M = np.zeros((H * H, H * H), np.float64)
        for j in range(H * H):
            e = np.zeros(H * H, np.float32)
            e[j] = 1.0
            M[:, j] = P.apply_m(sr, e.reshape(H, H), tfs).reshape(-1)
        assert (M >= 0).all() and M.max() > 0
        rho = np.abs(np.linalg.eigvals(M)).max()
        bounds = [float(b) for b in P.data_bound(sr, tfs, 6, all_iters=True)]
        print("weights" if weights is not None else "no weights", "rho", rho, "bounds", bounds)
        assert all(b >= rho for b in bounds)
        assert all(later <= earlier for earlier, later in zip(bounds, bounds[1:]))
        assert float(P.data_bound(sr, tfs, 6)) == bounds[-1] and float(P.data_bound(sr, tfs, 1)) == bounds[0]


# ---- 2. what it is for ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1])
def test_sixty_iterations_end_below_amsgrads_hundred_and_fifty(seed):
    """Measured on the CPU restatement: 24.14 < 24.89 (seed 0) and 22.49 < 23.23 (seed 1)."""
    case = RD.make_case(seed, n_bad=0)
    (n, hw, HW), samples, tfs, x0 = P.case_problem(case)
    adam = P.scalar_loss(LAM, case, RD.solve_case(case, "l2"))
    sr = P.make_sr(LAM, n, hw, HW)
    tau = P.pd_tau(P.data_bound(sr, tfs, 6), LAM[2])
    losses = [P.scalar_loss(LAM, case, x) for x, _, _ in P.pd_solve(sr, x0, samples, tfs, [tau] * 60, trajectory=True)]
    print(f"seed {seed}: AMSGrad 150 it. {adam:.4f}; primal-dual 20 it. {losses[19]:.4f}, 60 it. {losses[-1]:.4f}; tau {tau!r}")
    assert np.isfinite(losses).all()
    assert losses[-1] < adam


# ---- 3. the library ------------------------------------------------------------------------------------------------------------
def _cfg(opt=None, c0=1.0 / 16.0, **kw):
    from asr_amd import _lib, ops
    return ops.sr_config(_lib.OPT_PRIMAL_DUAL if opt is None else opt, False, c0, 0.0, 0.0, **kw)


def _dt(loss=0, delta=0.1, weights=None, shared=0, wy=None, wx=None, tv_shared=0):
    from asr_amd import _lib
    return _lib.SrDataTerm(loss, delta, weights, shared, wy, wx, tv_shared)


def _solves(lib, cfg, dt=None, dev=FAKE, x=FAKE, ws_bytes=1 << 30):
    """The status of the four solve entry points for one cfg (dt: for the two that take one)."""
    from asr_amd import _lib
    head = (x, dev, dev, dev, dev, dev, dev, dev, dev, dev, 1, None, dev, ws_bytes, *DIMS, 1.0, 0.3, 0.0, 0.0, C.byref(cfg))
    dt = _dt() if dt is None else dt
    mon = _lib.SrMonitor(1, 1e-4, 3, 0, None, FAKE)
    return dict(cfg=lib.asr_sr_solve_cfg_f32(*head, None), wtv=lib.asr_sr_solve_wtv_f32(*head, dev, dev, 0, None),
                dt=lib.asr_sr_solve_dt_f32(*head, C.byref(dt), None), mon=lib.asr_sr_solve_mon_f32(*head, C.byref(dt), C.byref(mon), None))


def test_the_library_exports_the_rule_and_keeps_its_abi(lib):
    from asr_amd import _lib, ops
    assert _lib.OPT_PRIMAL_DUAL == 5 and lib.asr_abi_version() == _lib.ABI_VERSION == 3
    assert hasattr(lib, "asr_sr_data_bound_f32") and hasattr(lib, "asr_sr_data_bound_workspace_bytes")
    b, n, H, W, h, w = 2, 3, 8, 8, 4, 4
    for fn in ("asr_sr_solve_workspace_bytes_cfg", "asr_sr_solve_workspace_bytes_dt", "asr_sr_solve_workspace_bytes_mon"):
        size = getattr(lib, fn)
        adam = size(b, n, H, W, h, w, C.byref(ops.sr_config()))
        for opt in (_lib.OPT_SGD, _lib.OPT_ADAGRAD, _lib.OPT_ADADELTA, _lib.OPT_ADAMAX):       # unchanged: none depends on the rule
            assert size(b, n, H, W, h, w, C.byref(ops.sr_config(opt))) == adam
        assert size(b, n, H, W, h, w, C.byref(_cfg())) == adam + 4 * 2 * b * H * W             # the second pair of dual planes
        assert size(b, n, H, W, h, w, C.byref(_cfg(plane_chunk=1))) == \
            size(b, n, H, W, h, w, C.byref(ops.sr_config(plane_chunk=1))) + 4 * 2 * b * H * W
    # the sizes the other optimisers have always had (tests/test_cabi_symbols.py pins the same numbers)
    assert lib.asr_sr_solve_workspace_bytes(2, 3, 8, 8, 4, 4) == 4 * (2 * 3 * 16 + 2 * 2 * 64 + (2 * 3 + 2) * 12 * 72 + 2)
    assert lib.asr_sr_solve_workspace_bytes_cfg(2, 3, 8, 8, 4, 4, C.byref(ops.sr_config())) == lib.asr_sr_solve_workspace_bytes(2, 3, 8, 8, 4, 4)
    pe = 12 * 72
    assert lib.asr_sr_data_bound_workspace_bytes(b, n, H, W, h, w, None) == \
        4 * (2 * b * n * h * w + 3 * b * H * W + (b * n + b) * pe) + 4 * b + 4 * 2 * 64 * b
    assert lib.asr_sr_data_bound_workspace_bytes(b, n, H, W, h, w, C.byref(ops.sr_config(plane_chunk=1))) == \
        4 * (2 * b * n * h * w + 3 * b * H * W + (b * 1 + b) * pe) + 4 * b + 4 * 2 * 64 * b
    assert lib.asr_sr_data_bound_workspace_bytes(0, n, H, W, h, w, None) == 0


def test_solve_refusals(lib):
    from asr_amd import _lib
    for dev in (FAKE, None):                       # None: the refusal came before any launch could have read a pointer
        x = FAKE if dev else None
        # the bilateral-TV prior
        got = _solves(lib, _cfg(use_btv=True), dev=dev, x=x)
        assert set(got.values()) == {UNSUPPORTED if dev else INVALID}, got
        if dev:
            assert b"bilateral TV" in lib.asr_last_error()
        # the dual ratio
        for c0 in (0.0, -0.01, 0.0626, 0.5, float("nan"), float("inf"), float("-inf")):
            got = _solves(lib, _cfg(c0=c0), dev=dev, x=x)
            assert set(got.values()) == {INVALID}, (c0, got)
            if dev:
                assert b"dual ratio" in lib.asr_last_error()
    # the L1 data term is not smooth; Huber and weights pass these checks (and are then refused for the short workspace)
    l1 = _solves(lib, _cfg(), dt=_dt(loss=_lib.DF_L1))
    assert l1["dt"] == l1["mon"] == UNSUPPORTED and b"smooth" in lib.asr_last_error()
    for dt in (_dt(loss=_lib.DF_HUBER, delta=0.1), _dt(weights=FAKE), _dt(loss=_lib.DF_HUBER, delta=0.2, weights=FAKE, wy=FAKE, wx=FAKE)):
        got = _solves(lib, _cfg(), dt=dt, ws_bytes=16)
        assert got["dt"] == got["mon"] == WORKSPACE, got
    # the largest ratio itself and a tiny one are accepted
    for c0 in (1.0 / 16.0, 1e-6):
        assert set(_solves(lib, _cfg(c0=c0), ws_bytes=16).values()) == {WORKSPACE}
    # the slots: m and v are the dual planes, vhat is not needed
    head = lambda m, v: (FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, m, v, None, FAKE, 1, None, FAKE, 16, *DIMS, 1.0, 0.3, 0.0, 0.0,
                         C.byref(_cfg()), None)
    assert lib.asr_sr_solve_cfg_f32(*head(FAKE, FAKE)) == WORKSPACE
    assert lib.asr_sr_solve_cfg_f32(*head(None, FAKE)) == INVALID and b"slot" in lib.asr_last_error()
    assert lib.asr_sr_solve_cfg_f32(*head(FAKE, None)) == INVALID
    # an optimiser past the new one is still unknown
    assert set(_solves(lib, _cfg(opt=6)).values()) == {INVALID} and b"unknown optimizer" in lib.asr_last_error()
    # the workspace: one byte short of the rule's own size
    need = lib.asr_sr_solve_workspace_bytes_cfg(*DIMS, C.byref(_cfg()))
    assert _solves(lib, _cfg(), ws_bytes=need - 1)["cfg"] == WORKSPACE
    adam_need = lib.asr_sr_solve_workspace_bytes_cfg(*DIMS, C.byref(_cfg(opt=_lib.OPT_ADAM)))
    assert need > adam_need and _solves(lib, _cfg(), ws_bytes=adam_need)["cfg"] == WORKSPACE


def test_the_one_step_entry_points_refuse_the_rule(lib):
    for dev in (FAKE, None):
        x_new = dev and dev + 4096                     # x_new must not alias x
        args = (dev, x_new, dev, dev, dev, dev, dev, dev, dev, dev, *DIMS, 1.0, 0.3, 0.0, 0.0, C.byref(_cfg()))
        # optimizer 5 is to them what it always was, an unknown one (tests/test_sr_update_host.py pins the message); null
        # pointers are refused first, as for every rule
        assert lib.asr_sr_backward_cfg_f32(*args, None) == INVALID
        assert lib.asr_sr_backward_wtv_f32(*args, dev, dev, 0, None) == INVALID
        if dev:
            assert b"unknown optimizer 5" in lib.asr_last_error()
    # gradient only (no x_new) is a one-step call too
    args = (FAKE, None, FAKE, FAKE, FAKE, None, None, None, None, FAKE, *DIMS, 1.0, 0.3, 0.0, 0.0, C.byref(_cfg()))
    assert lib.asr_sr_backward_cfg_f32(*args, None) == INVALID and b"unknown optimizer 5" in lib.asr_last_error()
    # the loss terms read the prior alone and take the rule's config (null pointers are their first refusal)
    assert lib.asr_sr_loss_terms_cfg_f64(None, None, None, *DIMS, C.byref(_cfg()), None) == INVALID
    assert b"null pointer" in lib.asr_last_error()


def _bound(lib, iters=6, lambda_df=1.0, dev=FAKE, out=FAKE, ws=FAKE, ws_bytes=1 << 30, dims=DIMS, cfg=None, weights=None):
    return lib.asr_sr_data_bound_f32(out, dev, dev, dev, dev, weights, 0, iters, ws, ws_bytes, *dims, lambda_df,
                                     C.byref(cfg) if cfg is not None else None, None)


def test_bound_refusals(lib):
    from asr_amd import ops
    assert _bound(lib, out=None) == INVALID and b"null pointer" in lib.asr_last_error()
    assert _bound(lib, dev=None) == INVALID and b"null pointer" in lib.asr_last_error()
    assert _bound(lib, ws=None) == INVALID and b"null pointer" in lib.asr_last_error()
    for iters in (0, -1, 65, 2 ** 31 - 1):
        assert _bound(lib, iters=iters) == INVALID and b"iters" in lib.asr_last_error()
    for lam in (-1.0, float("nan"), float("inf")):
        assert _bound(lib, lambda_df=lam) == INVALID and b"lambda_df" in lib.asr_last_error()
    assert _bound(lib, dims=(0, 2, 8, 8, 4, 4)) == INVALID
    assert _bound(lib, dims=(1, 2, 12, 12, 4, 4)) == UNSUPPORTED              # an odd factor, as for the solves
    assert _bound(lib, cfg=ops.sr_config(plane_chunk=-1)) == INVALID and b"plane_chunk" in lib.asr_last_error()
    need = lib.asr_sr_data_bound_workspace_bytes(*DIMS, None)
    assert _bound(lib, ws_bytes=need - 1) == WORKSPACE and b"workspace" in lib.asr_last_error()
    for iters in (1, 64):                                                        # the ends of the range pass the check
        assert _bound(lib, iters=iters, ws_bytes=need - 1) == WORKSPACE


# ---- 4. the upper layers -------------------------------------------------------------------------------------------------------
def test_check_pd_and_the_optimizer():
    from asr_amd import _lib, ops
    from asr_amd.superresolution_scripts.optimizer import Optimizer
    assert check_pd() == (6, 1.0 / 16.0) and check_pd(np.int64(1), 0.01) == (1, 0.01) and check_pd(64)[0] == 64
    for bad in (0, 65, -1, 1.5, True, None, "6"):
        with pytest.raises(ValueError, match="bound iterations"):
            check_pd(bad)
    for bad in (0.0, -0.1, 0.07, float("nan"), float("inf"), None, "x", True):
        with pytest.raises(ValueError, match="dual ratio"):
            check_pd(6, bad)
    opt = Optimizer("primal_dual")
    assert opt.optimizer.kind == _lib.OPT_PRIMAL_DUAL and opt.optimizer.bound_iters == 6
    cfg = opt.optimizer.config()
    assert (cfg.optimizer, cfg.c0, cfg.prior) == (5, 1.0 / 16.0, _lib.PRIOR_TV)
    cfg = Optimizer("primal_dual", pd_bound_iters=3, pd_dual_ratio=1 / 32).optimizer.config()
    assert cfg.c0 == 1.0 / 32.0
    with pytest.raises(ValueError, match="lr_scheduler"):
        Optimizer("primal_dual", lr_scheduler=True)
    with pytest.raises(ValueError, match="TV prior"):
        opt.optimizer.config(use_btv=True)
    with pytest.raises(ValueError):
        Optimizer("primal_dual", pd_bound_iters=0)
    # the step counter advances by num_iter per solve like the others
    opt.schedule_alphas(7)
    assert opt.optimizer.iterations == 7
    # the other optimisers are what they were
    assert Optimizer("adam", 1e-3, amsgrad=True).optimizer.config().optimizer == _lib.OPT_ADAM
    assert ops.sr_config(_lib.OPT_PRIMAL_DUAL, c0=1 / 16).optimizer == 5


def test_the_scripts_list_the_flag():
    import os
    import subprocess
    import sys
    from conftest import ROOT
    for script in ("validate_labelmap.py", "validate_classes.py", "SR_single_class.py"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script), "--help"], capture_output=True, text=True, cwd=ROOT)
        assert r.returncode == 0, r.stderr
        assert "--sr_optimizer" in r.stdout and "--pd_bound_iters" in r.stdout and "primal_dual" in r.stdout, script
