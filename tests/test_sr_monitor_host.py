"""The convergence monitor without a device: the stop rule's restatement (tests/sr_mon_ref.py) on known answers, the host
checks of every layer, the C entry point's refusals through ctypes (null or fake device pointers: refused before any launch),
the iterations CSV and the scripts' flags."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

from asr_amd.ops import check_sr_monitor          # the feature itself: nothing below runs without it
import sr_dt_ref as RD
import sr_mon_ref as M

FAKE = 1 << 20                      # non-null, never dereferenced on the host: every call below is refused before a launch
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
DIMS = (1, 2, 8, 8, 4, 4)


# ---- the rule ----------------------------------------------------------------------------------------------------------------
def test_a_strictly_decreasing_trace_never_stops():
    trace = 100.0 * 0.9 ** np.arange(30)
    assert M.stop_iterations(trace, 1, 1e-3, 3, 0) == 30
    assert M.stop_iterations(trace, 4, 1e-3, 1, 0) == 120 and M.stop_iterations(trace, 4, 1e-3, 1, 0, num_iter=117) == 117
    # ... unless it falls by less than the tolerance asks: 90 and 81 are not below 100 - 20, 72.9 is (and resets the stall)
    assert M.stop_iterations(trace, 1, 0.2, 2, 0) == 2 and M.stop_iterations(trace, 1, 0.2, 3, 0) == 30


def test_a_constant_trace_stops_at_evaluation_patience():
    for patience in (1, 2, 5):
        for every in (1, 3):
            assert M.stop_iterations(np.full(20, 7.0), every, 1e-4, patience, 0) == patience * every
    assert M.stop_iterations(np.full(20, 7.0), 1, 1e-4, 0, 0) == 20     # patience 0: never
    assert M.stop_iterations(np.zeros(20), 1, 1e-4, 2, 0) == 2          # a loss of 0 from the start
    assert M.stop_iterations(np.full(20, -3.0), 1, 1e-4, 2, 0) == 2     # |best| in the tolerance: a negative loss too


def test_a_rise_followed_by_a_new_best_resets_the_stall():
    trace = [10.0, 9.0, 9.5, 9.4, 8.0, 8.1, 8.2, 8.3, 1.0]
    assert M.stop_iterations(trace, 1, 1e-3, 3, 0) == 7                 # stall 1, 2 at evaluations 2, 3; reset at 4; 3 at 7
    assert M.stop_iterations(trace, 1, 1e-3, 2, 0) == 3
    assert M.stop_iterations(trace, 1, 1e-3, 4, 0) == 9                 # the new best at 8 comes first


def test_min_iter_delays_a_stop():
    const = np.full(30, 2.0)
    assert M.stop_iterations(const, 1, 1e-4, 2, 10) == 10
    assert M.stop_iterations(const, 3, 1e-4, 2, 10) == 12               # the first evaluation >= min_iter
    assert M.stop_iterations(const, 1, 1e-4, 2, 1) == 2                 # min_iter below the natural stop changes nothing
    assert M.stop_iterations(const, 1, 1e-4, 2, 99) == 30


def test_nan_counts_as_a_stall():
    nan = float("nan")
    assert M.stop_iterations([5.0, nan, nan, 1.0], 1, 1e-4, 2, 0) == 2
    assert M.stop_iterations([nan, nan, nan], 1, 1e-4, 2, 0) == 1       # no best yet: NaN is still no improvement
    assert M.stop_iterations([5.0, nan, 4.0, nan, 3.0], 1, 1e-4, 2, 0) == 5
    assert M.stop_iterations([math.inf, math.inf, 1.0], 1, 1e-4, 2, 0) == 1


def test_zero_tolerance_with_equal_losses_stalls():
    assert M.stop_iterations([3.0, 3.0, 3.0, 3.0], 1, 0.0, 3, 0) == 3
    assert M.stop_iterations([3.0, np.nextafter(3.0, 0), np.nextafter(np.nextafter(3.0, 0), 0), 2.0], 1, 0.0, 1, 0) == 4


def test_batches_are_columns():
    a = np.stack([np.full(10, 1.0), 10.0 - np.arange(10), np.r_[np.full(5, 2.0), np.full(5, np.nan)]], axis=1)
    assert M.stop_iterations(a, 1, 1e-4, 3, 0).tolist() == [3, 10, 3]


def test_scalar_loss_is_the_expression_of_the_rule():
    from asr_amd import ops
    t = np.array([[3.0, 5.0, 7.0, 11.0], [1e-3, 2e5, 0.1, 9.0]])
    lam = (0.7, 0.3, 0.05, 0.01)
    l = [float(np.float32(v)) for v in lam]
    want = [((l[0] * r[0] + l[1] * r[1]) + l[2] * r[2]) + l[3] * r[3] for r in t]
    assert M.scalar_loss(t, lam).tolist() == want == ops.sr_loss_from_terms(t, lam).tolist()
    no_l1 = [(l[0] * r[0] + l[1] * r[1]) + l[2] * r[2] for r in t]
    assert M.scalar_loss(t, lam[:3] + (0.0,)).tolist() == no_l1 == ops.sr_loss_from_terms(t, lam[:3] + (0.0,)).tolist()


def test_the_float32_summands_are_the_data_terms_rho():
    r = np.random.default_rng(0).standard_normal((3, 4, 5)).astype(np.float32) * 0.2
    w = np.random.default_rng(1).random((3, 4, 5), dtype=np.float32)
    for loss in RD.LOSSES:
        np.testing.assert_allclose(M.rho32(r, loss, 0.1), RD.rho64(r, loss, 0.1), rtol=3e-7)
        assert M.rho32(r, loss, 0.1, w).dtype == np.float32
        assert M.exact_sum(M.rho32(r, loss, 0.1, w))[0] == pytest.approx(RD.data_term64(r, loss, 0.1, w), rel=1e-6)
    x = np.random.default_rng(2).standard_normal((6, 7)).astype(np.float32)
    from oracle import sr as o_sr
    import torch
    assert M.exact_sum(M.btv_summands(x, 0.6, 2))[0] == pytest.approx(
        o_sr.bilateral_tv(torch.from_numpy(x[None, :, :, None]), 0.6, 2), rel=1e-12)
    assert M.btv_summands(x, 0.6, 2).shape == (15, 6, 7)


# ---- the host checks ----------------------------------------------------------------------------------------------------------
def test_check_sr_monitor():
    from asr_amd import ops
    assert check_sr_monitor({}) == ops.SR_MONITOR_DEFAULTS == dict(every=1, rel_tol=1e-4, patience=3, min_iter=0, history=True)
    got = check_sr_monitor(dict(every=np.int64(5), rel_tol=0, patience=0, min_iter=7, history=False))
    assert got == dict(every=5, rel_tol=0.0, patience=0, min_iter=7, history=False) and type(got["every"]) is int
    bad = [dict(every=0), dict(every=-1), dict(every=1.5), dict(every=True), dict(every=None), dict(every="2"),
           dict(rel_tol=-1e-9), dict(rel_tol=float("nan")), dict(rel_tol=float("inf")), dict(rel_tol="1e-4"), dict(rel_tol=None),
           dict(rel_tol=True), dict(patience=-1), dict(patience=2.0), dict(patience=None), dict(min_iter=-1), dict(min_iter=0.5),
           dict(history=1), dict(history=None), dict(tolerance=1e-3), dict(every=2 ** 31)]
    for params in bad:
        with pytest.raises(ValueError, match="monitor"):
            check_sr_monitor(params)
    for params in (None, 3, [("every", 1)], "every"):
        with pytest.raises(ValueError, match="dict"):
            check_sr_monitor(params)
    import torch
    x, y, tf = torch.zeros(2, 8, 8), torch.zeros(2, 3, 4, 4), torch.zeros(2, 3, 8)
    with pytest.raises(ValueError, match="monitor"):          # before anything touches a device
        ops.sr_solve(x, y, tf, tf, tf, tf, torch.zeros(1, 2), (1, 0.3, 0, 0), cfg=ops.sr_config(), monitor=dict(every=0))
    import inspect
    assert inspect.signature(ops.sr_solve).parameters["monitor"].default is None


def test_superresolution_and_path_host_checks():
    from asr_amd.pipeline import HotPath
    from asr_amd.superresolution_scripts.superresolution import Superresolution
    kw = dict(num_iter=2, num_aug=2, feature_size=(4, 4), output_size=(8, 8))
    sr = Superresolution(1, 0.3, 0, 0, **kw)
    assert sr.monitor is None and sr.last_trace is None
    assert Superresolution(1, 0.3, 0, 0, stop_rel_tol=1e-3, **kw).monitor == dict(every=1, rel_tol=1e-3, patience=3, min_iter=0,
                                                                                history=False)
    assert Superresolution(1, 0.3, 0, 0, keep_history=True, stop_every=5, **kw).monitor == dict(every=5, rel_tol=0.0, patience=0,
                                                                                             min_iter=0, history=True)
    assert Superresolution(1, 0.3, 0, 0, stop_rel_tol=0, stop_patience=1, stop_min_iter=4, keep_history=True,
                           **kw).monitor == dict(every=1, rel_tol=0.0, patience=1, min_iter=4, history=True)
    for bad in (dict(stop_rel_tol=-1.0), dict(stop_rel_tol=float("nan")), dict(stop_rel_tol="x"), dict(stop_rel_tol=1e-3, stop_patience=0),
                dict(stop_rel_tol=1e-3, stop_patience=-2), dict(stop_patience=-1), dict(stop_every=0), dict(stop_every=1.5),
                dict(stop_rel_tol=1e-3, stop_every=0), dict(stop_min_iter=-1), dict(stop_rel_tol=1e-3, stop_min_iter=-1),
                dict(keep_history=1), dict(stop_rel_tol=1e-3, verbose=True), dict(keep_history=True, verbose=True)):
        with pytest.raises(ValueError):
            Superresolution(1, 0.3, 0, 0, **kw, **bad)
    assert HotPath.check_sr_stop(None) is None
    assert HotPath.check_sr_stop({}) == dict(every=1, rel_tol=1e-4, patience=3, min_iter=0, history=False)
    assert HotPath.check_sr_stop(dict(rel_tol=1e-2, patience=0, every=4, min_iter=3)) == dict(every=4, rel_tol=1e-2, patience=0,
                                                                                              min_iter=3, history=False)
    for bad in (3, "1e-4", [1e-4], dict(tol=1e-4), dict(history=True), dict(rel_tol=-1), dict(patience=-1), dict(every=0),
                dict(min_iter=-3), dict(rel_tol=float("inf"))):
        with pytest.raises(ValueError, match="sr_stop"):
            HotPath.check_sr_stop(bad)
    path = HotPath(None, sr, mode="argmax")
    with pytest.raises(ValueError, match="sr_stop"):          # the first thing run_image_labels does
        path.run_image_labels(None, None, None, class_ids=(1, 2), sr_stop=dict(every=0))
    import inspect
    from asr_amd import evaluation
    assert inspect.signature(HotPath.run_image_labels).parameters["sr_stop"].default is None
    assert inspect.signature(evaluation.evaluate_labelmaps).parameters["sr_stop"].default is None


# ---- the library ---------------------------------------------------------------------------------------------------------------
def _cfg(**kw):
    from asr_amd import _lib, ops
    return ops.sr_config(_lib.OPT_ADAM, True, 0.1, 0.001, 1e-7, **kw)


def _dt(loss=0, delta=0.1, weights=None, shared=0, wy=None, wx=None, tv_shared=0):
    from asr_amd import _lib
    return _lib.SrDataTerm(loss, delta, weights, shared, wy, wx, tv_shared)


def _mon(every=1, rel_tol=1e-4, patience=3, min_iter=0, history=None, iters_done=FAKE):
    from asr_amd import _lib
    return _lib.SrMonitor(every, rel_tol, patience, min_iter, history, iters_done)


def _solve(lib, mon, dt=None, x=FAKE, dims=DIMS, cfg=None, ws_bytes=1 << 30, iters=1, dev=FAKE):
    """dev: every device pointer but x; None proves that the refusal came before any launch could have read one."""
    dt = C.byref(_dt()) if dt is None else dt
    return lib.asr_sr_solve_mon_f32(x, dev, dev, dev, dev, dev, dev, dev, dev, dev, iters, None, dev, ws_bytes, *dims,
                                    1.0, 0.3, 0.0, 0.0, C.byref(cfg or _cfg()), dt, mon, None)


def test_the_library_exports_the_monitor_and_keeps_its_abi(lib):
    from asr_amd import _lib
    assert hasattr(lib, "asr_sr_solve_mon_f32") and hasattr(lib, "asr_sr_solve_workspace_bytes_mon")
    assert lib.asr_abi_version() == _lib.ABI_VERSION == 3
    assert [f[0] for f in _lib.SrMonitor._fields_] == ["every", "rel_tol", "patience", "min_iter", "history", "iters_done"]
    assert C.sizeof(_lib.SrMonitor) == 40                                   # int, pad, double, int, int, two pointers
    cfg = _cfg()
    base = lib.asr_sr_solve_workspace_bytes_dt(2, 3, 8, 8, 4, 4, C.byref(cfg))
    # + alignment slack, 256 partials x 4 terms and the best loss per image in float64, two ints per image
    assert lib.asr_sr_solve_workspace_bytes_mon(2, 3, 8, 8, 4, 4, C.byref(cfg)) == base + 8 + 8 * (2 * 256 * 4 + 2) + 4 * 2 * 2


def test_monitor_refusals(lib):
    for dev in (FAKE, None):
        for x in ((FAKE, None) if dev else (None,)):
            def refused(mon, what):
                assert _solve(lib, mon, x=x, dev=dev) == INVALID, what
                assert what in lib.asr_last_error(), lib.asr_last_error()
            refused(None, b"null monitor")
            for every in (0, -1, -(2 ** 31)):
                refused(C.byref(_mon(every=every)), b"every")
            for tol in (-1e-300, -1.0, float("nan"), float("inf"), float("-inf")):
                refused(C.byref(_mon(rel_tol=tol)), b"rel_tol")
            refused(C.byref(_mon(patience=-1)), b"patience")
            refused(C.byref(_mon(min_iter=-1)), b"min_iter")
            refused(C.byref(_mon(iters_done=None)), b"iters_done")
    # every refusal of the _dt twin stays
    ok = C.byref(_mon())
    assert _solve(lib, ok, dt=C.byref(_dt(loss=7))) == INVALID and b"unknown loss" in lib.asr_last_error()
    assert _solve(lib, ok, dt=C.byref(_dt(loss=2, delta=0.0))) == INVALID and b"finite and > 0" in lib.asr_last_error()
    assert lib.asr_sr_solve_mon_f32(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 1, None, FAKE, 1 << 30, *DIMS,
                                    1.0, 0.3, 0.0, 0.0, C.byref(_cfg()), None, ok, None) == INVALID
    assert b"null data term" in lib.asr_last_error()
    assert _solve(lib, ok, x=None) == INVALID and b"null pointer" in lib.asr_last_error()
    assert _solve(lib, ok, iters=-1) == INVALID and b"num_iter" in lib.asr_last_error()
    assert _solve(lib, ok, dims=(1, 2, 12, 12, 4, 4)) == UNSUPPORTED
    assert _solve(lib, ok, dt=C.byref(_dt(wy=FAKE, wx=FAKE)), cfg=_cfg(use_btv=True)) == UNSUPPORTED
    bad = _cfg(); bad.prior = 7
    assert _solve(lib, ok, cfg=bad) == INVALID and b"unknown prior" in lib.asr_last_error()
    cfg = _cfg()
    need = lib.asr_sr_solve_workspace_bytes_mon(*DIMS, C.byref(cfg))
    assert _solve(lib, ok, ws_bytes=need - 1) == WORKSPACE and b"workspace" in lib.asr_last_error()
    assert _solve(lib, ok, ws_bytes=lib.asr_sr_solve_workspace_bytes_dt(*DIMS, C.byref(cfg))) == WORKSPACE


# ---- the CSV and the scripts ---------------------------------------------------------------------------------------------------
def test_sr_iters_csv_round_trips(tmp_path):
    from asr_amd.evaluation import SR_ITERS_CSV_COLUMNS, read_sr_iters_csv, write_sr_iters_csv
    rows = [("2007_000033", "1", 50), ("2007_000033", "15", 12), ("2007_000042", "15_max", 0), ("a,b \"c\"", "3", np.int32(7))]
    p = str(tmp_path / "iters.csv")
    write_sr_iters_csv(p, rows)
    assert read_sr_iters_csv(p) == [(a, b, int(c)) for a, b, c in rows]
    assert open(p).readline().strip() == ",".join(f'"{c}"' for c in SR_ITERS_CSV_COLUMNS) == '"image","class","iterations"'
    write_sr_iters_csv(p, [])
    assert read_sr_iters_csv(p) == []
    open(p, "w").write("x,y\n")
    with pytest.raises(ValueError, match="not an SR-iterations CSV"):
        read_sr_iters_csv(p)


def _help(script):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script), "--help"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_the_scripts_list_the_flags():
    out = _help("validate_labelmap.py")
    for flag in ("--sr_stop_tol", "--sr_stop_patience", "--sr_stop_every", "--sr_stop_min_iter", "--sr_iters_out"):
        assert flag in out, flag
    out = _help("SR_single_class.py")
    for flag in ("--sr_stop_tol", "--sr_stop_patience", "--sr_stop_every", "--sr_stop_min_iter"):
        assert flag in out, flag
    assert "--sr_iters_out" not in out
