"""Copy reweighting (include/asr_hip.h, "copy reweighting") without a GPU: the C entry points' refusals through ctypes (null or
fake device pointers: refused before any launch), the host checks, the identities of the numpy restatement, and the synthetic
construction of sr_dt_ref on the CPU restatement of the reweighted solve."""
import ctypes as C

import numpy as np
import pytest

from asr_amd.ops import check_sr_reweight          # the feature itself: nothing below runs without it
import sr_dt_ref as RD
import sr_rw_ref as RW

FAKE = 1 << 20                      # non-null, never dereferenced on the host: every call below is refused before a launch
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
DIMS = (1, 2, 8, 8, 4, 4)


# ---- the library ---------------------------------------------------------------------------------------------------------------
def _cfg(**kw):
    from asr_amd import _lib, ops
    return ops.sr_config(_lib.OPT_ADAM, True, 0.1, 0.001, 1e-7, **kw)


def _dt(loss=0, delta=0.1, weights=None, shared=0):
    from asr_amd import _lib
    return _lib.SrDataTerm(loss, delta, weights, shared, None, None, 0)


def _rw(kind=0, kappa=2.0, every=10, start=10, copy_weights=FAKE, history=None):
    from asr_amd import _lib
    return _lib.SrReweight(kind, kappa, every, start, copy_weights, history)


def _solve(lib, rw, dt=None, x=FAKE, dims=DIMS, cfg=None, ws_bytes=1 << 30, iters=1, dev=FAKE, mon=None, group=0):
    dt = C.byref(_dt()) if dt is None else dt
    return lib.asr_sr_solve_rw_f32(x, dev, dev, dev, dev, dev, dev, dev, dev, dev, iters, None, dev, ws_bytes, *dims,
                                   1.0, 0.3, 0.0, 0.0, C.byref(cfg or _cfg()), dt, mon, group, rw, None)


def test_the_library_exports_the_reweighting_and_keeps_its_abi(lib):
    from asr_amd import _lib
    for name in ("asr_sr_solve_rw_f32", "asr_sr_solve_workspace_bytes_rw", "asr_sr_copy_energy_f64", "asr_sr_copy_weights_f32",
                 "asr_sr_apply_copy_weights_f32"):
        assert hasattr(lib, name), name
    assert lib.asr_abi_version() == _lib.ABI_VERSION == 3
    assert [f[0] for f in _lib.SrReweight._fields_] == ["kind", "kappa", "every", "start", "copy_weights", "history"]
    assert C.sizeof(_lib.SrReweight) == 40                                  # int, pad, double, int, int, two pointers
    assert (_lib.RW_CAUCHY, _lib.RW_HARD, _lib.RW_MAX_COPIES) == (0, 1, 640)
    cfg = _cfg()
    for monitored in (0, 1):
        base = lib.asr_sr_solve_workspace_bytes_ml(2, 3, 8, 8, 4, 4, C.byref(cfg), monitored)
        # + w_eff [2, 3, 4, 4] float32, alignment slack, energy and mass per copy in float64
        assert lib.asr_sr_solve_workspace_bytes_rw(2, 3, 8, 8, 4, 4, C.byref(cfg), monitored) == base + 4 * 2 * 3 * 16 + 8 + 8 * 2 * 2 * 3


def test_the_kernel_section_holds_the_four_kernels_and_sr_hip_launches_them_through_it():
    """csrc/sr_rw_kernels.h is a section of sr.hip's translation unit: every kernel it launches is one of the four that
    tests/test_gpu_sr_rw.py pins, sr.hip includes it once and reaches the kernels through its launch functions alone."""
    import os
    from conftest import ROOT
    import sr_option_cases as T
    csrc = os.path.join(ROOT, "deeplabv3plus-augmented-superresolution_amd", "csrc")
    section = open(os.path.join(csrc, "sr_rw_kernels.h")).read()
    four = {"sr_rw_energy_kernel", "sr_rw_weights_kernel", "sr_rw_apply_kernel", "sr_rw_rearm_kernel"}
    assert T.source_instantiations(section) == four
    for k in four:
        assert f"SR_NO_PK_F32 void {k}(" in section, k
    unit = open(os.path.join(csrc, "sr.hip")).read()
    assert unit.count('#include "sr_rw_kernels.h"') == 1 and not any(k in unit for k in four)
    for fn in ("sr_rw_energy_launch", "sr_rw_weights_launch", "sr_rw_apply_launch", "sr_rw_rearm_launch"):
        assert fn + "(" in unit and "int " + fn + "(" in section, fn


def test_solve_refusals(lib):
    for dev in (FAKE, None):
        for x in ((FAKE, None) if dev else (None,)):
            def refused(rw, what):
                assert _solve(lib, C.byref(rw), x=x, dev=dev) == INVALID, what
                assert what in lib.asr_last_error(), lib.asr_last_error()
            for kind in (-1, 2, 7):
                refused(_rw(kind=kind), b"unknown reweighting kind")
            for kappa in (0.0, -2.0, float("nan"), float("inf"), float("-inf")):
                refused(_rw(kappa=kappa), b"kappa")
            for every in (0, -1, -(2 ** 31)):
                refused(_rw(every=every), b"every")
            refused(_rw(start=-1), b"start")
            refused(_rw(copy_weights=None), b"copy_weights")
    ok = C.byref(_rw())
    # the refusals of the entry point it wraps stay
    assert _solve(lib, ok, dt=C.byref(_dt(loss=7))) == INVALID and b"unknown loss" in lib.asr_last_error()
    assert _solve(lib, ok, x=None) == INVALID and b"null pointer" in lib.asr_last_error()
    assert _solve(lib, ok, dims=(1, 2, 12, 12, 4, 4)) == UNSUPPORTED
    assert _solve(lib, ok, group=1) == UNSUPPORTED and b"ASR_OPT_PRIMAL_DUAL" in lib.asr_last_error()
    assert _solve(lib, ok, group=3) == INVALID
    assert _solve(lib, ok, dims=(1, 641, 8, 8, 4, 4)) == INVALID and b"640" in lib.asr_last_error()
    cfg = _cfg()
    need = lib.asr_sr_solve_workspace_bytes_rw(*DIMS, C.byref(cfg), 0)
    assert _solve(lib, ok, ws_bytes=need - 1) == WORKSPACE and b"workspace" in lib.asr_last_error()
    # without rw the workspace of the wrapped entry point is enough: nothing is launched on a null stream with num_iter = 0
    assert _solve(lib, None, ws_bytes=lib.asr_sr_solve_workspace_bytes_ml(*DIMS, C.byref(cfg), 0) - 1) == WORKSPACE


def test_stand_alone_refusals(lib):
    dt = C.byref(_dt())
    assert lib.asr_sr_copy_energy_f64(None, dt, FAKE, FAKE, 1, 2, 4, 4, None) == INVALID and b"null pointer" in lib.asr_last_error()
    assert lib.asr_sr_copy_energy_f64(FAKE, None, FAKE, FAKE, 1, 2, 4, 4, None) == INVALID and b"null data term" in lib.asr_last_error()
    assert lib.asr_sr_copy_energy_f64(FAKE, C.byref(_dt(loss=5)), FAKE, FAKE, 1, 2, 4, 4, None) == INVALID
    assert lib.asr_sr_copy_energy_f64(FAKE, dt, FAKE, FAKE, 1, 0, 4, 4, None) == INVALID and b"bad shape" in lib.asr_last_error()
    assert lib.asr_sr_copy_energy_f64(FAKE, dt, FAKE, FAKE, 1, 641, 4, 4, None) == INVALID and b"640" in lib.asr_last_error()
    assert lib.asr_sr_copy_energy_f64(FAKE, dt, FAKE, FAKE, 1, 2, 4096, 4096, None) == INVALID and b"grid.y" in lib.asr_last_error()
    for kind, kappa, what in ((2, 2.0, b"kind"), (0, 0.0, b"kappa"), (1, float("nan"), b"kappa"), (0, float("inf"), b"kappa")):
        assert lib.asr_sr_copy_weights_f32(FAKE, FAKE, kind, kappa, FAKE, None, 1, 2, None) == INVALID
        assert what in lib.asr_last_error()
    assert lib.asr_sr_copy_weights_f32(FAKE, None, 0, 2.0, FAKE, None, 1, 2, None) == INVALID
    assert lib.asr_sr_copy_weights_f32(FAKE, FAKE, 0, 2.0, FAKE, None, 0, 2, None) == INVALID
    assert lib.asr_sr_copy_weights_f32(FAKE, FAKE, 0, 2.0, FAKE, None, 1, 641, None) == INVALID
    assert lib.asr_sr_apply_copy_weights_f32(FAKE, dt, None, FAKE, FAKE, 1, 2, 4, 4, None) == INVALID
    assert lib.asr_sr_apply_copy_weights_f32(FAKE, dt, FAKE, FAKE, FAKE, 1, 2, 0, 4, None) == INVALID
    assert lib.asr_sr_apply_copy_weights_f32(FAKE, C.byref(_dt(loss=2, delta=-1.0)), FAKE, FAKE, FAKE, 1, 2, 4, 4, None) == INVALID
    assert lib.asr_sr_apply_copy_weights_f32(FAKE, C.byref(_dt(weights=FAKE)), FAKE, FAKE, FAKE, 1, 2, 4, 4, None) == INVALID
    assert b"aliases" in lib.asr_last_error()


# ---- the host checks -------------------------------------------------------------------------------------------------------------
def test_check_sr_reweight():
    from asr_amd import ops
    assert check_sr_reweight({}) == dict(kind="cauchy", kappa=2.0, every=10, start=10, history=False) == ops.SR_REWEIGHT_DEFAULTS
    assert check_sr_reweight("HARD")["kind"] == "hard"
    assert check_sr_reweight(dict(kind="hard", kappa=3, every=np.int64(2), start=0, history=True)) == dict(
        kind="hard", kappa=3.0, every=2, start=0, history=True)
    for bad in (None, 3, ["cauchy"], "tukey", dict(kind="tukey"), dict(kind=0), dict(kappa=0), dict(kappa=-1.0), dict(kappa=float("nan")),
                dict(kappa=float("inf")), dict(kappa="2"), dict(kappa=True), dict(every=0), dict(every=1.5), dict(every=True),
                dict(start=-1), dict(start=2.0), dict(history=1), dict(stride=3)):
        with pytest.raises(ValueError, match="reweight"):
            check_sr_reweight(bad)
    assert ops.sr_reweight_iters(check_sr_reweight(dict(start=1, every=2)), 6) == [1, 3, 5]
    assert ops.sr_reweight_iters(check_sr_reweight({}), 10) == []
    import inspect
    assert inspect.signature(ops.sr_solve).parameters["reweight"].default is None


# ---- the restatement's identities ---------------------------------------------------------------------------------------------
def _energies(seed, B=2, N=7):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.1, 5.0, (B, N)), np.full((B, N), 16.0)


def test_block_sum_is_a_sum_in_a_fixed_order():
    rng = np.random.default_rng(0)
    for P in (1, 63, 64, 255, 256, 257, 1000):
        v = rng.standard_normal(P)
        assert abs(RW.block_sum(v) - np.sum(v)) <= 1e-12 * np.abs(v).sum()
    assert RW.block_sum(np.arange(1, 258)) == 257 * 258 / 2                # exact in any order
    # the order is the header's: thread 1 adds p = 1 and p = 257 before the tree adds it to thread 0's sum
    v = np.zeros(258); v[0], v[1], v[257] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert RW.block_sum(v) == 1.0 + 2.0 ** -52 and (1.0 + 2.0 ** -53) + 2.0 ** -53 == 1.0


def test_a_huge_kappa_gives_all_ones():
    e, a = _energies(1)
    for kind in RW.KINDS:
        c, s = RW.copy_weights(e, a, kind, 1e30)
        assert c.dtype == np.float32 and (c == 1.0).all() and (s > 0).all()


def test_a_zero_scale_gives_all_ones():
    e, a = _energies(2)
    e[0, :4] = 0.0                      # the lower median of 7 values with four zeros is 0
    for kind in RW.KINDS:
        c, s = RW.copy_weights(e, a, kind, 0.5)
        assert s[0] == 0.0 and (c[0] == 1.0).all()
        assert s[1] > 0.0 and (c[1] < 1.0).any()          # the largest of 7 distinct energies lies above half their median


def test_inactive_copies_get_zero_and_do_not_move_the_median():
    e, a = _energies(3, B=1, N=9)
    for kind in RW.KINDS:
        c0, s0 = RW.copy_weights(e, a, kind, 2.0)
        e2 = np.concatenate([e, [[0.0, np.nan, np.inf, 1e-9]]], axis=1)      # masked, NaN residual, overflow, masked with a tiny energy
        a2 = np.concatenate([a, [[0.0, 16.0, 16.0, 0.0]]], axis=1)
        c2, s2 = RW.copy_weights(e2, a2, kind, 2.0)
        assert s2[0] == s0[0] and (c2[0, :9] == c0[0]).all() and (c2[0, 9:] == 0.0).all()
        c3, s3 = RW.copy_weights(np.zeros((1, 3)), np.zeros((1, 3)), kind, 2.0)        # all inactive
        assert s3[0] == 0.0 and (c3 == 0.0).all()


def test_the_scale_is_the_lower_median_and_the_weights_are_the_rule():
    e = np.array([[4.0, 1.0, 3.0, 2.0], [5.0, 5.0, 1.0, 9.0]])
    a = np.ones((2, 4))
    c, s = RW.copy_weights(e, a, "hard", 1.5)
    assert s.tolist() == [2.0, 5.0]                                           # rank (4 - 1) // 2 = 1; ties keep their index order
    assert c.tolist() == [[0.0, 1.0, 1.0, 1.0], [1.0, 1.0, 1.0, 0.0]]
    c, _ = RW.copy_weights(e, a, "cauchy", 2.0)
    assert c[0, 0] == np.float32(0.5) and c[0, 3] == np.float32(1.0 / 1.25)   # t = 1 and t = 1/2
    assert (c <= 1.0).all() and (c > 0.0).all()


def test_energy_mass_and_apply_follow_the_data_term():
    rng = np.random.default_rng(4)
    r = rng.standard_normal((2, 3, 5, 7)).astype(np.float32)
    u = rng.uniform(0, 2, (2, 3, 5, 7)).astype(np.float32)
    u[1, 2] = 0.0
    for loss in RD.LOSSES:
        e, a = RW.copy_energy(r, loss, 0.1, None)
        assert (a == 35.0).all()
        for b in range(2):
            for i in range(3):
                assert abs(e[b, i] - RD.data_term64(r[b, i], loss, 0.1)) <= 1e-5 * e[b, i]
        e, a = RW.copy_energy(r, loss, 0.1, u)
        assert e[1, 2] == 0.0 and a[1, 2] == 0.0
        assert abs(a[0, 0] - u[0, 0].astype(np.float64).sum()) <= 1e-12 * a[0, 0]
        es, _ = RW.copy_energy(r, loss, 0.1, u[0])                                # shared: image 0's weights for both images
        assert (es[0] == e[0]).all() and not (es[1] == e[1]).all()
        c = RW.copy_weights(e, a, "cauchy", 2.0)[0]
        assert c[1, 2] == 0.0
        w_eff, q = RW.apply_copy_weights(r, c, loss, 0.1, u)
        assert (w_eff == u * c[:, :, None, None]).all() and (q == RD.weighted_psi(r, loss, 0.1, w_eff)).all()
        w_eff, q = RW.apply_copy_weights(r, c, loss, 0.1, None)
        assert (w_eff == np.broadcast_to(c[:, :, None, None], r.shape)).all() and (q == RD.weighted_psi(r, loss, 0.1, w_eff)).all()


def test_a_solve_that_never_reweights_is_the_data_term_solve():
    case = RD.make_case(0, H=16, h=8, n=4, n_bad=1)
    x0 = RD.solve_case(case, "l2", iters=4)
    x1, c = RW.solve_case_rw(case, "cauchy", iters=4, start=4)
    assert (x0 == x1).all() and (c == 1.0).all()
    x2, c = RW.solve_case_rw(case, "cauchy", iters=4, start=1, every=2)
    assert not (x0 == x2).all() and (c < 1.0).any()


# ---- the construction -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def construction():
    """seed -> (case, IoU under Huber, (x, c) hard, (x, c) Cauchy): 150 iterations each, kappa 2, every 10, start 10."""
    out = {}
    for seed in (0, 1):
        case = RD.make_case(seed)
        huber = RD.iou(RD.solve_case(case, "huber", 0.1), case["truth"])
        out[seed] = (case, huber, RW.solve_case_rw(case, "hard"), RW.solve_case_rw(case, "cauchy"))
    return out


@pytest.mark.parametrize("seed", (0, 1))
def test_hard_weights_separate_the_replaced_copies(construction, seed):
    case, huber, (x, c), _ = construction[seed]
    kept = np.setdiff1d(np.arange(len(c)), case["bad"])
    print(f"seed {seed}: hard IoU {RD.iou(x, case['truth']):.4f}, Huber {huber:.4f}, weights {c.tolist()}")
    assert (c[case["bad"]] == 0.0).all() and (c[kept] == 1.0).all()
    assert RD.iou(x, case["truth"]) > huber


@pytest.mark.parametrize("seed", (0, 1))
def test_cauchy_weights_separate_the_replaced_copies(construction, seed):
    case, huber, _, (x, c) = construction[seed]
    kept = np.setdiff1d(np.arange(len(c)), case["bad"])
    print(f"seed {seed}: Cauchy IoU {RD.iou(x, case['truth']):.4f}, Huber {huber:.4f}, replaced <= {c[case['bad']].max():.4f}, "
          f"kept >= {c[kept].min():.4f}")
    assert (c[case["bad"]] < 0.1).all() and (c[kept] > 0.3).all()
    assert RD.iou(x, case["truth"]) > huber


# ---- the upper layers' host checks and the scripts ---------------------------------------------------------------------------------
def test_superresolution_keywords_and_the_scripts_helper():
    from asr_amd.superresolution_scripts.superresolution import Superresolution
    kw = dict(num_iter=2, num_aug=2, feature_size=(4, 4), output_size=(8, 8))
    sr = Superresolution(1, 0.3, 0, 0, **kw)
    assert sr.reweight is None and sr.last_copy_weights is None
    assert Superresolution(1, 0.3, 0, 0, reweight="hard", **kw).reweight == dict(kind="hard", kappa=2.0, every=10, start=10, history=False)
    # what validate_classes.py and SR_single_class.py build from their flags: every flag reaches its constructor keyword
    flags = dict(kind="cauchy", kappa=3.5, every=4, start=7)
    assert Superresolution.reweight_keywords(None) == {}
    assert Superresolution.reweight_keywords(flags) == dict(reweight="cauchy", reweight_kappa=3.5, reweight_every=4, reweight_start=7)
    assert Superresolution(1, 0.3, 0, 0, **kw, **Superresolution.reweight_keywords(flags)).reweight == dict(flags, history=False)
    assert Superresolution(1, 0.3, 0, 0, **kw, **Superresolution.reweight_keywords(dict(kind="hard", every=3))).reweight == dict(
        kind="hard", kappa=2.0, every=3, start=10, history=False)
    for bad in (dict(kappa=2.0), dict(kind="hard", stride=2)):
        with pytest.raises(ValueError, match="reweight_keywords"):
            Superresolution.reweight_keywords(bad)
    for bad in (dict(reweight="tukey"), dict(reweight="hard", reweight_kappa=0), dict(reweight_every=0), dict(reweight_start=-1),
                dict(reweight="hard", verbose=True)):
        with pytest.raises(ValueError):
            Superresolution(1, 0.3, 0, 0, **kw, **bad)
    # a verbose object whose reweight is set afterwards (as the path sets it) is refused when it solves, before any launch
    import types
    import torch
    loud = Superresolution(1, 0.3, 0, 0, verbose=True, optimizer=object(), **kw)
    loud.reweight = check_sr_reweight("hard")
    with pytest.raises(ValueError, match="verbose"):
        loud._solve_batch(torch.zeros(1, 2, 4, 4), None, None, None)
    from asr_amd.pipeline import HotPath
    assert HotPath.check_sr_reweight(None) is None
    assert HotPath.check_sr_reweight("hard") == dict(kind="hard", kappa=2.0, every=10, start=10, history=False)
    for bad in (3, dict(history=True), dict(kind="tukey"), dict(kappa=-1)):
        with pytest.raises(ValueError, match="sr_reweight"):
            HotPath.check_sr_reweight(bad)
    path = HotPath(None, types.SimpleNamespace(output_size=(8, 8), use_BTV=False, verbose=True), mode="argmax")
    with pytest.raises(ValueError, match="verbose"):
        path.run_image_labels(None, None, None, class_ids=(1, 2), sr_reweight="hard")


def _script(name):
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location(name + "_rw", os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_scripts_flags_parse():
    import os
    import subprocess
    import sys
    from conftest import ROOT
    base = ["--images", "a", "--gt", "b"]
    for name in ("validate_labelmap", "validate_classes"):
        parser = _script(name).parser
        args = parser.parse_args(base)
        assert (args.sr_reweight, args.sr_reweight_kappa, args.sr_reweight_every, args.sr_reweight_start) == (None, None, None, None)
        args = parser.parse_args(base + ["--sr_reweight", "hard", "--sr_reweight_kappa", "1.5", "--sr_reweight_every", "4",
                                         "--sr_reweight_start", "2"])
        assert (args.sr_reweight, args.sr_reweight_kappa, args.sr_reweight_every, args.sr_reweight_start) == ("hard", 1.5, 4, 2)
        with pytest.raises(SystemExit):
            parser.parse_args(base + ["--sr_reweight", "tukey"])
    assert _script("validate_labelmap").parser.parse_args(base + ["--copy_weights_out", "cw.csv"]).copy_weights_out == "cw.csv"
    # each script itself: the flags are parsed and checked by the library's own rule before anything is loaded
    for name, args in (("validate_labelmap", base), ("validate_classes", base), ("SR_single_class", ["--data", "a", "--gt", "b"])):
        run = lambda extra: subprocess.run([sys.executable, os.path.join(ROOT, "scripts", name + ".py")] + args + extra,
                                           capture_output=True, text=True)
        r = run(["--sr_reweight", "cauchy", "--sr_reweight_kappa=-1"])
        assert r.returncode == 2 and "kappa must be a finite number > 0" in r.stderr, (name, r.stderr[-300:])
        r = run(["--sr_reweight", "hard", "--sr_reweight_start=-2"])
        assert r.returncode == 2 and "start must be an integer >= 0" in r.stderr, (name, r.stderr[-300:])
        r = run(["--sr_reweight_every", "3"])
        assert r.returncode == 2 and "need --sr_reweight" in r.stderr, (name, r.stderr[-300:])
        assert "--sr_reweight_kappa" in run(["--help"]).stdout
