"""Host side of the order-statistic fusions (asr_realign_select_f32: median, quantiles, trimmed mean over the realigned
copies): what the library and the Python layers decide before any launch.  No GPU is needed."""
import ctypes as C
import types

import numpy as np
import pytest

ERR_INVALID, ERR_UNSUPPORTED = -1, -2
FAKE = 1 << 20                    # non-null and aligned; never dereferenced on the host


def _ranks(lo, hi, t=None):
    n = len(lo)
    t = [0.5] * n if t is None else t
    return (C.c_int * max(n, 1))(*lo), (C.c_int * max(n, 1))(*hi), (C.c_float * max(n, 1))(*t)


def _select(lib, y=FAKE, out_q=FAKE, out_trim=None, lo=(0,), hi=(0,), num_q=None, trim_k=0, trans=FAKE, rot=FAKE, batch=1,
            n=4, H=8, W=8, h=4, w=4):
    lo_a, hi_a, t_a = _ranks(list(lo), list(hi))
    return lib.asr_realign_select_f32(y, out_q, out_trim, lo_a, hi_a, t_a, len(lo) if num_q is None else num_q, trim_k, trans,
                                      rot, batch, n, H, W, h, w, None)


def test_cap_is_host_arithmetic(lib):
    cap = lib.asr_realign_select_max_copies()
    assert cap >= 256
    # 64 pixels x 4 bytes per copy in a workgroup's 160 KiB
    assert cap == 160 * 1024 // 256


def test_argument_validation_needs_no_gpu(lib):
    """Every refusal below happens before any launch (and before any device call: this runs without a GPU)."""
    cap = lib.asr_realign_select_max_copies()
    # null pointers
    for kw in (dict(y=None), dict(trans=None), dict(rot=None), dict(out_q=None)):
        assert _select(lib, **kw) == ERR_INVALID and b"null pointer" in lib.asr_last_error(), kw
    assert lib.asr_realign_select_f32(FAKE, FAKE, None, None, None, None, 1, 0, FAKE, FAKE, 1, 4, 8, 8, 4, 4, None) == ERR_INVALID
    assert b"null pointer" in lib.asr_last_error()
    # num_q = 9
    assert _select(lib, lo=[0] * 9, hi=[0] * 9) == ERR_INVALID and b"num_q=9" in lib.asr_last_error()
    assert _select(lib, num_q=-1) == ERR_INVALID
    # num_q = 0 with no out_trim
    assert _select(lib, lo=(), hi=(), out_q=None) == ERR_INVALID and b"nothing to compute" in lib.asr_last_error()
    # lo > hi, hi = n, lo < 0
    assert _select(lib, lo=(2,), hi=(1,)) == ERR_INVALID and b"ranks[0] = (2, 1)" in lib.asr_last_error()
    assert _select(lib, lo=(0, 3), hi=(0, 4)) == ERR_INVALID and b"ranks[1] = (3, 4)" in lib.asr_last_error()
    assert _select(lib, lo=(-1,), hi=(0,)) == ERR_INVALID
    # 2 * trim_k >= n
    assert _select(lib, lo=(), hi=(), out_q=None, out_trim=FAKE, trim_k=2) == ERR_INVALID and b"trim_k=2" in lib.asr_last_error()
    assert _select(lib, lo=(), hi=(), out_q=None, out_trim=FAKE, trim_k=-1) == ERR_INVALID
    assert _select(lib, n=5, lo=(), hi=(), out_q=None, out_trim=FAKE, trim_k=3) == ERR_INVALID
    assert _select(lib, trim_k=1) == ERR_INVALID and b"without out_trim" in lib.asr_last_error()
    # bad shapes
    for kw in (dict(batch=0), dict(n=0), dict(H=0), dict(W=-1), dict(h=0), dict(w=0)):
        assert _select(lib, **kw) == ERR_INVALID and b"bad shape" in lib.asr_last_error(), kw
    # n above the cap: unsupported, and the message names the cap
    assert _select(lib, n=cap + 1) == ERR_UNSUPPORTED
    assert str(cap).encode() in lib.asr_last_error() and str(cap + 1).encode() in lib.asr_last_error()


def test_quantile_ranks():
    from asr_amd import ops
    assert ops.quantile_ranks(1, 0.5) == (0, 0, 0.0)
    assert ops.quantile_ranks(1, 0.0) == (0, 0, 0.0) and ops.quantile_ranks(1, 1.0) == (0, 0, 0.0)
    assert ops.quantile_ranks(2, 0.5) == (0, 1, 0.5)
    assert ops.quantile_ranks(5, 0.5) == (2, 2, 0.0)
    assert ops.quantile_ranks(100, 0.5) == (49, 50, 0.5)
    assert ops.quantile_ranks(200, 0.5) == (99, 100, 0.5)
    for n in (2, 5, 100, 640):
        assert ops.quantile_ranks(n, 0.0) == (0, 0, 0.0)
        assert ops.quantile_ranks(n, 1.0) == (n - 1, n - 1, 0.0)
    # p = q * (n - 1) in float64, t the float32 of its fraction; ranks always inside 0 .. n - 1 and adjacent
    for n in (3, 64, 65, 100, 200):
        for q in (0.1, 0.25, 0.75, 0.9):
            lo, hi, t = ops.quantile_ranks(n, q)
            p = np.float64(q) * np.float64(n - 1)
            assert (lo, hi) == (int(np.floor(p)), int(np.ceil(p))) and 0 <= lo <= hi <= n - 1 and hi - lo <= 1
            assert t == float(np.float32(p - lo)) and 0.0 <= t < 1.0
    # numpy's default (linear) quantile is the same rule
    s = np.sort(np.random.default_rng(3).standard_normal(100))
    lo, hi, t = ops.quantile_ranks(100, 0.3)
    assert abs((s[lo] + (s[hi] - s[lo]) * t) - np.quantile(s, 0.3)) < 1e-6
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            ops.quantile_ranks(10, bad)
    with pytest.raises(ValueError):
        ops.quantile_ranks(0, 0.5)


def test_compute_SR_rejects_an_unknown_type_naming_the_five(tmp_path):
    from asr_amd.superresolution_scripts import superres_utils as su
    assert su.SR_TYPES == ("aug", "mean", "max", "median", "trimmed_mean")
    with pytest.raises(ValueError) as e:
        su.compute_SR(types.SimpleNamespace(), [], [], [], "x", str(tmp_path), SR_type="mode")
    for t in su.SR_TYPES:
        assert repr(t) in str(e.value)
    assert not (tmp_path / "mode_SR").exists()


def test_trim_is_range_checked():
    from asr_amd.superresolution_scripts.superresolution import Superresolution
    assert Superresolution(1, 0, 0, 0).trim == 0.1
    assert Superresolution(1, 0, 0, 0, trim=0.0).trim == 0.0 and Superresolution(1, 0, 0, 0, trim=0.49).trim == 0.49
    for bad in (0.5, 0.75, -0.01, float("nan")):
        with pytest.raises(ValueError):
            Superresolution(1, 0, 0, 0, trim=bad)
    # k = int(trim * n): scipy.stats.trim_mean's convention
    assert [int(0.1 * n) for n in (5, 10, 19, 100)] == [0, 1, 1, 10]


def test_evaluation_refuses_an_unknown_extra_type():
    from asr_amd import evaluation as E
    with pytest.raises(ValueError):
        E.evaluate_precomputed(None, [], "", extra_sr_types=("mode",))
    with pytest.raises(ValueError):
        E.evaluate_precomputed(None, [], "", extra_sr_types=("max",))       # one of the reference's three: not an extra
    with pytest.raises(ValueError, match="out_dir"):
        E.evaluate_precomputed(None, ["1.hdf5"], "", extra_sr_types=("median",))


def test_iou_record_and_default_arity_are_unchanged():
    """distributed.IOU_FIELDS keeps its six columns and extra_sr_types defaults to the empty tuple (two return values)."""
    import inspect
    from asr_amd import distributed as D
    from asr_amd import evaluation as E
    assert D.IOU_FIELDS == ("standard_single", "standard_bg", "aug_single", "aug_bg", "max", "mean")
    assert inspect.signature(E.evaluate_precomputed).parameters["extra_sr_types"].default == ()
