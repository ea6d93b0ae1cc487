"""Host side of the coverage-normalised fusions (asr_realign_covered_f32: sum of the realigned values over the sum of the
realigned weights, the median over the copies that saw a pixel, the coverage map): what the library and the Python layers
decide before any launch.  No GPU is needed."""
import inspect

import pytest
import torch

ERR_INVALID, ERR_UNSUPPORTED = -1, -2
FAKE = 1 << 20                    # non-null and aligned; never dereferenced on the host


def _covered(lib, y=FAKE, wgt=FAKE, shared=0, mean=FAKE, median=None, cov=None, cov_min=0.5, valid_min=0.5, trans=FAKE, rot=FAKE,
             batch=1, n=4, H=8, W=8, h=4, w=4):
    return lib.asr_realign_covered_f32(y, wgt, shared, mean, median, cov, cov_min, valid_min, trans, rot, batch, n, H, W, h, w,
                                       None)


def test_argument_validation_needs_no_gpu(lib):
    """Every refusal below happens before any launch (and before any device call: this runs without a GPU)."""
    for kw in (dict(y=None), dict(wgt=None), dict(trans=None), dict(rot=None), dict(wgt=None, shared=1)):
        assert _covered(lib, **kw) == ERR_INVALID and b"null pointer" in lib.asr_last_error(), kw
    assert _covered(lib, mean=None) == ERR_INVALID and b"nothing to compute" in lib.asr_last_error()
    for kw in (dict(batch=0), dict(batch=65536), dict(n=0), dict(H=0), dict(W=-1), dict(h=0), dict(w=0)):
        assert _covered(lib, **kw) == ERR_INVALID and b"bad shape" in lib.asr_last_error(), kw
        assert _covered(lib, median=FAKE, cov=FAKE, **kw) == ERR_INVALID and b"bad shape" in lib.asr_last_error(), kw
    for name in ("cov_min", "valid_min"):
        for bad in (0.0, -0.5, float("inf"), float("nan")):
            assert _covered(lib, **{name: bad}) == ERR_INVALID, (name, bad)
            msg = lib.asr_last_error()
            assert name.encode() in msg and b"finite and > 0" in msg, (name, bad, msg)
            assert _covered(lib, mean=None, median=FAKE, **{name: bad}) == ERR_INVALID, (name, bad)


def test_the_cap_binds_only_the_median(lib):
    """n = cap + 1: unsupported with out_median, and the message names the cap and n.  (Without out_median the same n is
    accepted; that call launches, so it is a GPU test.)"""
    cap = lib.asr_realign_select_max_copies()
    for kw in (dict(median=FAKE), dict(mean=None, median=FAKE), dict(median=FAKE, cov=FAKE)):
        assert _covered(lib, n=cap + 1, **kw) == ERR_UNSUPPORTED, kw
        msg = lib.asr_last_error()
        assert str(cap).encode() in msg and str(cap + 1).encode() in msg and b"out_median" in msg
    # the refusals that do not depend on out_median still come first for such an n
    assert _covered(lib, n=cap + 1, median=FAKE, cov_min=0.0) == ERR_INVALID
    assert _covered(lib, n=cap + 1, mean=None) == ERR_INVALID and b"nothing to compute" in lib.asr_last_error()


def test_ops_realign_covered_refuses_before_the_library():
    from asr_amd import _lib, ops
    assert ops.COVERED_OUTPUTS == ("mean", "median", "cov")
    y = torch.zeros((2, 3, 4, 5))
    tf = torch.zeros((2, 3, 8))
    ones = torch.ones((4, 5))
    for want in ((), ("mode",), ("mean", "mean"), ("mean", "max"), "coverage"):
        with pytest.raises(_lib.AsrError, match="want"):
            ops.realign_covered(y, ones, tf, tf, (8, 10), want=want)
    for wgt in (torch.ones((5, 4)), torch.ones((4,)), torch.ones((3, 4, 5)), torch.ones((2, 3, 4, 4)), torch.ones((1, 3, 4, 5)),
                torch.ones((2, 1, 4, 5))):
        with pytest.raises(_lib.AsrError, match="wgt"):
            ops.realign_covered(y, wgt, tf, tf, (8, 10))
    with pytest.raises(_lib.AsrError, match=r"\[B,N,h,w\]"):
        ops.realign_covered(y[0], ones, tf, tf, (8, 10))
    with pytest.raises(_lib.AsrError, match="trans_tf"):
        ops.realign_covered(y, ones, tf[:, :2], tf, (8, 10))
    with pytest.raises(_lib.AsrError, match="rot_tf"):
        ops.realign_covered(y, ones, tf, tf[:1], (8, 10))
    for name in ("cov_min", "valid_min"):
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            with pytest.raises(_lib.AsrError, match=name):
                ops.realign_covered(y, ones, tf, tf, (8, 10), **{name: bad})
    # everything in order: the next stop is the device pointer of a host tensor (no CPU fallback)
    with pytest.raises(_lib.AsrError, match="device memory"):
        ops.realign_covered(y, ones, tf, tf, (8, 10), want=("mean", "median", "cov"))


def test_superresolution_keywords():
    from asr_amd.superresolution_scripts.superresolution import COVER_MODES, Superresolution
    assert COVER_MODES == ("frame", "validity")
    sr = Superresolution(1, 0, 0, 0)
    assert (sr.cover, sr.cov_min, sr.valid_min) == ("frame", 0.5, 0.5)
    sr = Superresolution(1, 0, 0, 0, cover="validity", cov_min=2.0, valid_min=0.25)
    assert (sr.cover, sr.cov_min, sr.valid_min) == ("validity", 2.0, 0.25)
    for bad in ("none", "", None, "Frame"):
        with pytest.raises(ValueError, match="cover"):
            Superresolution(1, 0, 0, 0, cover=bad)
    for name in ("cov_min", "valid_min"):
        for bad in (0.0, -0.5, float("inf"), float("nan")):
            with pytest.raises(ValueError, match=name):
                Superresolution(1, 0, 0, 0, **{name: bad})
    for m in ("covered_mean_superresolution", "covered_median_superresolution", "coverage_map", "realign_covered_batch"):
        assert callable(getattr(sr, m))
    assert list(inspect.signature(sr.realign_covered_batch).parameters) == ["copies", "angles", "shifts", "want"]


def test_sr_types(tmp_path):
    import types
    from asr_amd.superresolution_scripts import superres_utils as su
    assert su.EXTRA_SR_TYPES == ("median", "trimmed_mean", "covered_mean", "covered_median")
    with pytest.raises(ValueError) as e:
        su.compute_SR(types.SimpleNamespace(), [], [], [], "x", str(tmp_path), SR_type="covered")
    assert "'covered_mean'" in str(e.value) and "'covered_median'" in str(e.value)
    assert not (tmp_path / "covered_SR").exists()


def test_evaluation_accepts_the_names_and_keeps_its_default():
    from asr_amd import evaluation as E
    assert inspect.signature(E.evaluate_precomputed).parameters["extra_sr_types"].default == ()
    # the names pass the type check: the refusal that follows is the one about out_dir
    with pytest.raises(ValueError, match="out_dir"):
        E.evaluate_precomputed(None, ["1.hdf5"], "", extra_sr_types=("covered_mean", "covered_median"))
    with pytest.raises(ValueError, match="covered"):
        E.evaluate_precomputed(None, [], "", extra_sr_types=("covered",))
