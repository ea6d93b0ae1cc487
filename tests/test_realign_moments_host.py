"""Host side of the moments over the realigned copies (asr_realign_moments_f32: mean, population variance and valid count):
what the library and the Python layers decide before any launch.  No GPU is needed."""
import inspect

import pytest
import torch

ERR_INVALID = -1
FAKE = 1 << 20                    # non-null and aligned; never dereferenced on the host


def _moments(lib, y=FAKE, wgt=FAKE, shared=0, mean=FAKE, var=None, nv=None, valid_min=0.5, trans=FAKE, rot=FAKE, batch=1, n=4,
             H=8, W=8, h=4, w=4):
    return lib.asr_realign_moments_f32(y, wgt, shared, mean, var, nv, valid_min, trans, rot, batch, n, H, W, h, w, None)


def test_argument_validation_needs_no_gpu(lib):
    """Every refusal below happens before any launch (and before any device call: this runs without a GPU)."""
    for kw in (dict(y=None), dict(trans=None), dict(rot=None), dict(y=None, wgt=None)):
        assert _moments(lib, **kw) == ERR_INVALID and b"null pointer" in lib.asr_last_error(), kw
    for wgt in (FAKE, None):
        assert _moments(lib, wgt=wgt, mean=None) == ERR_INVALID and b"nothing to compute" in lib.asr_last_error()
        for kw in (dict(batch=0), dict(batch=65536), dict(n=0), dict(H=0), dict(W=-1), dict(h=0), dict(w=0)):
            assert _moments(lib, wgt=wgt, **kw) == ERR_INVALID and b"bad shape" in lib.asr_last_error(), kw
            assert _moments(lib, wgt=wgt, var=FAKE, nv=FAKE, **kw) == ERR_INVALID and b"bad shape" in lib.asr_last_error(), kw
    for bad in (0.0, -0.5, float("inf"), float("-inf"), float("nan")):
        for outs in (dict(), dict(mean=None, var=FAKE), dict(mean=None, nv=FAKE), dict(var=FAKE, nv=FAKE)):
            for shared in (0, 1):
                assert _moments(lib, valid_min=bad, shared=shared, **outs) == ERR_INVALID, (bad, outs)
                msg = lib.asr_last_error()
                assert b"valid_min" in msg and b"finite and > 0" in msg, (bad, msg)


def test_ops_realign_moments_refuses_before_the_library():
    from asr_amd import _lib, ops
    assert ops.MOMENT_OUTPUTS == ("mean", "var", "nv")
    assert inspect.signature(ops.realign_moments).parameters["want"].default == ("mean", "var")
    assert inspect.signature(ops.realign_moments).parameters["wgt"].default is None
    assert inspect.signature(ops.realign_moments).parameters["valid_min"].default == 0.5
    y = torch.zeros((2, 3, 4, 5))
    tf = torch.zeros((2, 3, 8))
    ones = torch.ones((4, 5))
    for want in ((), ("median",), ("var", "var"), ("mean", "cov"), "variance"):
        with pytest.raises(_lib.AsrError, match="want"):
            ops.realign_moments(y, tf, tf, (8, 10), want=want)
    for wgt in (torch.ones((5, 4)), torch.ones((4,)), torch.ones((3, 4, 5)), torch.ones((2, 3, 4, 4)), torch.ones((1, 3, 4, 5)),
                torch.ones((2, 1, 4, 5))):
        with pytest.raises(_lib.AsrError, match="wgt"):
            ops.realign_moments(y, tf, tf, (8, 10), wgt=wgt)
    with pytest.raises(_lib.AsrError, match=r"\[B,N,h,w\]"):
        ops.realign_moments(y[0], tf, tf, (8, 10))
    with pytest.raises(_lib.AsrError, match="trans_tf"):
        ops.realign_moments(y, tf[:, :2], tf, (8, 10))
    with pytest.raises(_lib.AsrError, match="rot_tf"):
        ops.realign_moments(y, tf, tf[:1], (8, 10), wgt=ones)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(_lib.AsrError, match="valid_min"):
            ops.realign_moments(y, tf, tf, (8, 10), wgt=ones, valid_min=bad)
    # everything in order: the next stop is the device pointer of a host tensor (no CPU fallback); without wgt valid_min is not read
    for kw in (dict(), dict(wgt=ones), dict(wgt=torch.ones((2, 3, 4, 5))), dict(valid_min=float("nan"))):
        with pytest.raises(_lib.AsrError, match="device memory"):
            ops.realign_moments(y, tf, tf, (8, 10), want=("mean", "var", "nv"), **kw)


def test_superresolution_surface():
    from asr_amd.superresolution_scripts.superresolution import Superresolution
    sr = Superresolution(1, 0, 0, 0)
    assert callable(sr.variance_superresolution) and callable(sr.realign_moments_batch)
    assert list(inspect.signature(sr.variance_superresolution).parameters) == ["augmented_copies", "angles", "shifts"]
    assert list(inspect.signature(sr.realign_moments_batch).parameters) == ["copies", "angles", "shifts", "want", "cover"]
    with pytest.raises(ValueError, match="cover"):
        sr.realign_moments_batch(torch.zeros((1, 2, 4, 4)), [[0, 0]], [[[0, 0], [0, 0]]], cover="both")
