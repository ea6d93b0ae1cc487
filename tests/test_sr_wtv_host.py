"""The edge-weighted TV prior without a device: every refusal of the C entry points through ctypes, the shape checks of the ops
wrappers, the ValueErrors of the upper layers, the script's parser, and the yardstick itself -- the restatement of
tests/sr_wtv_ref.py with unit weights is the oracle's own TV gradient bit for bit."""
import ctypes as C
import importlib.util
import inspect
import os
import types

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle import sr as o_sr
from oracle import tf_ops

import sr_wtv_ref as R

FAKE = 1 << 20                      # non-null, never dereferenced on the host: every call below is refused before a launch
INVALID, UNSUPPORTED = -1, -2


def _cfg(**kw):
    from asr_amd import _lib, ops
    return ops.sr_config(_lib.OPT_ADAM, True, 0.1, 0.001, 1e-7, **kw)


def _backward(lib, cfg, x=FAKE, wy=FAKE, wx=FAKE, dims=(1, 2, 8, 8, 4, 4), x_new=None, grad=FAKE):
    return lib.asr_sr_backward_wtv_f32(x, x_new, FAKE, FAKE, FAKE, None, None, None, None, grad, *dims, 1.0, 0.3, 0.0, 0.0,
                                       cfg, wy, wx, 1, None)


def _terms(lib, cfg, x=FAKE, wy=FAKE, wx=FAKE, dims=(1, 2, 8, 8, 4, 4)):
    return lib.asr_sr_loss_terms_wtv_f64(x, FAKE, FAKE, *dims, cfg, wy, wx, 0, None)


def _solve(lib, cfg, x=FAKE, wy=FAKE, wx=FAKE, dims=(1, 2, 8, 8, 4, 4), ws_bytes=1 << 30, slots=(FAKE, FAKE, FAKE), iters=1):
    return lib.asr_sr_solve_wtv_f32(x, FAKE, FAKE, FAKE, FAKE, FAKE, *slots, FAKE, iters, None, FAKE, ws_bytes, *dims,
                                    1.0, 0.3, 0.0, 0.0, cfg, wy, wx, 1, None)


def test_edge_weights_refusals(lib):
    f = lib.asr_tv_edge_weights_f32
    assert f(None, FAKE, FAKE, 1, 4, 4, 1.0, None) == INVALID and b"null pointer" in lib.asr_last_error()
    assert f(FAKE, None, FAKE, 1, 4, 4, 1.0, None) == INVALID
    assert f(FAKE, FAKE, None, 1, 4, 4, 1.0, None) == INVALID
    for batch, H, W in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (1, -3, 4), (65536, 4, 4)):
        assert f(FAKE, FAKE, FAKE, batch, H, W, 1.0, None) == INVALID, (batch, H, W)
        assert b"bad shape" in lib.asr_last_error()
    for beta in (-1.0, -1e-30, float("inf"), float("-inf"), float("nan")):
        assert f(FAKE, FAKE, FAKE, 1, 4, 4, beta, None) == INVALID, beta
        assert b"finite and >= 0" in lib.asr_last_error()


def test_weighted_entry_points_refuse_null_weights_and_bilateral_tv(lib):
    cfg = _cfg()
    for call in (_backward, _terms, _solve):
        assert call(lib, C.byref(cfg), wy=None) == INVALID and b"wy, wx" in lib.asr_last_error()
        assert call(lib, C.byref(cfg), wx=None) == INVALID and b"wy, wx" in lib.asr_last_error()
        assert call(lib, C.byref(cfg), x=None) == INVALID and b"null pointer" in lib.asr_last_error()
        assert call(lib, None) == INVALID and b"null config" in lib.asr_last_error()
        btv = _cfg(use_btv=True)
        assert call(lib, C.byref(btv)) == UNSUPPORTED
        assert b"bilateral TV has no weighted form here" in lib.asr_last_error()
    # H or W < 1
    for dims in ((1, 2, 0, 8, 4, 4), (1, 2, 8, 0, 4, 4), (1, 2, -8, 8, 4, 4)):
        for call in (_backward, _terms, _solve):
            assert call(lib, C.byref(cfg), dims=dims) == INVALID, dims


def test_weighted_entry_points_keep_the_refusals_of_their_twins(lib):
    from asr_amd import _lib
    cfg = _cfg()
    # shapes: an odd factor, f = 1, unequal factors
    for dims in ((1, 2, 12, 12, 4, 4), (1, 2, 8, 8, 8, 8), (1, 2, 8, 16, 4, 4)):
        assert _backward(lib, C.byref(cfg), dims=dims) == UNSUPPORTED, dims
        assert _solve(lib, C.byref(cfg), dims=dims) == UNSUPPORTED, dims
    assert _backward(lib, C.byref(cfg), dims=(66000, 1, 8, 8, 4, 4)) == INVALID and b"grid.z" in lib.asr_last_error()
    # backward: nothing to produce, x_new without alphas, x_new aliasing x, missing slots
    assert _backward(lib, C.byref(cfg), grad=None) == INVALID and b"x_new and/or grad_out" in lib.asr_last_error()
    assert _backward(lib, C.byref(cfg), x_new=FAKE + 4096) == INVALID and b"alphas required" in lib.asr_last_error()
    assert _backward(lib, C.byref(cfg), x_new=FAKE) == INVALID
    # config: optimizer, prior, bilateral-TV window, plane_chunk, slots, workspace
    bad = _cfg(); bad.optimizer = 9
    assert _solve(lib, C.byref(bad)) == INVALID and b"unknown optimizer" in lib.asr_last_error()
    bad = _cfg(); bad.prior = 7
    assert _terms(lib, C.byref(bad)) == INVALID and b"unknown prior" in lib.asr_last_error()
    bad = _cfg(use_btv=True, btv_shift=9)
    assert _terms(lib, C.byref(bad)) == INVALID and b"btv_shift" in lib.asr_last_error()
    bad = _cfg(plane_chunk=-1)
    assert _solve(lib, C.byref(bad)) == INVALID and b"plane_chunk" in lib.asr_last_error()
    assert _solve(lib, C.byref(cfg), slots=(FAKE, FAKE, None)) == INVALID and b"slot buffers" in lib.asr_last_error()
    assert _solve(lib, C.byref(cfg), iters=-1) == INVALID and b"num_iter" in lib.asr_last_error()
    assert _solve(lib, C.byref(cfg), ws_bytes=16) == _lib.load().asr_sr_solve_cfg_f32(
        FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 1, None, FAKE, 16, 1, 2, 8, 8, 4, 4, 1.0, 0.3, 0.0, 0.0,
        C.byref(cfg), None) == -4
    assert b"workspace" in lib.asr_last_error()
    assert _terms(lib, C.byref(cfg), dims=(0, 2, 8, 8, 4, 4)) == INVALID and b"bad batch" in lib.asr_last_error()
    assert lib.asr_abi_version() == 3


def test_ops_shape_checks():
    from asr_amd import ops
    from asr_amd._lib import AsrError
    x, resid = torch.zeros(2, 8, 8), torch.zeros(2, 3, 4, 4)
    tf = torch.zeros(2, 3, 8)
    cfg = ops.sr_config()
    good = (torch.ones(8, 8), torch.ones(8, 8))
    assert ops._tv_weights(good, x, "t")[2] == 1                              # [H, W]: shared
    assert ops._tv_weights((torch.ones(2, 8, 8), torch.ones(2, 8, 8)), x, "t")[2] == 0
    bad = [(torch.ones(8, 8),), torch.ones(8, 8), (torch.ones(8, 8), torch.ones(8, 4)), (torch.ones(4, 8), torch.ones(4, 8)),
           (torch.ones(3, 8, 8), torch.ones(3, 8, 8)), (torch.ones(1, 8, 8), torch.ones(1, 8, 8)),
           (torch.ones(8, 8), torch.ones(2, 8, 8)), (torch.ones(8, 8, dtype=torch.float64), torch.ones(8, 8)),
           (torch.ones(8, 16)[:, ::2], torch.ones(8, 8)), (np.ones((8, 8), np.float32), np.ones((8, 8), np.float32))]
    for w in bad:
        with pytest.raises(AsrError):
            ops.sr_backward(x, resid, tf, tf, (1, 0.3, 0, 0), cfg, tv_weights=w)
        with pytest.raises(AsrError):
            ops.sr_loss_terms(x, resid, cfg, tv_weights=w)
        with pytest.raises(AsrError):
            ops.sr_solve(x, resid, tf, tf, tf, tf, torch.zeros(1, 2), (1, 0.3, 0, 0), cfg=cfg, tv_weights=w)
    for g in (torch.zeros(8, 8), torch.zeros(8, 8, 1), torch.zeros(8, 8, 4), torch.zeros(2, 2, 8, 8, 3), torch.zeros(0, 8, 3),
              torch.zeros(8, 8, 3, dtype=torch.float64), torch.zeros(8, 8, 6)[..., ::2], np.zeros((8, 8, 3), np.float32)):
        with pytest.raises(AsrError):
            ops.tv_edge_weights(g, 1.0)
    for beta in (-1.0, float("nan"), float("inf"), "x", None, True):
        with pytest.raises(ValueError):
            ops.tv_edge_weights(torch.zeros(8, 8, 3), beta)
    assert ops.check_tv_beta(0) == 0.0 and ops.check_tv_beta(np.float32(10)) == 10.0
    for fn in (ops.sr_backward, ops.sr_loss_terms, ops.sr_solve):
        assert inspect.signature(fn).parameters["tv_weights"].default is None


def test_superresolution_refuses_a_guide_it_cannot_use():
    from asr_amd.superresolution_scripts.superresolution import Superresolution
    guide = np.zeros((8, 8, 3), np.float32)
    btv = Superresolution(1, 0.3, 0, 0, num_iter=2, num_aug=2, feature_size=(4, 4), output_size=(8, 8), use_BTV=True)
    for call in (lambda: btv.augmented_superresolution([], [], [], tv_guide=guide),
                 lambda: btv.augmented_superresolution_batch(None, [], [], tv_guide=guide),
                 lambda: btv.augmented_superresolution_classes(None, [], [], [], tv_guide=guide),
                 lambda: btv.loss_function(None, [], [], [], tv_guide=guide)):
        with pytest.raises(ValueError, match="bilateral TV"):
            call()
    sr = Superresolution(1, 0.3, 0, 0, num_iter=2, num_aug=2, feature_size=(4, 4), output_size=(8, 8))
    assert sr.tv_beta == 100.0
    for bad in (np.zeros((8, 8), np.float32), np.zeros((8, 8, 1), np.float32), np.zeros((16, 16, 3), np.float32),
                torch.zeros(2, 8, 4, 3), np.zeros((1, 2, 8, 8, 3), np.float32)):
        with pytest.raises(ValueError, match="output_size"):
            sr.augmented_superresolution([], [], [], tv_guide=bad)
        with pytest.raises(ValueError, match="output_size"):
            sr.loss_function(None, [], [], [], tv_guide=bad)
    for beta in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tv_beta"):
            Superresolution(1, 0.3, 0, 0, tv_beta=beta)
    for name in ("augmented_superresolution", "augmented_superresolution_batch", "augmented_superresolution_classes",
                 "loss_function"):
        assert inspect.signature(getattr(Superresolution, name)).parameters["tv_guide"].default is None
    assert inspect.signature(Superresolution.__init__).parameters["tv_beta"].default == 100.0


def test_run_image_labels_refuses_a_tv_guide_it_cannot_use():
    from asr_amd.pipeline import HotPath
    path = HotPath(None, types.SimpleNamespace(output_size=(8, 8), use_BTV=False))
    run = lambda image, beta: path.run_image_labels(image, [], [], class_ids=[3], tv_guide=beta)
    for beta in (-1.0, float("nan"), float("inf"), float("-inf"), "100", (4, 1e-3), True):
        with pytest.raises(ValueError, match="beta"):
            run(torch.zeros(8, 8, 3), beta)
    for image in (torch.zeros(8, 8, 1), torch.zeros(16, 16, 3), torch.zeros(8, 8)):
        with pytest.raises(ValueError, match="SR output size"):
            run(image, 100.0)
    btv = HotPath(None, types.SimpleNamespace(output_size=(8, 8), use_BTV=True))
    with pytest.raises(ValueError, match="bilateral TV"):
        btv.run_image_labels(torch.zeros(8, 8, 3), [], [], class_ids=[3], tv_guide=100.0)
    assert path.check_tv_guide(None, None) is None and path.check_tv_guide(0, (8, 8, 3)) == 0.0


def test_label_options_is_unchanged_and_the_keywords_default_to_off():
    from asr_amd import evaluation
    from asr_amd.pipeline import HotPath, LabelOptions
    from asr_amd.superresolution_scripts import superres_utils as su
    assert LabelOptions._fields == ("bands", "band_ignore", "n_conf", "factors", "guide", "covs", "sizes", "min_region",
                                    "segments")
    assert list(inspect.signature(HotPath.label_options).parameters) == [
        "self", "image_shape", "has_gt", "band_widths", "band_ignore_label", "confusion_labels", "th_factors", "guide",
        "coverages", "keep_uncertainty", "min_region", "segments"]
    assert inspect.signature(HotPath.run_image_labels).parameters["tv_guide"].default is None
    assert inspect.signature(evaluation.evaluate_labelmaps).parameters["tv_guide"].default is None
    sig = inspect.signature(su.compute_SR).parameters
    assert sig["tv_guide"].default is None and list(sig)[-4:] == ["tv_guide", "guide", "guide_radius", "guide_eps"]
    with pytest.raises(ValueError, match="'aug'"):
        su.compute_SR(None, [], [], [], "x", "unused", SR_type="mean", tv_guide=np.zeros((8, 8, 3), np.float32))


def test_compute_SR_hands_the_tv_guide_to_the_solve_and_nothing_without_it(monkeypatch, tmp_path):
    from asr_amd.superresolution_scripts import superres_utils as su
    target = np.arange(12, dtype=np.float32).reshape(3, 4, 1)
    seen = []

    def solve(masks, a, s, **kw):
        seen.append(kw)
        return target, None

    sr = types.SimpleNamespace(augmented_superresolution=solve)
    monkeypatch.setattr(su, "threshold_image", lambda image, th_value, th_factor=.15, th_mask=None: "mask")
    assert su.compute_SR(sr, [0], [0], [0], "x", str(tmp_path), SR_type="aug") == "mask"
    assert su.compute_SR(sr, [0], [0], [0], "x", str(tmp_path), SR_type="aug", max_masks=[1], tv_guide="G") == "mask"
    assert seen == [{}, {"tv_guide": "G"}, {"tv_guide": "G"}]


def test_validate_labelmap_parser():
    spec = importlib.util.spec_from_file_location("validate_labelmap_wtv", os.path.join(ROOT, "scripts", "validate_labelmap.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    base = ["--images", "a", "--gt", "b"]
    assert mod.parser.parse_args(base).tv_guide_beta is None
    args = mod.parser.parse_args(base + ["--tv_guide_beta", "100", "--guide_radius", "4"])
    assert args.tv_guide_beta == 100.0 and args.guide_radius == 4
    with pytest.raises(SystemExit):
        mod.parser.parse_args(base + ["--tv_guide_beta", "much"])
    # the value is checked by the parser, before any model or image is touched: the script itself, once
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "validate_labelmap.py")] + base + ["--tv_guide_beta=-1"],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "--tv_guide_beta: beta must be a finite number >= 0" in r.stderr


@pytest.mark.parametrize("H,W,h,w,n", [(32, 32, 8, 8, 3), (24, 40, 6, 10, 2)])
def test_unit_weights_restate_the_oracles_tv_gradient_bit_for_bit(H, W, h, w, n):
    rng = np.random.default_rng(3)
    lam = (1.0, 0.3, 0.7, 0.05)
    x = torch.from_numpy(rng.standard_normal((1, H, W, 1)).astype(np.float32))
    x[0, 3:6, 4:9, 0] = 0.5                                                    # flat patches: sign(0) on both sides
    y = torch.from_numpy(rng.random((n, h, w, 1), dtype=np.float32))
    angles = rng.uniform(-0.2, 0.2, n).astype(np.float32)
    shifts = rng.uniform(-3, 3, (n, 2)).astype(np.float32)
    kw = dict(num_aug=n, feature_size=(h, w), output_size=(H, W))
    ones = np.ones((H, W), np.float32)
    loss_o, grad_o = o_sr.Superresolution(*lam, **kw).loss_and_grad(x, y, angles, shifts)
    ref = R.WeightedSuperresolution(*lam, wy=ones, wx=ones, **kw)
    loss_r, grad_r = ref.loss_and_grad(x, y, angles, shifts)
    assert torch.equal(grad_o, grad_r)
    assert abs(float(loss_o) - float(loss_r)) <= 1e-5 * abs(float(loss_o))
    dy, dx = tf_ops.image_gradients(x)
    assert abs(ref.tv(x) - float(torch.sum((torch.abs(dy) + torch.abs(dx)).double()))) == 0.0
    # zero weights: the gradient of lambda_tv = 0
    zeros = np.zeros((H, W), np.float32)
    _, grad_z = R.WeightedSuperresolution(*lam, wy=zeros, wx=zeros, **kw).loss_and_grad(x, y, angles, shifts)
    _, grad_0 = o_sr.Superresolution(lam[0], 0.0, lam[2], lam[3], **kw).loss_and_grad(x, y, angles, shifts)
    assert torch.equal(grad_z, grad_0)
    # the weights themselves: ones for beta = 0 and for a constant guide, the last row / column always one
    g = rng.random((H, W, 3), dtype=np.float32)
    for wt in R.edge_weights(g, 0.0) + R.edge_weights(np.full((H, W, 3), 0.25, np.float32), 100.0):
        assert np.array_equal(wt, ones)
    wy, wx = R.edge_weights(g, 100.0)
    assert np.all(wy[-1] == 1.0) and np.all(wx[:, -1] == 1.0) and wy[:-1].max() < 1.0 and wy.min() > 0.0
    a = g[1, 2] - g[0, 2]
    d = np.float32(np.float32(a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
    assert wy[0, 2] == np.float32(1.0) / (np.float32(1.0) + np.float32(100.0) * d)
