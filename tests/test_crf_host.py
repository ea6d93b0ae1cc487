"""The windowed CRF's host side, without a GPU: the workspace arithmetic, every refusal of the C entry points (before any launch:
no device is touched), ops.check_crf, run_image_labels' refusals, where the keyword sits, and the unit's build flags."""
import ctypes as C
import importlib.util
import inspect
import os
import types

import numpy as np
import pytest
import torch

from conftest import ROOT

FAKE = 1 << 20                                   # non-null, aligned; never dereferenced: every call below is refused on the host
INVALID, UNSUPPORTED = -1, -2


def config(**kw):
    from asr_amd import _lib
    fields = dict(radius=3, dilation=1, iterations=5, w_app=4.0, w_smooth=1.0, theta_pos=2.0, theta_rgb=0.1, theta_smooth=1.0)
    fields.update(kw)
    return _lib.CrfConfig(**fields)


def ids(*values):
    return (C.c_int * max(len(values), 1))(*values)


def refine(lib, cfg, L=3, H=8, W=8, id_list=(1, 2), guide=FAKE, z=FAKE, ws=FAKE, labels=FAKE, q=None):
    return lib.asr_crf_refine_f32(guide, z, ids(*id_list), L, H, W, C.byref(cfg) if cfg is not None else None, ws, labels, q, None)


def test_workspace_bytes_is_host_arithmetic(lib):
    assert lib.asr_crf_workspace_bytes(21, 512, 512) == 2 * 4 * 21 * 512 * 512
    assert lib.asr_crf_workspace_bytes(2, 1, 1) == 16
    assert lib.asr_crf_workspace_bytes(32, 3, 65) == 2 * 4 * 32 * 3 * 65
    assert lib.asr_crf_workspace_bytes(21, 40000, 40000) == 2 * 4 * 21 * 40000 * 40000            # no 32-bit wrap
    for bad in ((1, 8, 8), (33, 8, 8), (3, 0, 8), (3, 8, 0), (0, 8, 8), (-1, 8, 8)):
        assert lib.asr_crf_workspace_bytes(*bad) == 0


def test_refine_refuses_bad_values_and_names_its_caps(lib):
    err = lambda: lib.asr_last_error().decode()
    assert refine(lib, config(radius=8)) == UNSUPPORTED and "cap of 7" in err()
    assert refine(lib, config(radius=5, dilation=4)) == UNSUPPORTED and "cap of 16" in err()
    assert refine(lib, config(radius=1, dilation=17)) == UNSUPPORTED and "cap of 16" in err()
    assert refine(lib, config(iterations=33)) == UNSUPPORTED and "cap of 32" in err()
    assert refine(lib, config(), L=33, id_list=tuple(range(1, 33))) == UNSUPPORTED and "cap of 32" in err()
    for bad, word in ((dict(radius=0), "radius"), (dict(radius=-1), "radius"), (dict(dilation=0), "dilation"),
                      (dict(iterations=-1), "iterations"), (dict(w_app=-1.0), "w_app"), (dict(w_app=float("nan")), "w_app"),
                      (dict(w_smooth=float("inf")), "w_smooth"), (dict(w_smooth=-0.5), "w_smooth"),
                      (dict(theta_pos=0.0), "theta_pos"), (dict(theta_rgb=-0.1), "theta_rgb"),
                      (dict(theta_rgb=float("nan")), "theta_rgb"), (dict(theta_smooth=0.0), "theta_smooth"),
                      (dict(theta_smooth=float("inf")), "theta_smooth")):
        assert refine(lib, config(**bad)) == INVALID and word in err(), bad
    assert refine(lib, config(), L=1, id_list=()) == INVALID and "labels" in err()
    assert refine(lib, config(), H=0) == INVALID and "shape" in err()
    assert refine(lib, config(), W=-3) == INVALID and "shape" in err()
    assert refine(lib, config(), id_list=(1, 1)) == INVALID and "twice" in err()
    assert refine(lib, config(), id_list=(0, 2)) == INVALID and "fallback" in err()
    assert refine(lib, config(), id_list=(-4, 2)) == INVALID
    assert refine(lib, config(), ws=FAKE + 2) == INVALID and "aligned" in err()
    span = 4 * 3 * 8 * 8                                    # q_out may not overlap z, in whole or in part
    for q in (FAKE, FAKE + span - 4, FAKE - span + 4):
        assert refine(lib, config(), q=q) == INVALID and "overlap" in err(), q
    for null in ("guide", "z", "ws", "labels"):
        assert refine(lib, config(), **{null: None}) == INVALID and "null pointer" in err(), null
    assert refine(lib, None) == INVALID and "null pointer" in err()
    assert lib.asr_crf_refine_f32(FAKE, FAKE, None, 3, 8, 8, C.byref(config()), FAKE, FAKE, None, None) == INVALID
    # a cap and a bad value together: the bad value is reported
    assert refine(lib, config(radius=9, dilation=0)) == INVALID and "dilation" in err()


def test_unary_entry_points_refuse_before_any_launch(lib):
    err = lambda: lib.asr_last_error().decode()
    scores = lambda scores=FAKE, ws=FAKE, z=FAKE, pixels=64, K=2, th=0.15, tau=0.1: lib.asr_crf_unaries_scores_f32(
        scores, ws, z, pixels, K, th, tau, None)
    for null in ("scores", "ws", "z"):
        assert scores(**{null: None}) == INVALID and "null pointer" in err()
    assert scores(pixels=0) == INVALID and "shape" in err()
    assert scores(K=0) == INVALID and "score planes" in err()
    assert scores(K=32) == UNSUPPORTED and "cap of 31" in err()
    for tau in (0.0, -0.1, float("nan"), float("inf")):
        assert scores(tau=tau) == INVALID and "tau" in err()
    assert scores(th=float("nan")) == INVALID and "th_factor" in err()
    labels = lambda lab=FAKE, z=FAKE, pixels=64, id_list=(3, 5), L=3, conf=0.7: lib.asr_crf_unaries_labels_f32(
        lab, z, pixels, ids(*id_list), L, conf, None)
    assert labels(lab=None) == INVALID and "null pointer" in err()
    assert labels(z=None) == INVALID and "null pointer" in err()
    assert labels(pixels=0) == INVALID and "shape" in err()
    assert labels(L=1, id_list=()) == INVALID and "labels" in err()
    assert labels(L=33, id_list=tuple(range(1, 33))) == UNSUPPORTED and "cap of 32" in err()
    assert labels(id_list=(3, 3)) == INVALID and "twice" in err()
    assert labels(id_list=(0, 3)) == INVALID and "fallback" in err()
    for conf in (1.0, 1.0 / 3.0, 0.2, 0.0, -1.0, float("nan"), 1.5):
        assert labels(conf=conf) == INVALID and "conf" in err(), conf
    assert lib.asr_crf_unaries_labels_f32(FAKE, FAKE, 64, None, 3, 0.7, None) == INVALID


def test_check_crf_defaults_and_errors():
    from asr_amd import ops
    p = ops.check_crf(None)
    assert p == ops.check_crf({}) == ops.check_crf(ops.CRF_DEFAULTS._asdict())
    assert p._fields == ("radius", "dilation", "iterations", "w_app", "w_smooth", "theta_pos", "theta_rgb", "theta_smooth")
    assert (p.radius, p.dilation, p.iterations, p.w_app, p.w_smooth, p.theta_pos, p.theta_smooth) == (3, 1, 5, 4.0, 1.0, 2.0, 1.0)
    assert p.theta_rgb == float(np.float32(0.1))
    q = ops.check_crf({"radius": np.int64(4), "dilation": 4, "iterations": 0, "w_app": 0, "theta_rgb": 0.05})
    assert (q.radius, q.dilation, q.iterations, q.w_app, q.theta_rgb) == (4, 4, 0, 0.0, float(np.float32(0.05)))
    assert isinstance(q.radius, int) and isinstance(q.w_app, float)
    for bad, word in (({"radius": 0}, "radius 0 below 1"), ({"radius": 8}, "cap of 7"), ({"radius": 2.5}, "integer"),
                      ({"radius": True}, "integer"), ({"radius": "3"}, "integer"), ({"radius": float("nan")}, "integer"),
                      ({"iterations": float("inf")}, "integer"), ({"dilation": None}, "integer"),
                      ({"dilation": 0}, "dilation 0 below 1"),
                      ({"radius": 5, "dilation": 4}, "cap of 16"), ({"iterations": -1}, "iterations"),
                      ({"iterations": 33}, "cap of 32"), ({"w_app": -1}, "w_app must be finite and >= 0"),
                      ({"w_smooth": float("nan")}, "w_smooth must be finite and >= 0"),
                      ({"theta_pos": 0}, "theta_pos must be finite and > 0"),
                      ({"theta_rgb": float("inf")}, "theta_rgb must be finite and > 0"),
                      ({"theta_smooth": -1}, "theta_smooth must be finite and > 0"), ({"sigma": 1}, "unknown field"),
                      ({"tau": 0.1}, "unknown field")):
        with pytest.raises(ValueError, match=word):
            ops.check_crf(bad)
    assert ops.check_crf_tau(0.1) == float(np.float32(0.1))
    for tau in (0, -1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tau"):
            ops.check_crf_tau(tau)
    assert ops.check_crf_conf(0.7, 21) == float(np.float32(0.7))
    for conf, n in ((1.0, 3), (0.3, 3), (0.0, 3), (float("nan"), 3), (np.float32(1) / np.float32(3), 3), (1 / 3, 3)):
        with pytest.raises(ValueError, match="conf"):
            ops.check_crf_conf(conf, n)


def test_check_crf_and_the_c_checks_agree_on_the_wording(lib):
    from asr_amd import ops
    for bad in (dict(radius=8), dict(radius=5, dilation=4), dict(iterations=33), dict(radius=0), dict(w_app=-1.0),
                dict(theta_rgb=0.0)):
        assert refine(lib, config(**bad)) < 0
        c_text = lib.asr_last_error().decode().split(": ", 1)[1]
        with pytest.raises(ValueError) as e:
            ops.check_crf(bad)
        py_text = str(e.value).split(": ", 1)[1]
        assert py_text.split(" (")[0] == c_text.split(" (")[0], (py_text, c_text)


def test_ops_refuse_host_tensors_and_bad_shapes():
    from asr_amd import _lib, ops
    with pytest.raises(ValueError, match=r"\[H, W, 3\]"):
        ops.crf_refine(torch.zeros(8, 8), torch.zeros(3, 8, 8), [1, 2])
    with pytest.raises(ValueError, match="z must be"):
        ops.crf_refine(torch.zeros(8, 8, 3), torch.zeros(2, 8, 8), [1, 2])
    with pytest.raises(_lib.AsrError, match="CPU"):
        ops.crf_refine(torch.zeros(8, 8, 3), torch.zeros(3, 8, 8), [1, 2])
    with pytest.raises(ValueError, match="scores must be"):
        ops.crf_unaries(torch.zeros(32, 4, 4), 0.15)
    with pytest.raises(ValueError, match="tau"):
        ops.crf_unaries(torch.zeros(2, 4, 4), 0.15, tau=0.0)
    with pytest.raises(ValueError, match="conf"):
        ops.crf_unaries_from_labels(torch.zeros(4, 4, dtype=torch.int32), [1, 2], 0.2)


def test_run_image_labels_refuses_a_crf_it_cannot_use():
    from asr_amd.pipeline import CrfOptions, HotPath
    sr = types.SimpleNamespace(output_size=(8, 8), use_BTV=False)
    path = HotPath(None, sr)
    image = torch.zeros(8, 8, 3)
    run = lambda p=path, img=image, **kw: p.run_image_labels(img, [], [], class_ids=[3, 5], **kw)
    with pytest.raises(ValueError, match="slice_max"):
        run(HotPath(None, sr, mode="slice_max"), crf={})
    with pytest.raises(ValueError, match="th_factors with crf"):
        run(crf={"iterations": 3}, th_factors=[0.1, 0.2], gt_dev=torch.zeros(8, 8, dtype=torch.int32))
    for bad in (torch.zeros(8, 8, 1), torch.zeros(16, 16, 3), torch.zeros(8, 8)):
        with pytest.raises(ValueError, match="SR output size"):
            run(img=bad, crf={})
    for bad, word in (({"radius": 8}, "cap of 7"), ({"tau": 0}, "tau"), ({"standard_conf": 0.2}, "conf"),
                      ({"standard_conf": 1.0}, "conf"), ({"sigma": 2}, "unknown field"), ((3, 1), "dict"), (5, "dict")):
        with pytest.raises(ValueError, match=word):
            run(crf=bad)
    bare = HotPath(None, None)                               # mode, sweep and the fields are refused before self.sr is read
    with pytest.raises(ValueError, match="slice_max"):
        HotPath(None, None, mode="slice_max").run_image_labels(None, [], [], class_ids=[3], crf={})
    with pytest.raises(ValueError, match="th_factors with crf"):
        bare.run_image_labels(None, [], [], class_ids=[3], crf={}, th_factors=[0.2], gt_dev=torch.zeros(1))
    with pytest.raises(ValueError, match="iterations above the cap of 32"):
        bare.run_image_labels(None, [], [], class_ids=[3], crf={"iterations": 33})
    assert bare.check_crf(None, None) is None
    assert path.check_crf(None, None) is None
    with pytest.raises(ValueError, match="32 class ids above the cap of 31"):       # L = K + 1 <= 32: refused before the model
        path.run_image_labels(image, [], [], class_ids=range(1, 33), crf={})
    assert path.check_crf({}, (8, 8, 3), None, 31) is not None
    got = path.check_crf({"iterations": 3, "tau": 0.2, "standard_conf": 0.7}, (8, 8, 3), None, 2)
    assert isinstance(got, CrfOptions) and got.params.iterations == 3 and got.params.radius == 3
    assert got.tau == float(np.float32(0.2)) and got.standard_conf == float(np.float32(0.7))
    assert path.check_crf({}, (8, 8, 3)).standard_conf is None


def test_the_keyword_sits_after_tv_guide_in_both_functions():
    from asr_amd import evaluation
    from asr_amd.pipeline import HotPath
    from asr_amd.superresolution_scripts import superres_utils as su
    names = list(inspect.signature(HotPath.run_image_labels).parameters)
    assert names[names.index("tv_guide") + 1] == "crf" and names[-2:] == ["crf", "segments"]
    assert inspect.signature(HotPath.run_image_labels).parameters["crf"].default is None
    names = list(inspect.signature(evaluation.evaluate_labelmaps).parameters)
    assert names[names.index("tv_guide") + 1] == "crf"
    assert inspect.signature(evaluation.evaluate_labelmaps).parameters["crf"].default is None
    assert list(inspect.signature(su.crf_labels).parameters)[:4] == ["scores", "guide", "class_ids", "th_factor"]


def test_the_unit_is_a_later_source_with_its_flags():
    spec = importlib.util.spec_from_file_location(
        "asr_build", os.path.join(ROOT, "deeplabv3plus-augmented-superresolution_amd", "csrc", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    flags = dict(b.ALL_SOURCES)["crf.hip"]
    assert "-ffp-contract=off" in flags and "-packed-fp32-ops" in flags
    assert "crf.hip" in dict(b.LATER_SOURCES) and "crf.hip" not in dict(b.SOURCES) and "crf.hip" not in b.POSTPASS
    assert b.LATER_SOURCES[-1][0] == "crf.hip"
