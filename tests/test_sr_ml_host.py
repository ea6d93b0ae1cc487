"""CPU: the multi-label coupling's restatement tests/sr_ml_ref.py (the projection rule of include/asr_hip.h, "multi-label
coupling", the group stop rule) against the exact float64 projection, and the host refusals of the Python surface."""
import numpy as np
import pytest
import torch

import sr_ml_ref as M

GROUPS = (1, 2, 3, 5, 21, 32)
F = np.float32


def _inputs(G, seed=0, pixels=4000):
    """normal(0.3, 0.6) columns of G values, plus columns scaled so that many sums lie just above and below 1."""
    rng = np.random.default_rng(seed + G)
    v = rng.normal(0.3, 0.6, (G, pixels)).astype(np.float32)
    v[:, ::7] = (v[:, ::7] / np.float32(max(G, 1))).astype(np.float32)
    return v


@pytest.mark.parametrize("G", GROUPS)
def test_the_restatement_is_the_exact_projection_to_1e_6(G):
    v = _inputs(G)
    got = M.simplex_project(v)
    want = M.exact_projection(v)
    diff = float(np.abs(got.astype(np.float64) - want).max())
    s = got[0].astype(np.float32)
    for j in range(1, G):
        s = (s + got[j]).astype(np.float32)
    exact_sum = float(got.astype(np.float64).sum(axis=0).max())
    print(f"G={G}: max |restatement - exact| {diff:.3e}, min {float(got.min()):.3e}, max float32 sum {float(s.max()):.9f}, "
          f"max exact sum {exact_sum:.9f}")
    assert got.dtype == np.float32
    assert diff <= 1e-6
    assert float(got.min()) >= 0.0
    assert float(s.max()) <= 1.0 + 2e-6 and exact_sum <= 1.0 + 2e-6
    assert (np.maximum(v, 0).sum(axis=0) > 1).any() and (np.maximum(v, 0).sum(axis=0) < 1).any()     # both branches ran


@pytest.mark.parametrize("G", GROUPS)
def test_feasible_inputs_come_back_bit_for_bit(G):
    rng = np.random.default_rng(10 + G)
    v = (rng.random((G, 500), dtype=np.float32) / np.float32(G)).astype(np.float32)      # every sum < 1 up to rounding
    v[:, :50] = 0.0
    s = v[0].copy()
    for j in range(1, G):
        s = (s + v[j]).astype(np.float32)
    v = v[:, s <= 1.0]
    assert v.shape[1] > 400
    v[0, 0] = F(1.0)                                             # an exact sum of 1
    v[1:, 0] = F(0.0)
    got = M.simplex_project(v)
    assert got.tobytes() == v.tobytes()
    # -0 and negatives become +0, the rest of a feasible column is untouched
    w = v.copy()
    w[0, 1] = F(-0.0)
    w[0, 2] = F(-3.0)
    got = M.simplex_project(w)
    assert got[0, 1] == 0 and not np.signbit(got[0, 1]) and got[0, 2] == 0
    assert got[1:].tobytes() == w[1:].tobytes()


@pytest.mark.parametrize("G", GROUPS)
def test_the_result_does_not_depend_on_the_order_of_equal_values(G):
    """Columns with repeated values: any permutation of the column permutes the result with it -- for G >= 3 up to the order of
    the float32 sum, so the permutations tried here swap EQUAL values only, which leaves the sum's operands in place."""
    rng = np.random.default_rng(20 + G)
    v = rng.choice(np.array([0.0, 0.25, 0.5, 0.75, 1.0], np.float32), size=(G, 300)).astype(np.float32)
    got = M.simplex_project(v)
    for col in range(v.shape[1]):
        for val in np.unique(v[:, col]):
            idx = np.flatnonzero(v[:, col] == val)
            assert (got[idx, col] == got[idx[0], col]).all()      # equal inputs, equal outputs: their order cannot matter
    # and a descending sort that breaks ties the other way gives the same theta: project the column reversed
    if G >= 2:
        rev = M.simplex_project(v[::-1].copy())[::-1]
        same_sum = np.ones(v.shape[1], bool)
        if G >= 3:                                               # reversing changes the order of the float32 sum itself
            a = np.maximum(v, 0)
            s1, s2 = a[0].copy(), a[-1].copy()
            for j in range(1, G):
                s1 = (s1 + a[j]).astype(np.float32)
                s2 = (s2 + a[G - 1 - j]).astype(np.float32)
            same_sum = (s1 > 1) == (s2 > 1)
        assert np.array_equal(rev[:, same_sum], got[:, same_sum])


def test_the_group_stop_rule_on_hand_made_losses():
    # two members whose sum stalls although one of them still improves
    losses = [[10.0, 10.0], [9.0, 11.0], [8.0, 12.0], [7.0, 13.0]]
    assert M.group_stop(losses, rel_tol=1e-3, patience=2) == 2
    assert M.group_stop(losses, rel_tol=1e-3, patience=1) == 1
    assert M.group_stop(losses, rel_tol=1e-3, patience=0) is None
    assert M.group_stop(losses, rel_tol=1e-3, patience=1, min_iter=3) == 3
    # a falling sum never stops; every = 2 reports the iteration, not the row
    falling = [[10.0, 10.0], [9.0, 10.0], [8.0, 10.0]]
    assert M.group_stop(falling, rel_tol=1e-3, patience=1) is None
    assert M.group_stop(losses, rel_tol=1e-3, patience=1, every=2) == 2
    # a group of one is the per-image rule; a NaN loss never improves
    assert M.group_stop([[5.0], [5.0], [5.0]], rel_tol=0.0, patience=2) == 2
    assert M.group_stop([[np.nan, 1.0]], rel_tol=0.0, patience=1) == 0
    # the sum runs in index order in float64: (1e16 + 1) + -1e16 is 0, not 1
    assert M.group_stop([[1e16, 1.0, -1e16], [0.5, 0.0, 0.0]], rel_tol=0.0, patience=1) == 1


def test_the_fusion_rule_restated():
    ids = [3, 7, 9]
    s = np.array([[0.6, 0.2, 0.5, 0.25, 0.0], [0.3, 0.2, 0.5, 0.25, 0.0], [0.0, 0.1, 0.0, 0.25, 0.0]], np.float32)
    # 0.6 > 0.1 -> 3; 0.2 > 0.5 fails -> 0; tie 0.5 / 0.5, bg 0 -> the first, 3; 0.25 == bg 0.25 -> 0 (strict); all zero -> 0
    assert M.fuse_labels_simplex(s, ids).tolist() == [3, 0, 3, 0, 0]


# ---- host refusals ---------------------------------------------------------------------------------------------------------------
def test_check_coupling():
    from asr_amd import _lib, ops
    pd = ops.sr_config(_lib.OPT_PRIMAL_DUAL, c0=1.0 / 16.0)
    assert ops.check_coupling(3, 6, pd) == 3 and ops.check_coupling(1, 5, pd) == 1 and ops.check_coupling(32, 64, pd) == 32
    assert ops.check_coupling(0, 5, ops.sr_config()) == 0                       # 0: the uncoupled solve, any rule
    assert ops.check_coupling(np.int64(2), 4, pd) == 2
    for bad in (-1, 33, 2.0, "3", True, None):
        with pytest.raises(ValueError, match="coupling"):
            ops.check_coupling(bad, 6, pd)
    with pytest.raises(ValueError, match="multiple"):
        ops.check_coupling(4, 6, pd)
    with pytest.raises(ValueError, match="primal-dual"):
        ops.check_coupling(3, 6, ops.sr_config())
    with pytest.raises(ValueError, match="primal-dual"):
        ops.check_coupling(3, 6, None)
    # ops.sr_solve refuses before anything touches a device
    x, y, tf = torch.zeros(2, 8, 8), torch.zeros(2, 3, 4, 4), torch.zeros(2, 3, 8)
    with pytest.raises(ValueError, match="coupling"):
        ops.sr_solve(x, y, tf, tf, tf, tf, torch.zeros(1, 2), (1, 0.3, 0, 0), cfg=ops.sr_config(), coupling=2)
    with pytest.raises(ValueError, match="coupling"):
        ops.sr_solve(torch.zeros(3, 8, 8), torch.zeros(3, 3, 4, 4), torch.zeros(3, 3, 8), tf, tf, tf, torch.zeros(1, 3),
                     (1, 0.3, 0, 0), cfg=pd, coupling=2)
    import inspect
    assert inspect.signature(ops.sr_solve).parameters["coupling"].default is None


def _sr(kind):
    from asr_amd.superresolution_scripts.optimizer import Optimizer
    from asr_amd.superresolution_scripts.superresolution import Superresolution
    opt = Optimizer("primal_dual") if kind == "primal_dual" else Optimizer("adam", 1e-3, amsgrad=True)
    return Superresolution(1.0, 0.3, 0.7, 0.0, num_iter=2, num_aug=2, optimizer=opt, feature_size=(4, 4), output_size=(8, 8))


def test_the_script_needs_the_primal_dual_optimizer_for_the_flag():
    import os
    import subprocess
    import sys
    from conftest import ROOT
    script = os.path.join(ROOT, "scripts", "validate_labelmap.py")
    base = [sys.executable, script, "--images", "a", "--gt", "b", "--couple_classes"]
    for extra, what in (([], "--couple_classes needs --sr_optimizer primal_dual"),
                        (["--sr_optimizer", "primal_dual", "--mode", "slice"], "--couple_classes in slice mode"),
                        (["--sr_optimizer", "primal_dual", "--th_factors", "0.1,0.2"], "--couple_classes with --th_sweep"),
                        (["--sr_optimizer", "primal_dual", "--crf_iters", "2"], "--couple_classes with --crf_iters")):
        r = subprocess.run(base + extra, capture_output=True, text=True, cwd=ROOT)
        assert r.returncode == 2 and what in r.stderr, (extra, r.stderr[-400:])
    r = subprocess.run([sys.executable, script, "--help"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0 and "--couple_classes" in r.stdout


def test_the_path_refuses_couple_before_any_device_call():
    """No model, no image, host tensors only: a refusal that came after the first launch would fail differently."""
    import inspect
    from asr_amd import evaluation as E
    from asr_amd.pipeline import HotPath
    from asr_amd.superresolution_scripts.superresolution import Superresolution
    assert inspect.signature(HotPath.run_image_labels).parameters["couple"].default is False
    assert inspect.signature(Superresolution.augmented_superresolution_classes).parameters["couple"].default is False
    assert inspect.signature(E.evaluate_labelmaps).parameters["couple"].default is False
    pd, adam = _sr("primal_dual"), _sr("adam")
    for mode in ("slice", "slice_max"):
        with pytest.raises(ValueError, match="couple in " + mode):
            HotPath(None, pd, mode=mode).run_image_labels(None, [], [], class_ids=[1, 2], couple=True)
    with pytest.raises(ValueError, match="th_factors with couple"):
        HotPath(None, pd, mode="argmax").run_image_labels(None, [], [], class_ids=[1, 2], couple=True, th_factors=[0.15, 0.5],
                                                          gt_dev=torch.zeros((8, 8), dtype=torch.int32))
    with pytest.raises(ValueError, match="crf with couple"):
        HotPath(None, pd, mode="argmax").run_image_labels(None, [], [], class_ids=[1, 2], couple=True, crf=dict(iterations=1))
    with pytest.raises(ValueError, match="primal_dual"):
        HotPath(None, adam, mode="argmax").run_image_labels(None, [], [], class_ids=[1, 2], couple=True)
    with pytest.raises(ValueError, match="True or False"):
        HotPath(None, pd, mode="argmax").run_image_labels(None, [], [], class_ids=[1, 2], couple=3)
    # the solver object itself, on host tensors
    with pytest.raises(ValueError, match="primal_dual"):
        adam.augmented_superresolution_classes(torch.zeros(2, 2, 4, 4), np.zeros(2), np.zeros((2, 2)), [0, 0], couple=True)
    # evaluate_labelmaps: before it lists, reads or draws anything
    with pytest.raises(ValueError, match="primal_dual"):
        E.evaluate_labelmaps(HotPath(None, adam, mode="argmax"), [], [], couple=True)
    with pytest.raises(ValueError, match="couple in slice"):
        E.evaluate_labelmaps(HotPath(None, pd, mode="slice"), [], [], couple=True)
