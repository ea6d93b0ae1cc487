"""The case table of tests/sr_option_cases.py without a device: its cases launch every option instantiation that csrc/sr.hip
has (the list is read from the source text itself, sr.hip with its #include "sr_*_kernels.h" sections spliced in, so a template
argument added later to any of them without a case fails here; the exact-adjoint forms have their cases in tests/sr_adj_cases.py), its
transform sets keep the bounds of test_gpu_sr_shapes._transform_set, and the "neutral" values of
tests/test_gpu_sr_option_shapes.py are neutral in the restatements that suite leans on."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle import sr as o_sr

import sr_dt_ref as RD
import sr_mon_ref as M
import sr_option_cases as T
import sr_pd_ref as P
import sr_wtv_ref as RW

SR_HIP = os.path.join(ROOT, "deeplabv3plus-augmented-superresolution_amd", "csrc", "sr.hip")


@pytest.fixture(scope="module")
def in_source():
    return T.source_instantiations(T.spliced_source(SR_HIP))        # sr.hip with its #include "sr_*_kernels.h" sections in place


# ---- 1. coverage ---------------------------------------------------------------------------------------------------------------------
def test_the_source_holds_the_hand_written_list_and_nothing_else(in_source):
    known = T.OPTION_KERNELS | T.SOLVER_HELPERS | T.OTHER_KERNELS | T.RW_KERNELS | T.ADJ_KERNELS
    print("in sr.hip and its sections:", len(in_source), "forms;", len(T.OPTION_KERNELS), "option instantiations")
    with open(SR_HIP) as f:                                            # the sections are read: sr.hip alone holds fewer forms
        assert T.source_instantiations(f.read()) < in_source
    assert len(T.RW_KERNELS) == 4 and len(T.ADJ_KERNELS) == 1 + 8
    assert in_source - known == set(), "launched in sr.hip, in no list of sr_option_cases.py"
    assert known - in_source == set(), "listed in sr_option_cases.py, launched nowhere in sr.hip"
    assert len(T.OPTION_KERNELS) == 5 + 8 + 8 + 4 + 4 + 9
    # the reader sees a form in each place sr.hip selects a kernel: a launch, a switch, a ?: initialiser, a template parameter
    later = ("hipLaunchKernelGGL((sr_forward_residual_kernel<true, true, true, true>), g, b, 0, s);\n"
             "        case 16: return sr_grad_translate_kernel<4, true>;\n"
             "    const auto k = w ? sr_backward_gather_kernel<true, true, 1> : sr_backward_gather_kernel<false, true, 1>;\n"
             "        default: return sr_backward_adam_kernel<0, WTV, 2>;\n")
    assert T.source_instantiations(later) == {
        "sr_forward_residual_kernel<true,true,true,true>", "sr_grad_translate_kernel<4,true>", "sr_backward_gather_kernel<true,true,1>",
        "sr_backward_gather_kernel<false,true,1>", "sr_backward_adam_kernel<0,false,2>", "sr_backward_adam_kernel<0,true,2>"}
    assert not T.source_instantiations(later) & known


def test_every_option_instantiation_has_a_case(in_source):
    by_kernel = {}
    for case in T.TABLE:
        for k in T.instantiations(case):
            by_kernel.setdefault(k, []).append(case)
    for k in sorted(T.OPTION_KERNELS):
        print(f"{k}: {len(by_kernel.get(k, []))} cases, e.g. {tuple(by_kernel[k][0]) if k in by_kernel else None}")
    launched = set(by_kernel)
    assert launched & T.OPTION_KERNELS == T.OPTION_KERNELS, sorted(T.OPTION_KERNELS - launched)
    assert launched - T.OPTION_KERNELS <= T.SOLVER_HELPERS, sorted(launched - T.OPTION_KERNELS - T.SOLVER_HELPERS)
    assert launched <= in_source
    # what the issue names: no suite ran these before
    for k in ("sr_grad_translate_kernel<3,true>", "sr_grad_translate_kernel<0,true>", "sr_backward_gather_pd_kernel<true,true>",
              "sr_backward_adam_kernel<3,true>", "sr_backward_adam_kernel<0,true>"):
        assert any(c.kind == "T2" for c in by_kernel[k]) and any(c.kind == "T0" for c in by_kernel[k]), k
    for k in ("sr_bound_maxima_kernel", "sr_bound_next_v_kernel", "sr_bound_out_kernel"):
        assert {T.factor(c.shape) for c in by_kernel[k]} >= {8, 6, 4} and {c.kind for c in by_kernel[k]} == {"T0", "T2"}
    stops = [c for c in T.TABLE if c.monitor == "stop" and c.chunk == 2]
    assert {T.factor(c.shape) for c in stops} >= {8, 6}


def test_every_exact_adjoint_form_has_a_case_on_rotations_and_on_the_counted_loop(in_source):
    """The kernels of the included section csrc/sr_adj_kernels.h against the table of tests/sr_adj_cases.py."""
    import sr_adj_cases as TA
    by_kernel = {}
    for case in TA.TABLE:
        for k in TA.instantiations(case):
            by_kernel.setdefault(k, []).append(case)
    assert set(by_kernel) <= in_source
    assert set(by_kernel) - T.ADJ_KERNELS <= T.OPTION_KERNELS | T.SOLVER_HELPERS        # the unchanged forward / grad-translate forms
    assert {f"sr_grad_translate_kernel<{L}>" for L in (0, 1, 2, 3)} <= set(by_kernel)
    for k in sorted(T.ADJ_KERNELS):
        families = {c.family for c in by_kernel.get(k, [])}
        print(f"{k}: {len(by_kernel.get(k, []))} cases on {sorted(families)}")
        assert families, k
        assert "rotations" in families, k
        assert families & set(TA.LOOP_FAMILIES), k
    # the loop families do take the counted loop, rotations the 3 x 3 form (tests/test_sr_adj_cases_host.py holds every problem)
    for family in TA.FORM_FAMILIES:
        assert {TA.side(t[2]) for t in TA.problem(TA.FORM_SHAPE, family, TA.FORM_N).tfs} == {TA.FAMILIES[family][1]}
    assert TA.FAMILIES["rotations"][1] == "fixed" and all(TA.FAMILIES[f][1] == "loop" for f in TA.LOOP_FAMILIES)


def test_the_dispatch_restatement():
    f = T.instantiations
    assert [T.log2f(v) for v in (2, 4, 8, 6, 10, 16)] == [1, 2, 3, 0, 0, 0]
    assert [T.factor(s) for s in "ABCDE"] == [4, 2, 8, 6, 4]
    c = T.Case("C", "T2", "l2", "none", "none", "adam", "off", 0)
    assert f(c) == {"sr_affine_flags_kernel", "sr_forward_residual_kernel<true>", "sr_loss_df_kernel", "sr_loss_prior_kernel<false>",
                    "sr_grad_translate_kernel<3>", "sr_backward_gather_kernel<false>"}
    assert f(c, want_loss=False) == f(c) - {"sr_loss_df_kernel", "sr_loss_prior_kernel<false>"}
    # all-one weights alone make it a data-term call; so does the monitor, whatever the loss
    assert "sr_forward_residual_kernel<true,true>" in f(c._replace(weights="shared"))
    m = f(c._replace(shape="D", monitor="trace", tvw="batch"))
    assert m == {"sr_affine_flags_kernel", "sr_mon_init_kernel", "sr_forward_residual_kernel<true,true,true>", "sr_mon_loss_df_kernel",
                 "sr_mon_loss_prior_kernel<true>", "sr_mon_decide_kernel", "sr_grad_translate_kernel<0,true>",
                 "sr_backward_gather_kernel<true,true>"}
    assert "sr_backward_gather_pd_kernel<true,true>" in f(c._replace(rule="pd", monitor="stop", tvw="shared"))
    assert f(c._replace(rule="steps", loss="l1", tvw="batch", shape="B")) == {
        "sr_forward_residual_kernel<false,true>", "sr_backward_adam_kernel<1,true>", "sr_loss_df_dt_kernel", "sr_loss_prior_kernel<true>"}
    assert "sr_forward_residual_kernel<false>" in f(c._replace(rule="steps"))
    with pytest.raises(AssertionError):
        f(c._replace(rule="pd", loss="l1"))
    with pytest.raises(AssertionError):
        f(c._replace(rule="bound", tvw="batch"))


def test_every_option_combination_runs_on_pure_and_on_general_transforms():
    kinds = {}
    for c in T.TABLE:
        kinds.setdefault(T.option_combination(c), set()).add(c.kind)
    print(len(T.TABLE), "cases,", len(kinds), "option combinations")
    for combo, seen in sorted(kinds.items()):
        assert seen == {"T0", "T2"}, (combo, seen)
    assert len(T.TABLE) == len(set(T.TABLE))
    assert {c.shape for c in T.TABLE} == set("ABCDE")
    share = sum(c.shape in "BCD" for c in T.TABLE) / len(T.TABLE)
    assert share >= 0.6, share                                          # A and E only where a narrow or tall plane is the point


# ---- 2. the inputs -------------------------------------------------------------------------------------------------------------------
def test_transform_sets_keep_their_bounds_and_their_out_of_frame_copy():
    for shape, kind in sorted({(c.shape, c.kind) for c in T.TABLE}):
        p = T.problem(shape, kind)
        assert (p.n, p.b) == (T.N_COPIES, T.BATCH) and p.n > T.OUT_OF_FRAME
        assert not np.array_equal(p.rot[0], p.rot[1]) and not np.array_equal(p.tr[0], p.tr[1])      # one set per image
        for t in (p.rot, p.tr):
            lo, hi = T._proj_range(t, p.H, p.W)
            assert 0.5 <= lo and hi <= 1.5, (shape, kind, lo, hi)
        for t in (p.irot, p.itr):
            lo, hi = T._proj_range(t, p.H, p.W)
            assert 0.25 <= lo and hi <= 4.0, (shape, kind, lo, hi)
        corners = np.array([[0, 0], [p.W - 1, 0], [0, p.H - 1], [p.W - 1, p.H - 1]], np.float64)
        for i in range(p.b):
            assert np.array_equal(p.rot[i, 0], [1, 0, 0, 0, 1, 0, 0, 0]) and np.array_equal(p.tr[i, 0], [1, 0, 0, 0, 1, 0, 0, 0])
            t = p.tr[i, T.OUT_OF_FRAME].astype(np.float64)
            den = t[6] * corners[:, 0] + t[7] * corners[:, 1] + 1.0
            xs = (t[0] * corners[:, 0] + t[1] * corners[:, 1] + t[2]) / den
            ys = (t[3] * corners[:, 0] + t[4] * corners[:, 1] + t[5]) / den
            # every tap of every pixel of that copy lies outside the frame, by more than the bilinear footprint
            assert (xs <= -2).all() or (xs >= p.W + 1).all() or (ys <= -2).all() or (ys >= p.H + 1).all(), (shape, kind, i)
            general = (p.tr[i, :, 6:] != 0).any() or (p.tr[i, :, 0] != 1).any() or (p.rot[i, :, 6:] != 0).any()
            assert general == (kind == "T2"), (shape, kind, i)
        if kind == "T2":                       # the three branches the kind is there for, in every image
            for i in range(p.b):
                assert (p.tr[i, :, 0] == np.float32(1.05)).any() and (p.tr[i, :, 6:] != 0).any() and (p.rot[i, :, 6:] != 0).any()
                assert (p.irot[i, :, 6:] != 0).any()                   # the gather's non-affine form


@pytest.mark.parametrize("case", [c for c in T.D_CASES if c.loss == "l2" and c.tvw == "none"], ids=lambda c: "-".join(map(str, c)))
def test_the_stop_cases_stop_image_0_at_2_and_image_1_later(case):
    """The condition the device test of section d puts on its inputs, on the CPU: the oracle's loss along the AMSGrad steps of
    the restated rule.  Image 0 (all-zero copies, start 0) has a loss of exactly 0 and stops at iteration 2; image 1's loss
    falls at each of its first evaluations, so it is still running then."""
    import sr_update_ref as RU
    from oracle import tf_ops
    from test_gpu_sr_wtv import _adam_alphas
    p, y = T.problem(case), T.stop_copies(case)
    lam, iters, tol = (1.0, 0.3, 0.7, 0.05), 4, 1e-6
    sr = p.oracle(lam)
    opt, flag, c0, c1, c2, _ = RU.RULES["amsgrad"]
    alphas = _adam_alphas(iters, T.BATCH, lr=1e-2)
    alphas[:, 1] *= np.float32(1.25)
    losses = np.zeros((iters, T.BATCH))
    for i in range(T.BATCH):
        smp = torch.from_numpy(y[i][..., None])
        x = tf_ops.resize_bilinear(smp[0:1], (p.H, p.W)).numpy()[:, :, :, 0]
        m, v, vhat = (np.zeros_like(x) for _ in range(3))
        for it in range(iters):
            loss, g = sr.loss_and_grad_tf(torch.from_numpy(x[..., None]), smp, p.rot[i], p.tr[i], p.irot[i], p.itr[i])
            losses[it, i] = float(loss)
            x, m, v, vhat = RU.step(opt, flag, c0, c1, c2, x, g.numpy()[..., 0], m, v, vhat, alphas[it, i:i + 1])
    print(case, losses.T.tolist())
    assert not losses[:, 0].any()
    assert (np.diff(losses[:, 1]) < -tol * losses[:-1, 1]).all()
    done = M.stop_iterations(losses, 1, tol, 2, 0)
    assert done[0] == 2 < done[1]


# ---- 3. the neutral values -------------------------------------------------------------------------------------------------------
def test_a_wide_huber_with_unit_weights_is_the_residual_bit_for_bit():
    rng = np.random.default_rng(1)
    r = rng.standard_normal((2, 5, 6, 10)).astype(np.float32)
    r.reshape(-1)[:6] = [0.0, -0.0, 1e-45, -1e-45, np.float32(1e38), np.float32(-1e38)]
    big = float(np.abs(r).max())
    ones = np.ones_like(r)
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    for delta in (big, 2.0 * big):
        for w in (None, ones, ones[0]):
            q = RD.weighted_psi(r, "huber", delta, w)
            assert q.dtype == np.float32 and np.array_equal(bits(q), bits(r)), (delta, w is None)
    assert not np.array_equal(RD.weighted_psi(r, "huber", 0.5 * big), r)                 # and a narrower one is not
    assert np.array_equal(M.rho32(r[np.abs(r) < 1e3], "huber", 1e3, None), M.rho32(r[np.abs(r) < 1e3], "l2"))


@pytest.mark.parametrize("shape,kind", [("D", "T2"), ("B", "T0")])
def test_unit_edge_weights_are_the_plain_tv_gradient(shape, kind):
    p = T.problem(shape, kind)
    lam = (1.0, 0.3, 0.7, 0.05)
    ones = np.ones((p.H, p.W), np.float32)
    kw = dict(num_aug=p.n, feature_size=(p.h, p.w), output_size=(p.H, p.W))
    x = p.target(0).clone()
    x[0, 3:6, 4:9, 0] = 0.5                                                              # flat patches: sign(0) on both sides
    args = (x, p.samples(0), p.rot[0], p.tr[0], p.irot[0], p.itr[0])
    _, g_plain = o_sr.Superresolution(*lam, **kw).loss_and_grad_tf(*args)
    _, g_unit = RW.WeightedSuperresolution(*lam, wy=ones, wx=ones, **kw).loss_and_grad_tf(*args)
    assert torch.equal(g_plain, g_unit)
    assert np.array_equal(M.tv_summands(x[0, :, :, 0].numpy(), ones, ones), M.tv_summands(x[0, :, :, 0].numpy()))
    # and in the primal-dual statements: unit weights are the unweighted box
    sr = SimpleNamespace(lambda_tv=0.3, lambda_L2=0.7, lambda_L1=0.05)
    rng = np.random.default_rng(2)
    xs, g = x[0, :, :, 0].numpy(), rng.standard_normal((p.H, p.W)).astype(np.float32)
    py, px = (0.3 * rng.uniform(-1, 1, (p.H, p.W)).astype(np.float32) for _ in range(2))
    for a, b in zip(P.pd_update(sr, xs, py, px, g, 0.2), P.pd_update(sr, xs, py, px, g, 0.2, wy=ones, wx=ones)):
        assert np.array_equal(a, b)


def test_a_monitor_with_patience_0_never_stops():
    rng = np.random.default_rng(3)
    flat, rising, noisy = np.zeros(12), np.arange(12.0), rng.random(12)
    losses = np.stack([flat, rising, noisy, np.full(12, np.nan), np.full(12, np.inf)], axis=1)
    for every in (1, 3):
        assert np.array_equal(M.stop_iterations(losses, every, 0.0, 0, 0), np.full(5, 12 * every))
        assert np.array_equal(M.stop_iterations(losses, every, 0.0, 0, 0, num_iter=7), np.full(5, 7))
    # ... while patience 2 stops a loss that is 0 from the start at its second stalled evaluation, whatever the tolerance
    for tol in (0.0, 1e-3, 0.5):
        assert M.stop_iterations(flat, 1, tol, 2, 0) == 2
