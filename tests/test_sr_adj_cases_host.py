"""The transform families of tests/sr_adj_cases.py without a device: on every family and shape the restatement
tests/sr_adj_ref.py stays the dense transpose of the oracle's forward operator within tests/test_sr_adj_host.transpose_bound, each
family lies on the side of 1.46875, of 8 and of 16384 it is there for, the properties the device test leans on (the window's
extent and a copy that adds nothing change no value) hold on the restatement, and `instantiations` is the exact dispatch."""
import numpy as np
import pytest

from oracle import tf_ops
from test_sr_adj_host import dense_forward, transpose_bound

import sr_adj_cases as T
import sr_adj_ref as A

N = 5


def _tfs_id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


# ---- 1. the reference on the new families ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", T.SHAPES, ids=_tfs_id)
@pytest.mark.parametrize("family", list(T.FAMILIES))
def test_the_restatement_is_the_dense_transpose_on_every_family(family, shape):
    p = T.problem(shape, family, N)
    H, W, h, w = shape
    _, want_side, want_exact = T.FAMILIES[family]
    for i in range(1):                                          # the dense operator is the cost: one image per case
        tfs, r = p.tfs[i], p.resid[i]
        assert A.exact_applies(tfs[0], tfs[1], tfs[2]) == int(want_exact), (family, i)
        assert T.side(tfs[2]) == want_side, (family, i, T.halves(tfs[2]).max())
        got = A.data_grad_from_resid(r, tfs, (H, W), 1.0, "exact").reshape(-1).astype(np.float64)
        if not want_exact:                                      # the registered statements: what the library falls back to
            assert np.array_equal(got, A.data_grad_from_resid(r, tfs, (H, W), 1.0, "registered").reshape(-1))
            continue
        Amat = dense_forward(tfs, (H, W), (h, w))
        want = 2.0 * (Amat.T @ r.reshape(-1).astype(np.float64))
        used = float((np.abs(got - want) / transpose_bound(Amat, r, (H, W), N)).max())
        print(f"{family} {H}x{W} image {i}: halves {T.halves(tfs[2]).min():.4f} .. {T.halves(tfs[2]).max():.4f}; exact uses at most "
              f"{used:.4f} of the bound")
        assert used <= 1.0 and got.any()
        assert not np.array_equal(got, A.data_grad_from_resid(r, tfs, (H, W), 1.0, "registered").reshape(-1))


# ---- 2. the families -----------------------------------------------------------------------------------------------------------------
def test_unit_scales_are_the_oracles_rotations_bit_for_bit():
    rng = np.random.default_rng(1)
    for H, W in ((12, 20), (8, 8), (8, 72)):
        angles = rng.uniform(-1.6, 1.6, 7).astype(np.float32)
        assert np.array_equal(T.affine_rotations(angles, 1.0, 1.0, 0.0, (H, W)), tf_ops.angles_to_projective_transforms(angles, H, W))
    # the map is R(angle) @ [[sx, shear], [0, sy]] about the centre: the centre is a fixed point, the columns are R's, scaled
    t = T.affine_rotations([0.3], 0.5, 1.25, 0.2, (9, 13))[0].astype(np.float64)
    c, s = np.cos(0.3), np.sin(0.3)
    np.testing.assert_allclose([t[0], t[1], t[3], t[4]], [0.5 * c, 0.2 * c - 1.25 * s, 0.5 * s, 0.2 * s + 1.25 * c], rtol=1e-6)
    np.testing.assert_allclose([t[0] * 6 + t[1] * 4 + t[2], t[3] * 6 + t[4] * 4 + t[5]], [6.0, 4.0], atol=1e-5)


@pytest.mark.parametrize("n", T.COPIES)
def test_every_family_lies_on_its_side_of_the_three_thresholds(n):
    for shape in T.SHAPES:
        for family, (k, want_side, want_exact) in T.FAMILIES.items():
            p = T.problem(shape, family, n)
            assert 2 <= p.b <= 4
            for i, (rot, tr, irot, itr) in enumerate(p.tfs):
                hv = T.halves(irot)
                assert T.side(irot) == want_side, (family, shape, n, i, float(hv.max()))
                assert A.exact_applies(rot, tr, irot) == int(want_exact), (family, shape, n, i)
                assert (irot[:, 6:] == 0).all() and (rot[:, 6:] == 0).all()
                assert np.array_equal(tr[:, [0, 1, 3, 4, 6, 7]], np.tile(np.float32([1, 0, 0, 1, 0, 0]), (n, 1)))      # pure
                shifts = -tr[:, [2, 5]]
                assert (np.abs(shifts) <= np.float32([0.4 * p.W + 0.5, 0.4 * p.H + 0.5])).all() and (shifts[n - 1] == np.round(shifts[n - 1])).all()
                far = (np.abs(irot[:, [2, 5]]) > A.MAX_SHIFT).any()
                assert far == (family == "far_shift") and (family != "far_shift" or abs(irot[min(1, n - 1), 2]) > A.MAX_SHIFT)
            if n > 1:
                assert not np.array_equal(p.tfs[0][0], p.tfs[1][0])                       # one transform set per image
    top = lambda family: float(max(T.halves(t[2]).max() for t in T.problem(T.SHAPES[0], family, n).tfs))
    # the pairs around 1.46875 and around 8 sit within 1e-3 and 0.2 of them, on either side
    assert 1.4677 < top("just_fixed") <= T.FIXED_HALF < top("just_loop") < 1.4699
    assert 7.8 < top("near_wide") <= A.MAX_HALF < top("too_wide") < 8.1
    assert top("rotations") <= 1.43 and top("shrink") < 1.0 and 2.0 <= top("zoom2") < 2.86 and 5.0 <= top("zoom5") < 7.1
    for family, axis in (("wide_x", 0), ("wide_y", 1)):                                  # one axis alone sends the image to the loop
        hv = np.concatenate([T.halves(t[2]) for t in T.problem(T.SHAPES[0], family, n).tfs])
        assert (hv[:, axis] > 2.5).all() and (hv[:, 1 - axis] < 1.2).all(), family
    if n >= 5:
        hv = np.concatenate([T.halves(t[2]) for t in T.problem(T.SHAPES[0], "aniso_shear", n).tfs])
        assert (hv[:, 0] > 2 * hv[:, 1]).any() and (hv[:, 1] > 2 * hv[:, 0]).any()        # narrow on one axis, wide on the other
        assert hv.max() > 5.0


# ---- 3. what the device test leans on ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["rotations", "just_fixed", "zoom2", "zoom5", "aniso_shear"])
def test_the_windows_extent_changes_no_value(family):
    for shape in (T.SHAPES[0], T.SHAPES[2]):
        p = T.problem(shape, family, N)
        rot, tr, irot, itr = p.tfs[0]
        want = A.data_grad_from_resid(p.resid[0], p.tfs[0], shape[:2], 1.0, "exact")
        assert want.any()
        for moved in T.perturbed_inverses(irot):
            assert not np.array_equal(moved, irot) and A.exact_applies(rot, tr, moved) == 1
            assert np.array_equal(A.data_grad_from_resid(p.resid[0], (rot, tr, moved, itr), shape[:2], 1.0, "exact"), want)


def test_a_copy_with_a_zero_residual_changes_no_value():
    for shape in (T.SHAPES[0], T.SHAPES[2]):
        p = T.problem(shape, "rotations", N)
        for i in range(p.b):
            tfs, resid = T.with_zero_copy(p, i)
            assert len(resid) == N + 1 and T.side(p.tfs[i][2]) == "fixed" and T.side(tfs[2]) == "loop"
            assert A.exact_applies(tfs[0], tfs[1], tfs[2]) == 1
            want = A.data_grad_from_resid(p.resid[i], p.tfs[i], shape[:2], 1.0, "exact")
            assert np.array_equal(A.data_grad_from_resid(resid, tfs, shape[:2], 1.0, "exact"), want)        # a zero's sign may differ


# ---- 4. the dispatch -----------------------------------------------------------------------------------------------------------------
def test_the_exact_dispatch_restatement():
    f = T.instantiations
    assert [T.factor(s) for s in T.SHAPES] == [4, 6, 2, 8, 4]
    c = T.Case(T.SHAPES[0], "zoom2", "grad", False, "off", 0, 5)
    assert f(c) == {"sr_adjoint_flags_kernel", "sr_grad_translate_kernel<2>", "sr_backward_gather_adj_kernel<false,false>"}
    assert f(c._replace(rule="step", wtv=True, shape=T.SHAPES[1])) == {
        "sr_adjoint_flags_kernel", "sr_grad_translate_kernel<0>", "sr_backward_gather_adj_kernel<true,false>"}
    assert f(c._replace(rule="adam", wtv=True)) == {
        "sr_adjoint_flags_kernel", "sr_forward_residual_kernel<true,true>", "sr_grad_translate_kernel<2>",
        "sr_backward_gather_adj_kernel<true,false>"}
    assert f(c._replace(rule="adam"), want_loss=True) - f(c._replace(rule="adam")) == {"sr_loss_df_dt_kernel", "sr_loss_prior_kernel<false>"}
    assert f(c._replace(rule="pd", wtv=True, monitor="stop", shape=T.SHAPES[3])) == {
        "sr_adjoint_flags_kernel", "sr_mon_init_kernel", "sr_forward_residual_kernel<true,true,true>", "sr_mon_loss_df_kernel",
        "sr_mon_loss_prior_kernel<true>", "sr_mon_decide_kernel", "sr_grad_translate_kernel<3,true>",
        "sr_backward_gather_pd_adj_kernel<true,true>"}
    assert "sr_backward_gather_adj_kernel<false,true>" in f(c._replace(rule="sgd", monitor="trace"))
    assert "sr_backward_gather_pd_adj_kernel<false,false>" in f(c._replace(rule="pd", shape=T.SHAPES[2]))
    assert f(c._replace(rule="bound")) == {
        "sr_adjoint_flags_kernel", "sr_bound_next_v_kernel", "sr_forward_residual_kernel<true,true>", "sr_grad_translate_kernel<2>",
        "sr_backward_gather_adj_kernel<false,false>", "sr_bound_maxima_kernel", "sr_bound_out_kernel"}
    # no case launches a registered gather kernel, and a family that falls back runs the same kernels
    for case in T.TABLE:
        assert not any(k.startswith(("sr_backward_gather_kernel", "sr_backward_gather_pd_kernel", "sr_affine_flags")) for k in f(case))
    assert f(c._replace(family="too_wide")) == f(c)
    for bad in (c._replace(rule="grad", monitor="trace"), c._replace(rule="bound", wtv=True), c._replace(rule="bound", monitor="stop"),
                c._replace(family="rotation"), c._replace(shape=(8, 12, 4, 6))):
        with pytest.raises(AssertionError):
            f(bad)


def test_the_table_has_the_shapes_copies_and_chunks_the_kernels_branch_on():
    assert len(T.TABLE) == len(set(T.TABLE))
    grads = [c for c in T.TABLE if c.rule == "grad"]
    assert {(c.shape, c.family, c.n, c.chunk) for c in grads} == {(s, f, n, k) for s in T.SHAPES for f in T.FAMILIES for n in T.COPIES
                                                                  for k in T.CHUNKS}
    assert set(T.COPIES) == {1, 5, 6, 9} and set(T.CHUNKS) == {0, 3, 1}
    assert any(W > 64 and W % 64 for _, W, _, _ in T.SHAPES)                            # a second, ragged gather block in x
    assert {T.log2f(T.factor(s)) for s in T.SHAPES} == {0, 1, 2, 3}
    assert set(T.LOOP_FAMILIES) == {"just_loop", "zoom2", "zoom5", "aniso_shear", "wide_x", "wide_y", "near_wide"}
    assert {T.batch_of(s, n) for s in T.SHAPES for n in T.COPIES} == {2, 3, 4}
