"""Host-only evidence for tests/base_kernel_cases.py: the launch geometry it restates is the sources' own, its table reaches
every path it names, its references agree with oracle/, its data is not vacuous, a correct numpy producer passes every check_*
function and each deliberately wrong one fails at least one case of its entry point.  The GPU tests run the same table through
the same check_* functions."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import base_kernel_cases as bk  # noqa: E402
from oracle import augment as o_aug, sr as o_sr, tf_ops  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deeplabv3plus-augmented-superresolution_amd", "csrc")
SMALL = 1 << 20              # mutations and oracle comparisons run on the cases below this many elements


@pytest.fixture(scope="module", autouse=True)
def _free():
    yield
    bk.free_big()


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(pattern, text):
    m = re.findall(pattern, text)
    assert len(m) == 1, (pattern, m)
    return m[0]


# ---- the restated launch geometry is the sources' -----------------------------------------------------------------------------
def test_geometry_constants_match_the_sources():
    r, w, h = _src("reduce.hip"), _src("warp.hip"), _src("asr_common.h")
    assert int(_one(r"per_wg = asr_cdiv\(per_segment, (\d+)\)", r)) == bk.MINMAX_SPLIT
    a, b, c = _one(r"cap = segments >= (\d+) \? 1 : (\d+) / segments", r) + (_one(r"minmax_kernel, dim3\(\(unsigned\)per_wg, "
                                                                               r"\(unsigned\)segments\), dim3\((\d+)\)", r),)
    assert int(a) == int(b) == bk.MINMAX_WG_CAP and int(c) == bk.MINMAX_BLOCK
    assert set(re.findall(r"blockIdx\.x \* (\d+) \+ threadIdx\.x; i < per_seg; i \+= \(int64_t\)gridDim\.x \* (\d+)\) \{\n        const "
                          r"float v = p\[i\]", r)) == {(str(bk.MINMAX_BLOCK),) * 2}
    g = _one(r"int stream_grid\(int64_t n\) \{\n    int64_t g = asr_cdiv\(n, (\d+)\);\n    return \(int\)\(g < (\d+) \? "
             r"\(g > 0 \? g : 1\) : (\d+)\);", r)
    assert [int(v) for v in g] == [bk.BLOCK, bk.STREAM_CAP, bk.STREAM_CAP]
    assert [int(v) for v in _one(r"iou_counts_kernel, dim3\(stream_grid\(per_segment\) > (\d+) \? (\d+) :", r)] == [bk.IOU_CAP] * 2
    assert [int(v) for v in _one(r"asr_class_counts_i32[^}]*?stream_grid\(per_segment\) > (\d+) \? (\d+) :", r)] == [bk.COUNTS_CAP] * 2
    assert [int(v) for v in _one(r"asr_iou_counts_classes_i32[^}]*?stream_grid\(pixels\) > (\d+) \? (\d+) :", r)] == \
        [bk.IOU_CLASSES_CAP] * 2
    assert int(_one(r"constexpr int kMaxStageClasses = (\d+);", r)) == bk.MAX_STAGE_CLASSES
    assert int(_one(r"constexpr int kMaxIouMasks = (\d+);", r)) == bk.MAX_IOU_MASKS
    assert len(re.findall(r"classes <= kMaxStageClasses", r)) == 3          # argmax, OPM, class_activation
    assert int(_one(r"constexpr int kThreads = (\d+);", w)) == bk.BLOCK
    x, y = _one(r"const int64_t cap = (\d+) \* (\d+);", w)
    assert int(x) * int(y) == bk.WARP_CAP
    assert [int(v) for v in _one(r"ASR_UNSUPPORTED\(n > (\d+) \|\| h > (\d+),", w)] == [bk.MAX_GRID_YZ] * 2
    assert "case 1:" in w and "case 3:" in w and len(re.findall(r"case \d+: hipLaunchKernelGGL\(augment_copies_kernel", w)) == 2
    assert re.search(r"fminf\(fmaxf\(f, -1\.0e9f\), 1\.0e9f\)", h)


# ---- reach --------------------------------------------------------------------------------------------------------------------
def test_minmax_cases_reach_every_regime():
    cases = bk.CASES["minmax"]
    grids = {(c.per, c.segments): bk.minmax_grid(c.per, c.segments) for c in cases}
    assert {p for (p, s) in grids} >= {1, 63, 64, 65, 1023, 1024, 1025, 16384, 16385, 3 * 16384 + 5}
    assert grids[(16384, 1)] == 1 and grids[(16385, 1)] == 2 and grids[(3 * 16384 + 5, 3)] == 4
    assert grids[(5 * 16384 + 1, 7)] == 6 == bk.cdiv(5 * 16384 + 1, bk.MINMAX_SPLIT)                         # uncapped
    assert grids[(4 * 16384 + 5, 300)] == 3 < bk.cdiv(4 * 16384 + 5, bk.MINMAX_SPLIT) == 5                   # capped: a second trip
    assert bk.cdiv(4 * 16384 + 5, 3 * bk.MINMAX_BLOCK) > bk.MINMAX_SPLIT // bk.MINMAX_BLOCK
    assert grids[(16385, 1024)] == 1 and bk.cdiv(16385, bk.MINMAX_BLOCK) > 16                                # one workgroup, on past 16 K
    assert max(c.segments * c.per * 4 for c in cases) < 200e6
    # a negative extreme, +-FLT_MAX, an infinity and a zero pair in a workgroup other than the first, first and last element of its share
    seen = set()
    for c in cases:
        g = bk.minmax_grid(c.per, c.segments)
        if g == 1 or not c.position.startswith("wg"):
            continue
        imin, imax = bk.minmax_position_indices(c.per, c.segments)[c.position]
        b = int(c.position[2:].split("_")[0])
        share = bk.minmax_share(c.per, g, b)
        assert {imin, imax} == {int(share[0]), int(share[-1])}, c.id
        if b > 0:
            seen |= {(k, c.position.split("_")[1]) for k in bk.minmax_kinds(c)}
    assert seen == {(k, e) for k in bk.MINMAX_KINDS for e in ("first", "last")}
    for key, g in grids.items():                                            # every workgroup of every split shape has its two cases
        if g > 1:
            names = set(bk.minmax_position_indices(*key))
            assert {"e0", "last"} <= names and len(names) >= 2 * g, key


def test_minmax_data_is_what_it_claims():
    for c in bk.CASES["minmax"]:
        if c.segments * c.per > SMALL:
            continue
        x, planted = bk.build_minmax(c)
        ref = bk.minmax_ref(x)
        assert bk.same_bits(ref[:, 0] + 0, planted[:, 0] + 0) and bk.same_bits(ref[:, 1] + 0, planted[:, 1] + 0), c.id
        for s, k in enumerate(bk.minmax_kinds(c)):
            if c.per > 1 and k == "neg":
                assert (x[s] < 0).all()
            if c.per > 1 and k == "pos":
                assert (x[s] > 0).all()
            if c.per > 2 and k == "mixed":
                assert (x[s] < 0).any() and (x[s] > 0).any()
            if c.per > 2 and k == "zeros":
                assert (x[s] == 0).all() and np.signbit(x[s]).any() and not np.signbit(x[s]).all()
            if s:                                                           # a neighbour's result is another result
                assert ref[s, 0] != ref[s - 1, 0] or k == "zeros" or c.per == 1, c.id
                assert (ref[s] != ref[s - 1]).any(), c.id
                a, b = bk.minmax_kinds(c)[s - 1], k
                if {a, b} <= {"neg", "mixed", "pos"}:                       # finite kinds: disjoint ranges
                    assert ref[s, 0] > ref[s - 1, 1] or ref[s, 1] < ref[s - 1, 0], c.id


def _trips(entry_cases, n_of, cap):
    return {c.id: bk.second_pass_tiles(n_of(c), bk.capped_grid(n_of(c), cap)) for c in entry_cases}


def test_every_capped_grid_has_a_second_trip_with_a_full_and_a_ragged_tile():
    for entry in ("argmax", "opm_argmax", "slice_max", "activation"):
        t = _trips(bk.CASES[entry], lambda c: c.pixels, bk.STREAM_CAP)
        for classes in bk.BIG_CLASSES:                                      # staged (21) and straight from global memory (33)
            assert t[f"c{classes}_p{bk.BIG_PIXELS}"] == (1, 1), entry
        assert bk.staged(21) and bk.staged(32) and not bk.staged(33)
        shapes = {(c.classes, c.pixels) for c in bk.CASES[entry]}
        want = {(cl, p) for cl in bk.LOGIT_CLASSES for p in bk.LOGIT_PIXELS if cl >= (2 if entry == "slice_max" else 1)}
        assert shapes >= want and {(21, bk.BIG_PIXELS), (33, bk.BIG_PIXELS)} <= shapes
    assert max(t for t in _trips(bk.CASES["threshold"], lambda c: c.per, bk.STREAM_CAP).values()) == (1, 1)
    assert {c.per for c in bk.CASES["threshold"]} == {257, 16385, 2048 * 256 + 300}
    for entry in ("iou", "iou_shared"):
        t = _trips(bk.CASES[entry], lambda c: c.per, bk.IOU_CAP)
        assert {t[c.id] for c in bk.CASES[entry] if c.per == 16385} == {(0, 1)}
        assert {t[c.id] for c in bk.CASES[entry] if c.per == 64 * 256 * 3 + 77} == {(128, 1)}
        assert {t[c.id] for c in bk.CASES[entry] if c.per <= 16384} == {(0, 0)}
    t = _trips(bk.CASES["class_counts"], lambda c: c.per, bk.COUNTS_CAP)
    assert t["p16385_s3_uniform"] == (0, 1) and t[f"p{64 * 256 * 2 + 9}_s3_outside"] == (64, 1)
    assert set(_trips(bk.CASES["iou_classes"], lambda c: c.pixels, bk.IOU_CLASSES_CAP).values()) == {(1, 1)}
    stride = bk.case_by_id("warp", "stride_5x512x512")
    total = stride.n * stride.out_hw[0] * stride.out_hw[1]
    assert bk.warp_grid(total) == bk.WARP_CAP and total > bk.WARP_CAP * bk.BLOCK and total % bk.BLOCK == 0
    assert all(bk.warp_grid(c.n * c.out_hw[0] * c.out_hw[1]) < bk.WARP_CAP for c in bk.CASES["warp"] if c is not stride)
    assert any(bk.minmax_grid(c.per, c.segments) > 1 for c in bk.CASES["normalize"])
    assert any(bk.minmax_grid(c.per_copy * c.classes, c.copies) > 1 for c in bk.CASES["opm_slice"])
    assert {(c.M, c.K) for c in bk.CASES["iou_classes"]} == {(1, 1), (1, 21), (8, 1), (8, 21)} and bk.MAX_IOU_MASKS == 8
    assert any(c.shape[2] > bk.BLOCK for c in bk.CASES["augment"]) and any(c.shape[2] == bk.BLOCK for c in bk.CASES["augment"])
    assert {s[3] for s in bk.AUGMENT_REFUSALS.values()} >= {2, 4} and bk.AUGMENT_REFUSALS["n65536"][0] > bk.MAX_GRID_YZ
    for c in bk.CASES["minmax"] + bk.CASES["threshold"] + bk.CASES["iou"] + bk.CASES["class_counts"]:
        assert c.segments <= bk.MAX_GRID_YZ


def test_logit_rows_win_tie_and_sit_in_the_second_trip():
    first = bk.STREAM_CAP * bk.BLOCK
    for entry_case in bk.CASES["argmax"]:
        x = bk.build_logits(entry_case)
        classes, pixels = entry_case.classes, entry_case.pixels
        arg, rowmax = bk.first_argmax(x), x.max(axis=1)
        at_max = x == rowmax[:, None]
        tie = at_max.sum(axis=1) >= 2
        if pixels >= 255:
            for c in range(classes):
                assert (arg == c).mean() >= 0.01, (entry_case.id, c)
                assert classes == 1 or (at_max[:, c] & tie).any(), (entry_case.id, c)
            assert np.isneginf(x).all(axis=1).any() and np.isposinf(x).any(axis=1).any()
            assert classes == 1 or (bk.argmax_ref(x) != bk.argmax_ref(x, last=True)).any()
            z = x == 0
            assert z.any() and np.signbit(x[z]).any() and (classes == 1 or not np.signbit(x[z]).all())
        if pixels == bk.BIG_PIXELS:
            sec = slice(first, first + bk.BLOCK)
            for c in range(classes):
                assert ((arg[sec] == c) & ~tie[sec]).any() and (at_max[sec, c] & tie[sec]).any(), (entry_case.id, c)
            assert tie[-1] and arg[-1] == classes - 2                       # the one-row tile: a tie, first maximum wins
            assert np.isinf(x[first:]).any()


def test_threshold_data_is_what_it_claims():
    for c in bk.CASES["threshold"]:
        img, mask, fac, value = bk.build_threshold(c)
        ref = bk.threshold_ref(img, mask, fac, value)
        for s in range(c.segments):
            share = (ref[s] == value).mean()
            assert (share == 0) if c.kind == "one" else (0 < share < 1), (c.id, s, share)
            if mask is not None:
                eq = img[s] == mask[s]
                assert eq.sum() > 5 and (ref[s][eq] == value).all()
                assert (eq & (np.signbit(img[s]) != np.signbit(mask[s]))).any()
                continue
            mx = img[s].max()
            th = np.float32(mx * np.float32(fac))
            assert ((img[s] == th) & (ref[s] == 0)).sum() >= 3, (c.id, "pixels at the threshold, off")
            assert (mx < 0) == (c.kind == "negmax")
            if c.kind == "f32prod":                                         # a pixel between the float64 and the float32 product
                exact = np.float64(mx) * np.float64(fac)
                assert float(th) > exact and ((img[s].astype(np.float64) > exact) & (img[s] <= th)).any(), c.id
            if c.kind == "zero":
                assert th == 0 and np.signbit(img[s][img[s] == 0]).any() and not np.signbit(img[s][img[s] == 0]).all()
            if s:
                assert img[s].max() != img[s - 1].max()


def test_count_data_is_what_it_claims():
    for c in bk.CASES["iou"] + bk.CASES["iou_shared"]:
        truth, pred = bk.build_iou(c)
        ref = bk.iou_case_ref(c, truth, pred)
        assert (ref > 0).all(), c.id
        assert set(np.unique(truth)) == set(bk.IOU_TRUTH_LABELS) or c.per < 1000
        if c.class_id == 0:
            assert np.array_equal(ref[:, 0], ref[:, 2]) and np.array_equal(ref[:, 1], ref[:, 3])
        assert c.class_id == 0 or len({tuple(r) for r in ref}) == c.segments          # (class 0: every mask is 0 but for the strays)
    for c in bk.CASES["iou_classes"]:
        ids, truth, preds = bk.build_iou_classes(c)
        assert (bk.iou_classes_ref(c, ids, truth, preds) > 0).all(), c.id
        assert preds.nbytes < 200e6
    for c in bk.CASES["class_counts"]:
        truth, pred, (keep_t, keep_p) = bk.build_class_counts(c)
        ref = bk.class_counts_ref(truth, pred)
        assert ref.sum() > 0 or c.per < 10
        if c.kind == "outside" and c.per >= 255:
            assert set(bk.OUT_OF_RANGE_LABELS) <= set(truth.reshape(-1).tolist()) and not keep_t.all() and not keep_p.all()
            assert ((truth == pred) & ~keep_t).any()
            for s in range(c.segments):                                     # the labels outside 0..255 change nothing
                assert np.array_equal(ref[s, 0], np.bincount(truth[s][keep_t[s]], minlength=256))
                assert np.array_equal(ref[s, 1], np.bincount(pred[s][keep_p[s]], minlength=256))
                both = keep_t[s] & keep_p[s] & (truth[s] == pred[s])
                assert np.array_equal(ref[s, 2], np.bincount(truth[s][both], minlength=256))
        if c.kind == "single":
            assert ref[0, 0].max() == c.per == ref[0, 2].max()
        if c.segments > 1 and c.kind != "outside":
            for s in range(c.segments):                                     # a segment's labels are absent from its neighbours' counts
                others = np.delete(ref, s, axis=0).sum(axis=(0, 1))
                assert not others[ref[s, 0] > 0].any(), c.id
    assert bk.case_by_id("class_counts", "p40000_s1_single").per == 40000


def test_warp_cases_reach_the_named_coordinates():
    h, w = bk.WARP_IN

    def coords(tf, out_hw):
        xs, ys = np.meshgrid(np.arange(out_hw[1], dtype=np.float32), np.arange(out_hw[0], dtype=np.float32))
        with np.errstate(all="ignore"):
            proj = tf[6] * xs + tf[7] * ys + np.float32(1)
            return (tf[0] * xs + tf[1] * ys + tf[2]) / proj, (tf[3] * xs + tf[4] * ys + tf[5]) / proj, proj

    T = bk.WARP_TRANSFORMS
    ix, iy, proj = coords(T["proj_zero"], (h, w))
    assert (proj[:, 8] == 0).all() and np.isinf(ix[:, 8]).all() and np.isinf(iy[:, 8]).all() and (proj[:, 9:] < 0).all()
    assert not np.isnan(ix).any() and not np.isnan(iy).any()               # non-zero numerators: no 0 / 0
    ix, iy, proj = coords(T["proj_neg"], (h, w))
    inside = (ix > 0) & (ix < w - 1) & (iy > 0) & (iy < h - 1)
    assert (proj < 0).any() and (proj > 0).any() and (inside & (proj < 0)).any()
    for out_hw in bk.WARP_OUTS.values():
        ix, iy, _ = coords(T["far"], out_hw)
        assert np.isfinite(ix).all() and np.isfinite(iy).all() and (np.abs(ix) > 2.0 ** 31).all()       # the clamp of asr_coord_to_int
        ix, iy, _ = coords(T["past_frame"], out_hw)
        assert (ix < -1).all()
    ix, iy, _ = coords(T["frac_neg"], (h, w))
    assert ((ix > -1) & (ix < 0) & (iy > -1) & (iy < 0)).any() and (np.trunc(ix) != np.floor(ix)).any()
    img = bk.warp_image((h, w, 3), 1)
    _, taps = bk.warp_np(img, T["rot0.3"], 1, taps=True)
    assert ((taps >= 1) & (taps <= 3)).mean() >= 0.05                       # one to three taps out of frame
    N = bk.NEAREST_TRANSFORMS
    for name in ("shift+0.5", "shift-0.5", "shift1.5"):
        ix, iy, _ = coords(N[name], (h, w))
        assert (ix % 1 == 0.5).all()                                        # exact halves
    ix, _, _ = coords(N["shift-0.5"], (h, w))
    assert ix.max() == w - 0.5                                              # rounds to w: out of frame
    ix, iy, _ = coords(N["neg_zero"], (h, w))
    assert ((ix > -0.5) & (ix < 0)).any() and ((iy > -0.5) & (iy < 0)).any()
    assert {c.c for c in bk.CASES["warp"]} == set(bk.WARP_CHANNELS) and {c.combo for c in bk.CASES["warp"]} == set(bk.WARP_COMBOS)
    assert {c.out_hw for c in bk.CASES["warp"]} >= set(bk.WARP_OUTS.values())
    assert {c.shape for c in bk.CASES["augment"]} == set(bk.AUGMENT_SHAPES)
    for shape in bk.AUGMENT_SHAPES:                                         # every pool entry meets every shape; copy 0 identity once
        cs = [c for c in bk.CASES["augment"] if c.shape == shape]
        assert {(c.start + i) % len(bk.AUGMENT_POOL) for c in cs for i in range(shape[0])} == set(range(len(bk.AUGMENT_POOL)))
        assert any(c.start == 0 for c in cs)


# ---- the references agree with oracle/ ------------------------------------------------------------------------------------------
def test_normalize_and_slice_references_agree_with_the_oracle():
    for c in bk.CASES["normalize"]:
        x = bk.build_normalize(c)
        ref = bk.normalize_segments_ref(c, x)
        for s in range(c.segments):
            o = o_sr.min_max_normalization(x[s], new_min=c.new_min, new_max=c.new_max)
            assert o.dtype == np.float32 and bk.same_bits(o, ref[s]), c.id
        spans = [float(s.max() - s.min()) for s in x]
        if c.data == "const_mid":
            assert spans[1] == 0 and spans[0] > 0 and spans[2] > 1e3 * spans[0] and (ref[1] == np.float32(c.new_min)).all()
        else:
            assert x.max() < 0
    for c in bk.CASES["opm_slice"]:
        x = bk.build_opm_slice(c)
        if c.copies > 1:
            assert x[1].max() == x[1].min() and x[2].max() > 1e3 * x[0].max()
        if (c.new_min, c.new_max) != (0.0, 1.0):
            continue
        for cid in c.class_ids:
            cm, _ = o_aug.opm(x[:, :, None, :], cid, "slice")
            assert bk.same_bits(np.stack(cm)[..., 0, 0], bk.opm_slice_ref(c, x, cid)), (c.id, cid)


def test_argmax_references_agree_with_the_oracle():
    for c in bk.CASES["slice_max"] + [k for k in bk.CASES["argmax"] if k.classes == 1]:
        if c.pixels * c.classes > SMALL:
            continue
        x = bk.build_logits(c)
        assert np.array_equal(o_aug.create_mask(x)[..., 0], bk.argmax_ref(x)), c.id
        for cid in c.class_ids:
            cm, _ = o_aug.opm(x[None], cid, "argmax")
            assert bk.same_bits(cm[0][..., 0], bk.opm_argmax_ref(x, cid)), (c.id, cid)
            if c.classes > 1:
                cm, mm = o_aug.opm(x[None], cid, "slice_max")
                cls, mx = bk.slice_max_ref(x, cid)
                assert bk.same_bits(cm[0][..., 0], cls) and np.array_equal(mm[0][..., 0], mx), (c.id, cid)


def test_threshold_and_count_references_agree_with_the_oracle():
    for c in bk.CASES["threshold"]:
        img, mask, fac, value = bk.build_threshold(c)
        ref = bk.threshold_ref(img, mask, fac, value)
        for s in range(c.segments):
            o = o_sr.threshold_image(img[s], value, th_factor=fac, th_mask=None if mask is None else mask[s])
            assert np.array_equal(o, ref[s]), (c.id, s)
    for c in bk.CASES["iou"] + bk.CASES["iou_shared"]:
        truth, pred = bk.build_iou(c)
        ref = bk.iou_case_ref(c, truth, pred)
        for s in range(c.segments):
            o = o_aug.single_class_IOU(truth if c.shared else truth[s], pred[s], c.class_id, c.include_bg)
            assert o == bk.iou_ratio(ref[s], c.include_bg), (c.id, s)
    for c in bk.CASES["class_counts"]:
        if c.kind == "outside":
            continue
        truth, pred, _ = bk.build_class_counts(c)
        ref = bk.class_counts_ref(truth, pred)
        for s in range(c.segments):
            o = o_aug.Mean_IOU(truth[s], pred[s])
            m = bk.mean_iou_of_counts(ref[s])
            assert o == m or (np.isnan(o) and np.isnan(m)), (c.id, s, o, m)


def _oracle_warp(data, nearest):
    src, tf, n, out_hw = data
    img = src if src.ndim == 4 else np.broadcast_to(src, (n,) + src.shape).copy()
    return tf_ops.projective_transform(torch.from_numpy(np.ascontiguousarray(img)), np.ascontiguousarray(tf).reshape(-1, 8),
                                       output_shape=out_hw, interpolation="nearest" if nearest else "bilinear").numpy()


def test_warp_restatement_agrees_with_the_oracle():
    h, w = bk.WARP_IN
    for a in (0.3, np.pi / 2, np.pi, -3.0, 0.4, 0.0):
        assert bk.same_bits(bk.rotation_tf(a, h, w), tf_ops.angles_to_projective_transforms([a], h, w)[0])
    assert bk.same_bits(bk.shift_tf(7.25, -3.5), tf_ops.translations_to_projective_transforms([[7.25, -3.5]])[0])
    for c in bk.CASES["warp"] + bk.CASES["nearest"]:
        data = bk.build_warp(c)
        mine = bk.warp_np(*data, nearest=c.nearest)
        ref = _oracle_warp(data, c.nearest)
        assert np.isfinite(ref).all() and np.array_equal(mine, ref), c.id
        bk.check_warp(c, data, mine, ref=ref)
        if c.tf_name in ("far", "past_frame") and c.combo[1] == "s":
            assert not ref.any(), c.id
        if c.tf_name == "proj_zero" and c.out_hw[1] > 8 and c.combo[1] == "s":
            assert not ref[:, :, 8:].any() and ref[:, :, :8].any(), c.id
    for c in bk.CASES["augment"]:
        image, rot, trans, angles, shifts = bk.build_augment(c)
        n = c.shape[0]
        tiled = torch.from_numpy(np.broadcast_to(image, (n,) + image.shape).copy())
        ref = tf_ops.translate(tf_ops.rotate(tiled, angles), shifts).numpy()
        mine = bk.augment_np(image, rot, trans)
        assert np.array_equal(mine, ref), c.id
        bk.check_augment(c, (image, rot, trans, angles, shifts), mine, ref=ref)


def test_float32_activation_stays_inside_the_bounds():
    worst = 0.0
    for c in bk.CASES["activation"]:
        if c.pixels * c.classes > SMALL:
            continue
        x = bk.build_activation(c)
        for kind in ("softmax", "sigmoid"):
            worst = max(worst, bk.check_activation(c, x, kind, bk.activation_f32(x, kind)))
    assert 0 < worst < 1e-6


# ---- mutations: a correct producer passes, every wrong one is caught -----------------------------------------------------------
def _caught(fn, *args):
    try:
        fn(*args)
    except AssertionError:
        return True
    return False


def _assert_rejected(name, hits):
    assert hits, f"no case rejects the wrong producer '{name}'"


def _minmax_producer(x, segments, mut=None):
    per = x.shape[1]
    g = bk.minmax_grid(per, segments)
    out = np.empty((segments, 2), np.float32)
    out[:, 0], out[:, 1] = np.inf, -np.inf
    for b in range(1 if mut == "first_wg" else g):
        share = bk.minmax_share(per, g, b)
        if mut == "drop_tail":
            share = share[share < per // 1024 * 1024]
        if not len(share):
            continue
        part = x[:, share]
        if mut == "signed_bits":
            mn, mx = part.view(np.int32).min(axis=1).view(np.float32), part.view(np.int32).max(axis=1).view(np.float32)
        else:
            mn, mx = part.min(axis=1), part.max(axis=1)
        out[:, 0], out[:, 1] = np.minimum(out[:, 0], mn), np.maximum(out[:, 1], mx)
    if mut == "seg0":
        out[:] = out[0]
    return out


def test_minmax_mutations():
    small = [c for c in bk.CASES["minmax"] if c.segments * c.per <= SMALL]
    hits = {m: [] for m in ("signed_bits", "drop_tail", "first_wg", "seg0")}
    for c in small:
        x, _ = bk.build_minmax(c)
        bk.check_minmax(c, x, _minmax_producer(x, c.segments))
        for m in hits:
            if _caught(bk.check_minmax, c, x, _minmax_producer(x, c.segments, m)):
                hits[m].append(c.id)
    for m, h in hits.items():
        _assert_rejected(m, h)
    assert any("wg1" in i or "wg3" in i for i in hits["first_wg"]) and any("_s3_" in i for i in hits["seg0"])
    assert any("_p1025_" in "_" + i or i.startswith("p1025_") for i in hits["drop_tail"])


def _rows(x, f, mut=None, width=None):
    """f over the rows of x as a grid of stream_grid workgroups would walk them, with the named mistake"""
    pixels = x.shape[0]
    src = x[:, :32] if mut == "first32" else x
    out = np.array(f(src))
    if mut == "first32" and width:                                          # (activation: the classes past 32 are never written)
        out = np.concatenate([out, np.zeros((pixels, x.shape[1] - out.shape[1]), out.dtype)], axis=1) if out.shape[1] < x.shape[1] else out
    first = bk.stream_grid(pixels) * bk.BLOCK
    if mut == "second_reuse" and pixels > first:
        out[first:] = out[:pixels - first]
    if mut == "ragged_dropped" and pixels % bk.BLOCK:
        out[pixels // bk.BLOCK * bk.BLOCK:] = 0
    return out


def test_argmax_family_mutations():
    muts = ("last_max", "first32", "second_reuse", "ragged_dropped")
    hits = {(e, m): [] for e in ("argmax", "opm_argmax", "slice_max", "activation") for m in muts if (e, m) != ("activation", "last_max")}
    hits[("slice_max", "includes_self")] = []
    for c in bk.CASES["argmax"]:
        x = bk.build_logits(c)
        cid = c.class_ids[-1]
        bk.check_argmax(c, x, _rows(x, bk.argmax_ref))
        bk.check_opm_argmax(c, x, cid, _rows(x, lambda r: bk.opm_argmax_ref(r, cid)))
        for m in muts:
            f = (lambda r: bk.argmax_ref(r, last=True)) if m == "last_max" else bk.argmax_ref
            if _caught(bk.check_argmax, c, x, _rows(x, f, m)):
                hits[("argmax", m)].append(c.id)
            g = lambda r: np.where(f(r) == cid, cid, 0).astype(np.float32)
            if _caught(bk.check_opm_argmax, c, x, cid, _rows(x, g, m)):
                hits[("opm_argmax", m)].append(c.id)
        if c.classes < 2:
            continue
        for cid in c.class_ids:
            def sm(r, last=False, self_too=False):
                keep = [j for j in range(r.shape[1]) if j != cid or self_too]
                return np.stack([r[:, cid] if cid < r.shape[1] else np.zeros(len(r), np.float32), r[:, keep].max(axis=1)], axis=1)
            ok = _rows(x, sm)
            bk.check_slice_max(c, x, cid, ok[:, 0].copy(), ok[:, 1].copy())
            for m in muts + ("includes_self",):
                if m == "last_max":
                    continue
                got = _rows(x, (lambda r: sm(r, self_too=True)) if m == "includes_self" else sm, m)
                if _caught(bk.check_slice_max, c, x, cid, got[:, 0].copy(), got[:, 1].copy()):
                    hits[("slice_max", m)].append(c.id)
    del hits[("slice_max", "last_max")]
    for c in bk.CASES["activation"]:
        x = bk.build_activation(c)
        kind = "softmax"
        bk.check_activation(c, x, kind, _rows(x, lambda r: bk.activation_f32(r, kind)))
        for m in muts[1:]:
            if _caught(bk.check_activation, c, x, kind, _rows(x, lambda r: bk.activation_f32(r, kind), m, width=True)):
                hits[("activation", m)].append(c.id)
    for (e, m), h in hits.items():
        _assert_rejected(f"{e}:{m}", h)
        if m == "second_reuse":
            assert all(str(bk.BIG_PIXELS) in i for i in h)
        if m == "first32":
            assert all(i.startswith(("c33", "c40")) for i in h)


def test_threshold_mutations():
    hits = {m: [] for m in ("ge", "mask_gt", "f64", "seg0")}
    for c in bk.CASES["threshold"]:
        if c.per * c.segments > SMALL:
            continue
        data = bk.build_threshold(c)
        bk.check_threshold(c, data, bk.threshold_ref(*data))
        for m in hits:
            if _caught(bk.check_threshold, c, data, bk.threshold_ref(*data, **{m: True})):
                hits[m].append(c.id)
    for m, h in hits.items():
        _assert_rejected(m, h)
    assert any("f32prod" in i for i in hits["f64"]) and all("mask" in i for i in hits["mask_gt"])


def test_count_mutations():
    hits = {m: [] for m in ("no_remap", "skip255", "drop_tail")}
    for c in bk.CASES["iou"] + bk.CASES["iou_shared"]:
        truth, pred = bk.build_iou(c)
        bk.check_iou(c, (truth, pred), bk.iou_case_ref(c, truth, pred))
        for m in ("no_remap", "skip255"):
            if _caught(bk.check_iou, c, (truth, pred), bk.iou_case_ref(c, truth, pred, **{m: True})):
                hits[m].append(c.id)
        cut = bk.iou_case_ref(c, truth[..., :16384], pred[..., :16384])
        if _caught(bk.check_iou, c, (truth, pred), cut):
            hits["drop_tail"].append(c.id)
    for m, h in hits.items():
        _assert_rejected(m, h)
    assert all(i.endswith("bg1") for i in hits["no_remap"]) and all("p255_" not in i and "p16384_" not in i for i in hits["drop_tail"])
    hits = {m: [] for m in ("and255", "both_outside")}
    for c in bk.CASES["class_counts"]:
        truth, pred, keep = bk.build_class_counts(c)
        bk.check_class_counts(c, (truth, pred, keep), bk.class_counts_ref(truth, pred))
        for m in hits:
            if _caught(bk.check_class_counts, c, (truth, pred, keep), bk.class_counts_ref(truth, pred, **{m: True})):
                hits[m].append(c.id)
    for m, h in hits.items():
        _assert_rejected(m, h)
        assert all("outside" in i for i in h)
    for c in bk.CASES["iou_classes"]:
        if c.M * c.K > 8:
            continue
        data = bk.build_iou_classes(c)
        bk.check_iou_classes(c, data, bk.iou_classes_ref(c, *data))
        wrong = bk.iou_classes_ref(c, *data)
        wrong[..., 0] -= 1
        assert _caught(bk.check_iou_classes, c, data, wrong)


def test_warp_mutations():
    hits = {m: [] for m in ("trunc", "clamp_edge", "swap_xy", "tf0", "proj0")}
    for c in bk.CASES["warp"]:
        if c.c not in (1, 3) or c.n * c.out_hw[0] * c.out_hw[1] > SMALL:
            continue
        data = bk.build_warp(c)
        for m in hits:
            if _caught(bk.check_warp, c, data, bk.warp_np(*data, mut=m)):
                hits[m].append(c.id)
    for m, h in hits.items():
        _assert_rejected(m, h)
    assert any(i.startswith("frac_neg") for i in hits["trunc"]) and all(i.startswith("proj_zero") for i in hits["proj0"])
    assert all(i.endswith("b") for i in hits["tf0"])
    hits = {m: [] for m in ("half_even", "swap_xy", "tf0", "proj0")}
    for c in bk.CASES["nearest"]:
        data = bk.build_warp(c)
        for m in hits:
            if _caught(bk.check_warp, c, data, bk.warp_np(*data, nearest=True, mut=m)):
                hits[m].append(c.id)
    for m, h in hits.items():
        if m != "proj0":                    # (nearest: an infinite coordinate is out of frame with or without the proj test)
            _assert_rejected("nearest:" + m, h)
    assert all(i.startswith(("shift", "proj_zero")) for i in hits["half_even"])             # the transforms with exact halves
    hits = {m: [] for m in ("trunc", "clamp_edge", "swap_xy", "tf0", "cols256")}
    for c in bk.CASES["augment"]:
        data = bk.build_augment(c)
        for m in hits:
            if _caught(bk.check_augment, c, data, bk.augment_np(*data[:3], mut=m)):
                hits[m].append(c.id)
    for m, h in hits.items():
        _assert_rejected("augment:" + m, h)
    assert all(i.startswith(("3x5x300", "2x3x257")) for i in hits["cols256"])


# ---- the wrappers' checks come before any device pointer is taken ---------------------------------------------------------------
def test_wrapper_shape_checks_run_on_the_host():
    from asr_amd import ops
    from asr_amd._lib import AsrError
    x = torch.zeros(10)
    li = torch.zeros(10, dtype=torch.int32)
    for segments in (3, 4, 11, 0):
        with pytest.raises(AsrError, match="threshold: image does not split into equal non-empty segments"):
            ops.threshold(x, 8, segments=segments)
        with pytest.raises(AsrError, match="iou_counts: truth / pred do not split into equal non-empty segments"):
            ops.iou_counts(li, li, 8, segments=segments)
    with pytest.raises(AsrError, match="threshold: out size mismatch"):
        ops.threshold(x, 8, out=torch.zeros(9, dtype=torch.int32))
    with pytest.raises(AsrError, match="threshold: out must be a contiguous int32 tensor, got torch.float32"):
        ops.threshold(x, 8, out=torch.zeros(10))
    with pytest.raises(AsrError, match=r"threshold: out must be a contiguous int32 tensor, got torch.int32 \(not contiguous\)"):
        ops.threshold(x, 8, out=torch.zeros(10, 2, dtype=torch.int32)[:, 0])
    logits0 = torch.zeros(4, 5, 3)
    for shape in ((8, 9), (80,), (1, 8, 10), (10, 8)):
        with pytest.raises(AsrError, match=r"standard_mask: out must be \(8, 10\)"):
            ops.standard_mask(logits0, (8, 10), 1, out=torch.zeros(shape, dtype=torch.int32))
    # M = 0 never reaches the library; neither does a pixel count that does not match
    with pytest.raises(AsrError, match="iou_counts_classes: size mismatch"):
        ops.iou_counts_classes(li, torch.zeros(1, 0, 10, dtype=torch.int32), [8])
    # a correct call gets past the new checks to the device-pointer check
    with pytest.raises(AsrError, match="on the CPU"):
        ops.threshold(x, 8, segments=2)
    with pytest.raises(AsrError, match="on the CPU"):
        ops.iou_counts(li, li, 8, segments=5)
    with pytest.raises(AsrError, match="on the CPU"):
        ops.standard_mask(logits0, (8, 10), 1, out=torch.zeros(8, 10, dtype=torch.int32))
