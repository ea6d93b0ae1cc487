"""The base kernels of csrc/reduce.hip on the GPU at their edges: minmax across workgroups with negative, zero, +-FLT_MAX and
infinite extremes at the ends of every workgroup's share; the second trip of every capped grid with a full and a ragged tile;
32 / 33 classes on either side of the LDS staging limit and one class; ties, +-0.0 and infinite logits; thresholds equal to a
pixel, of a negative maximum, and where the float32 product differs from the exact one; labels outside 0..255; the segmented
forms; the refusals.

Cases, data, references and checks: tests/base_kernel_cases.py, shared with tests/test_base_kernel_cases_host.py, which shows on
the CPU that the table reaches these paths and that subtly wrong kernels fail these checks on this data.  Exact where the result
is defined exactly (min / max, argmax, counts, thresholds, the float32 normalisation bit for bit); class_activation within the
bounds of test_class_activation_matches_torch against float64.  Each activation test prints its largest error ("MAXERR")."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))      # tests/base_kernel_cases.py, whatever pytest's import mode
import base_kernel_cases as bk  # noqa: E402
from oracle import augment as o_aug  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _free_big_cases():
    yield
    bk.free_big()
    torch.cuda.empty_cache()


def _up(dev, a):
    a = np.ascontiguousarray(a)
    return (torch.from_numpy(a) if a.flags.writeable else torch.tensor(a)).to(dev)       # (the cached big cases are read-only)


def _down(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("id", bk.ids("minmax"))
def test_minmax(dev, id):
    from asr_amd import ops
    case = bk.case_by_id("minmax", id)
    x, _ = bk.build_minmax(case)
    got = _down(ops.minmax(_up(dev, x), segments=case.segments))
    bk.check_minmax(case, x, got)


@pytest.mark.parametrize("id", bk.ids("normalize"))
def test_minmax_normalize(dev, id):
    from asr_amd import ops
    case = bk.case_by_id("normalize", id)
    x = bk.build_normalize(case)
    xd = _up(dev, x)
    got = _down(ops.minmax_normalize(xd, segments=case.segments, new_min=case.new_min, new_max=case.new_max))
    bk.check_normalize(case, x, got)
    assert bk.same_bits(_down(xd), x), (id, "the input changed")


@pytest.mark.parametrize("id", bk.ids("opm_slice"))
def test_opm_slice(dev, id):
    from asr_amd import ops
    case = bk.case_by_id("opm_slice", id)
    x = bk.build_opm_slice(case)
    xd = _up(dev, x)
    for cid in case.class_ids:
        bk.check_opm_slice(case, x, cid, _down(ops.opm_slice(xd, cid, new_min=case.new_min, new_max=case.new_max)))


@pytest.mark.parametrize("id", bk.ids("argmax"))
def test_argmax(dev, id):
    from asr_amd import ops
    case = bk.case_by_id("argmax", id)
    x = bk.build_logits(case)
    bk.check_argmax(case, x, _down(ops.argmax(_up(dev, x))))


@pytest.mark.parametrize("id", bk.ids("opm_argmax"))
def test_opm_argmax(dev, id):
    from asr_amd import ops
    case = bk.case_by_id("opm_argmax", id)
    x = bk.build_logits(case)
    xd = _up(dev, x)
    for cid in case.class_ids:
        bk.check_opm_argmax(case, x, cid, _down(ops.opm_argmax(xd, cid)))


@pytest.mark.parametrize("id", bk.ids("slice_max"))
def test_opm_slice_max(dev, id):
    from asr_amd import ops
    case = bk.case_by_id("slice_max", id)
    x = bk.build_logits(case)
    xd = _up(dev, x)
    for cid in case.class_ids:                          # two classes: the id first and last
        cls, mx = ops.opm_slice_max(xd, cid)
        bk.check_slice_max(case, x, cid, _down(cls), _down(mx))


def test_opm_slice_max_refuses_one_class(dev):
    from asr_amd import ops
    from asr_amd._lib import AsrError
    with pytest.raises(AsrError, match="asr_opm_slice_max_f32"):
        ops.opm_slice_max(torch.zeros(5, 1, device=dev), 0)


@pytest.mark.parametrize("id", bk.ids("activation"))
def test_class_activation(dev, id):
    from asr_amd import ops
    case = bk.case_by_id("activation", id)
    x = bk.build_activation(case)
    xd = _up(dev, x)
    for kind in ("softmax", "sigmoid"):
        err = bk.check_activation(case, x, kind, _down(ops.class_activation(xd, kind)))
        print(f"MAXERR {id} {kind} {err:.3e}")
    assert bk.same_bits(_down(xd), x), (id, "the input changed")


@pytest.mark.parametrize("id", bk.ids("threshold"))
def test_threshold(dev, id):
    from asr_amd import ops
    case = bk.case_by_id("threshold", id)
    data = bk.build_threshold(case)
    img, mask, fac, value = data
    got = ops.threshold(_up(dev, img), value, th_factor=fac, th_mask=None if mask is None else _up(dev, mask), segments=case.segments)
    bk.check_threshold(case, data, _down(got))
    # into a given buffer: the same bytes
    out = torch.full(img.shape, -7, dtype=torch.int32, device=dev)
    ops.threshold(_up(dev, img), value, th_factor=fac, th_mask=None if mask is None else _up(dev, mask), segments=case.segments, out=out)
    assert torch.equal(out, got), id


@pytest.mark.parametrize("id", bk.ids("iou"))
def test_iou_counts(dev, id):
    from asr_amd import ops
    case = bk.case_by_id("iou", id)
    truth, pred = bk.build_iou(case)
    got = _down(ops.iou_counts(_up(dev, truth), _up(dev, pred), case.class_id, include_bg=case.include_bg, segments=case.segments))
    bk.check_iou(case, (truth, pred), got)
    for s in range(case.segments):                      # and the ratio the reference makes of them
        assert bk.iou_ratio(got[s], case.include_bg) == o_aug.single_class_IOU(truth[s], pred[s], case.class_id, case.include_bg), (id, s)


@pytest.mark.parametrize("id", bk.ids("iou_shared"))
def test_iou_counts_shared_truth(dev, id):
    from asr_amd import ops
    case = bk.case_by_id("iou_shared", id)
    truth, pred = bk.build_iou(case)
    got = _down(ops.iou_counts_shared_truth(_up(dev, truth), _up(dev, pred), case.class_id, include_bg=case.include_bg))
    bk.check_iou(case, (truth, pred), got)
    for s in range(case.segments):
        assert bk.iou_ratio(got[s], case.include_bg) == o_aug.single_class_IOU(truth, pred[s], case.class_id, case.include_bg), (id, s)


@pytest.mark.parametrize("id", bk.ids("iou_classes"))
def test_iou_counts_classes(dev, id):
    from asr_amd import ops
    case = bk.case_by_id("iou_classes", id)
    data = bk.build_iou_classes(case)
    ids, truth, preds = data
    got = _down(ops.iou_counts_classes(_up(dev, truth), _up(dev, preds), ids, include_bg=case.include_bg))
    bk.check_iou_classes(case, data, got)


@pytest.mark.parametrize("m", [0, bk.MAX_IOU_MASKS + 1])
def test_iou_counts_classes_refuses_mask_counts(dev, m):
    from asr_amd import ops
    from asr_amd._lib import AsrError
    truth = torch.zeros(300, dtype=torch.int32, device=dev)
    preds = torch.zeros((2, m, 300), dtype=torch.int32, device=dev)
    with pytest.raises(AsrError, match="size mismatch" if m == 0 else "1..8 masks"):
        ops.iou_counts_classes(truth, preds, [3, 8])


@pytest.mark.parametrize("id", bk.ids("class_counts"))
def test_class_counts(dev, id):
    from asr_amd import ops
    case = bk.case_by_id("class_counts", id)
    data = bk.build_class_counts(case)
    truth, pred, _ = data
    got = _down(ops.class_counts(_up(dev, truth), _up(dev, pred), segments=case.segments))
    bk.check_class_counts(case, data, got)
    if case.kind != "outside":
        for s in range(case.segments):
            o, m = o_aug.Mean_IOU(truth[s], pred[s]), bk.mean_iou_of_counts(got[s])
            assert o == m or (np.isnan(o) and np.isnan(m)), (id, s, o, m)
