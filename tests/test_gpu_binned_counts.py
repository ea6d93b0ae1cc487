"""asr_binned_class_counts_f32 (csrc/reduce.hip: binned_hist_kernel): asr_class_counts_i32's counts over the pixels whose u lies
at or below each of B device-side edges, integer-exact against a numpy restatement of the rule of include/asr_hip.h."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PIXELS = (1, 63, 64, 65, 1025, 70001)          # 70 001: past one trip of a workgroup's loop (64 x 256) and past one workgroup
PREDS = (1, 4, 8)
BINS = (1, 5, 16)
LABELS = np.array(list(range(21)) + [255, -3, 256, 300], np.int32)
F32 = np.float32


def _edges(num_bins):
    """Unsorted, repeated, with +0.0 (against u's -0.0), +inf, a negative value and a NaN among them."""
    pool = np.array([0.5, 0.0, np.inf, 0.25, 0.5, -1.0, 0.75, np.nan, 0.0, 1.0, 0.125, np.inf, 0.25, 0.9, 0.6, -np.inf], F32)
    return pool[:num_bins].copy() if num_bins > 1 else np.array([0.5], F32)


def _problem(pixels, num_preds, seed):
    rng = np.random.default_rng(seed)
    truth = rng.choice(LABELS, pixels)
    preds = np.where(rng.uniform(size=(num_preds, pixels)) < 0.6, truth[None], rng.choice(LABELS, (num_preds, pixels))).astype(np.int32)
    # heavy ties at 0 (both signs), values equal to an edge, +inf and NaN
    u = rng.choice(np.array([0.0, -0.0, 0.0, 0.25, 0.5, 0.75, 0.3, 0.6, 2.0, np.inf, np.nan], F32), pixels)
    some = rng.uniform(size=pixels) < 0.3
    u = np.where(some, rng.uniform(0, 1, pixels).astype(F32), u).astype(F32)
    return truth, preds, u


def _rule(truth, preds, u, edges, ignore):
    out = np.zeros((preds.shape[0], len(edges), 3, 256), np.int64)
    with np.errstate(invalid="ignore"):
        for j, e in enumerate(edges):
            held = u <= e                                      # f32 compare: NaN on either side is False, -0 <= +0 is True
            if ignore != -1:
                held = held & (truth != ignore)
            t = truth[held]
            t_ok = (t >= 0) & (t < 256)
            for p in range(preds.shape[0]):
                q = preds[p][held]
                q_ok = (q >= 0) & (q < 256)
                out[p, j, 0] = np.bincount(t[t_ok], minlength=256)
                out[p, j, 1] = np.bincount(q[q_ok], minlength=256)
                out[p, j, 2] = np.bincount(t[t_ok & (t == q)], minlength=256)
    return out


@pytest.mark.parametrize("pixels", PIXELS)
def test_against_numpy(dev, pixels):
    from asr_amd import ops
    for num_preds in PREDS:
        truth, preds, u = _problem(pixels, num_preds, 1000 + pixels + num_preds)
        td, pd, ud = (torch.as_tensor(a).to(dev) for a in (truth, preds, u))
        for num_bins in BINS:
            edges = _edges(num_bins)
            ed = torch.as_tensor(edges).to(dev)
            for ignore in (255, -1):
                got = ops.binned_class_counts(td, pd, ud, ed, ignore_label=ignore)
                assert got.dtype == torch.int64 and tuple(got.shape) == (num_preds, num_bins, 3, 256)
                want = _rule(truth, preds, u, edges, ignore)
                assert np.array_equal(got.cpu().numpy(), want), (pixels, num_preds, num_bins, ignore)
            assert np.array_equal(ops.binned_class_counts(td, pd, ud, ed, ignore_label=None).cpu().numpy(), want)
    if pixels >= 1025:
        assert want[:, 0].any() and (want[:, 0, 0, 255] > 0).any()      # ignore -1: void is counted as a label


def test_the_edge_cases_mean_what_the_header_says(dev):
    from asr_amd import ops
    truth = torch.tensor([1, 1, 1, 1, 1, 255, -3, 300], dtype=torch.int32, device=dev)
    pred = torch.tensor([[1, 2, 1, 1, 1, 1, 1, 1]], dtype=torch.int32, device=dev)
    u = torch.tensor([-0.0, 0.0, 0.5, float("inf"), float("nan"), 0.0, 0.0, 0.0], dtype=torch.float32, device=dev)
    edges = torch.tensor([0.0, float("inf"), float("nan"), 0.5, 0.0], dtype=torch.float32, device=dev)
    c = ops.binned_class_counts(truth, pred, u, edges, ignore_label=255).cpu().numpy()[0]
    # [truth == 1, pred == 1, both] per bin; the void pixel is in no bin, the labels -3 and 300 count nowhere as truth
    assert [tuple(c[j, :, 1]) for j in range(5)] == [(2, 3, 1), (4, 5, 3), (0, 0, 0), (3, 4, 2), (2, 3, 1)]
    assert c[:, 0].sum(axis=-1).tolist() == [2, 4, 0, 3, 2] and c[:, :, 255].sum() == 0
    c = ops.binned_class_counts(truth, pred, u, edges, ignore_label=-1).cpu().numpy()[0]
    assert [tuple(c[j, :, 1]) for j in range(5)] == [(2, 4, 1), (4, 6, 3), (0, 0, 0), (3, 5, 2), (2, 4, 1)]
    assert c[:, 0, 255].tolist() == [1, 1, 0, 1, 1]


@pytest.mark.parametrize("pixels", [65, 70001])
def test_all_inf_edges_are_class_counts(dev, pixels):
    """Every edge +inf, no NaN in u, ignore_label -1: each bin is asr_class_counts_i32's counts bit for bit."""
    from asr_amd import ops
    for num_preds, num_bins in ((1, 1), (4, 5), (8, 16)):
        truth, preds, u = _problem(pixels, num_preds, 77 + pixels)
        u = np.nan_to_num(u, nan=3.0, posinf=np.inf)
        td, pd, ud = (torch.as_tensor(a).to(dev) for a in (truth, preds, u))
        ed = torch.full((num_bins,), float("inf"), dtype=torch.float32, device=dev)
        got = ops.binned_class_counts(td, pd, ud, ed, ignore_label=-1)
        for p in range(num_preds):
            plain = ops.class_counts(td, pd[p].contiguous())[0]
            for j in range(num_bins):
                assert torch.equal(got[p, j], plain), (pixels, p, j)
        out = torch.full((num_preds * num_bins * 768,), -7, dtype=torch.int64, device=dev)       # out=: zeroed by the call
        again = ops.binned_class_counts(td, pd, ud, ed, ignore_label=-1, out=out)
        assert torch.equal(again, got) and again.data_ptr() == out.data_ptr()


def test_ops_refuses_bad_sizes(dev):
    from asr_amd import _lib, ops
    t = torch.zeros(16, dtype=torch.int32, device=dev)
    u = torch.zeros(16, dtype=torch.float32, device=dev)
    e = torch.zeros(3, dtype=torch.float32, device=dev)
    for kw in (dict(preds=torch.zeros(15, dtype=torch.int32, device=dev)), dict(u=u[:8]), dict(preds=t.repeat(9)),
               dict(edges=torch.zeros(17, device=dev)), dict(edges=torch.zeros((1, 3), device=dev)), dict(edges=e[:0]),
               dict(out=torch.zeros(5, dtype=torch.int64, device=dev)), dict(edges=e.cpu())):
        args = dict(truth=t, preds=t, u=u, edges=e)
        out = kw.pop("out", None)
        args.update(kw)
        with pytest.raises(_lib.AsrError):
            ops.binned_class_counts(args["truth"], args["preds"], args["u"], args["edges"], out=out)


def test_risk_coverage_helpers(dev):
    """utils.risk_coverage_counts / risk_coverage_mIoU: the 100 % row is Mean_IOU's own counts without void, rows are nested,
    and an informative u (large exactly where the prediction is wrong) makes the curve rise as the coverage falls."""
    from asr_amd import ops, utils
    rng = np.random.default_rng(4)
    truth = rng.choice(np.array([0, 0, 0, 5, 9, 255], np.int32), (40, 50))
    pred = np.where(rng.uniform(size=truth.shape) < 0.7, truth, 5).astype(np.int32)
    pred[truth == 255] = 0
    u = np.where(pred != truth, 1.0, 0.0).astype(F32) + rng.uniform(0, 0.5, truth.shape).astype(F32)
    percents = [50, 90, 100]                # about 76 % of the counted pixels are right: the 50 % row holds none of the wrong ones
    counts, share = utils.risk_coverage_counts(truth, pred, u, percents, return_share=True)
    assert counts.shape == (3, 3, 256) and counts.dtype == np.int64
    keep = truth != 255
    plain = ops.class_counts(torch.as_tensor(truth[keep]).to(dev), torch.as_tensor(pred[keep]).to(dev))[0].cpu().numpy()
    assert np.array_equal(counts[2], plain)
    assert (np.diff(counts, axis=0) >= 0).all() and (share >= np.array(percents) / 100).all() and share[2] == 1.0
    miou = utils.risk_coverage_mIoU(truth, pred, u, percents)
    assert miou.shape == (3,) and miou[0] == 1.0 and miou[0] > miou[1] > miou[2] == utils.mean_iou_from_counts(plain)
