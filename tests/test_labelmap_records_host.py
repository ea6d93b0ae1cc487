"""The record layout of the label-map scores, stated a second time: the device buffer of pipeline._LabelCounts and the
all-gather record of evaluation.gather_labelmap_records against the offset arithmetic written out below, for every on/off
combination of the four optional scores.  The restatement is deliberate: an edit of label_record's field list that moves data
fails here."""
import itertools
import pickle

import numpy as np
import pytest
import torch

B, L, T, C = 2, 3, 3, 2                       # band widths, confusion labels, threshold factors, coverages
ALL_KEYS = ("standard", "aug", "max", "mean")
KEY_SETS = (ALL_KEYS, ("aug",))
COMBOS = list(itertools.product((0, B), (0, L), (0, T), (0, C)))
assert len(COMBOS) == 16


def _device_offsets(keys, b, l, t, c):
    """Where each score starts in the int64 buffer: counts, band, confusion, sweep, coverage, retained, end."""
    m = len(keys)
    ms = len([k for k in keys if k != "standard"]) if t else 0
    split = m * 768
    conf = split * (1 + b)
    cells = (l + 1) ** 2 if l else 0
    sweep = conf + m * cells
    cov = sweep + ms * t * 768
    ret = cov + m * c * 768
    return split, conf, sweep, cov, ret, ret + (c + 1 if c else 0)


@pytest.mark.parametrize("keys", KEY_SETS, ids=lambda k: "+".join(k))
@pytest.mark.parametrize("b,l,t,c", COMBOS)
def test_label_counts_buffer_and_to_host(keys, b, l, t, c):
    from asr_amd.label_record import label_fields
    from asr_amd.pipeline import _LabelCounts
    from asr_amd.utils import mean_iou_from_counts
    m, sr_keys = len(keys), [k for k in keys if k != "standard"]
    split, conf, sweep, cov, ret, end = _device_offsets(keys, b, l, t, c)
    tally = _LabelCounts(label_fields(keys, b, l, t, c), torch.device("cpu"))
    assert tally._buf.dtype == torch.int64 and tally._buf.numel() == end
    tally._buf.copy_(torch.arange(end))
    host = np.arange(end, dtype=np.int64)

    # the views the ops.*_counts(out=...) calls write into: their place and their length
    def at(view, lo, hi):
        assert view.numel() == hi - lo and view.is_contiguous()
        assert np.array_equal(view.reshape(-1).numpy(), host[lo:hi])

    at(tally.counts, 0, split)
    assert tuple(tally.counts.shape) == (m, 3, 256)                          # row j: label map j
    if b:
        at(tally.band, split, conf)
        assert tally.band.numel() == m * b * 768
    if l:
        at(tally.confusion, conf, sweep)
        assert tally.confusion.numel() == m * (l + 1) * (l + 1)
    if t:
        at(tally.sweep, sweep, cov)
        assert tuple(tally.sweep.shape) == (len(sr_keys), t, 3, 256)         # row i: SR type i
    if c:
        at(tally.coverage, cov, ret)
        assert tally.coverage.numel() == m * c * 768
    at(tally.retained, ret, end)
    assert tally.retained.numel() == (c + 1 if c else 0)

    miou = lambda stack: np.array([mean_iou_from_counts(x) for x in stack], dtype=np.float64)
    counts = host[:split].reshape(m, 3, 256)
    exp = {"counts": {k: counts[j] for j, k in enumerate(keys)},
           "Mean_IOU": {k: mean_iou_from_counts(counts[j]) for j, k in enumerate(keys)}}
    if b:
        band = host[split:conf].reshape(m, b, 3, 256)
        exp["band_counts"] = {k: band[j] for j, k in enumerate(keys)}
        exp["band_Mean_IOU"] = {k: miou(band[j]) for j, k in enumerate(keys)}
    if l:
        mat = host[conf:sweep].reshape(m, l + 1, l + 1)
        exp["confusion"] = {k: mat[j] for j, k in enumerate(keys)}
    if t:
        sw = host[sweep:cov].reshape(len(sr_keys), t, 3, 256)
        exp["sweep_counts"] = {k: sw[i] for i, k in enumerate(sr_keys)}
        exp["sweep_Mean_IOU"] = {k: miou(sw[i]) for i, k in enumerate(sr_keys)}
    if c:
        cv = host[cov:ret].reshape(m, c, 3, 256)
        exp["coverage_counts"] = {k: cv[j] for j, k in enumerate(keys)}
        exp["coverage_Mean_IOU"] = {k: miou(cv[j]) for j, k in enumerate(keys)}
        exp["coverage_share"] = np.float64(host[ret:end - 1]) / np.float64(host[end - 1])
    got = tally.to_host()
    assert list(got) == list(exp)
    for name, want in exp.items():
        if name == "coverage_share":
            assert got[name].dtype == np.float64 and np.array_equal(got[name], want)
            continue
        assert list(got[name]) == list(want), name
        for k in want:
            if name == "Mean_IOU":
                assert isinstance(got[name][k], float)
            elif name.endswith("Mean_IOU"):
                assert got[name][k].dtype == np.float64 and got[name][k].shape == want[k].shape
            else:
                assert got[name][k].dtype == np.int64 and got[name][k].shape == want[k].shape
            np.testing.assert_array_equal(got[name][k], want[k], err_msg=f"{name}[{k}]")


@pytest.mark.parametrize("b,l,t,c", COMBOS)
def test_one_rank_gather_record_and_result(monkeypatch, b, l, t, c):
    from asr_amd import evaluation as E
    rng = np.random.default_rng(7)
    m, ms, side = 4, 3, (l + 1 if l else 0)
    num_images, mine = 3, [0, 2]                                            # no rank reports image 1
    n = len(mine)
    data = {"": (rng.random((n, m)), rng.integers(0, 1000, (n, m, 3, 256))),
            "band_": (rng.random((n, m, B)), rng.integers(0, 1000, (n, m, B, 3, 256))),
            "confusion": (None, rng.integers(0, 1000, (n, m, L + 1, L + 1))),
            "sweep_": (rng.random((n, ms, T)), rng.integers(0, 1000, (n, ms, T, 3, 256))),
            "coverage_": (rng.random((n, m, C)), rng.integers(0, 1000, (n, m, C, 3, 256)))}
    data[""][0][1, 2] = np.nan                                              # a NaN Mean_IOU travels as it is
    fields = E.label_fields(E.LABELMAP_KEYS, b, l, t, c)
    assert [f.prefix for f in fields] == [p for p, on in zip(data, (1, b, l, t, c)) if on]
    sent = []
    real = E.D.all_gather_rows

    def spy(indices, rows, total, width):
        sent.append((list(indices), np.array(rows), total, width))
        return real(indices, rows, total, width)

    monkeypatch.setattr(E.D, "all_gather_rows", spy)
    out = E.gather_labelmap_records(mine, fields, {f: data[f.prefix] for f in fields}, num_images)

    # what travelled: one float64 record per image, Mean_IOU cells then count cells of each score in turn
    base = m + m * 768
    conf = base + m * b + m * b * 768
    sweep = conf + m * side * side
    cov = sweep + ms * t + ms * t * 768
    width = cov + m * c + m * c * 768
    assert len(sent) == 1
    indices, rec, total, got_width = sent[0]
    assert indices == mine and total == num_images and got_width == width
    assert rec.dtype == np.float64 and rec.shape == (n, width)
    flat = lambda a: np.asarray(a, dtype=np.float64).reshape(n, -1)
    np.testing.assert_array_equal(rec[:, :m], flat(data[""][0]))
    np.testing.assert_array_equal(rec[:, m:base], flat(data[""][1]))
    if b:
        np.testing.assert_array_equal(rec[:, base:base + m * b], flat(data["band_"][0]))
        np.testing.assert_array_equal(rec[:, base + m * b:conf], flat(data["band_"][1]))
    if l:
        np.testing.assert_array_equal(rec[:, conf:sweep], flat(data["confusion"][1]))
    if t:
        np.testing.assert_array_equal(rec[:, sweep:sweep + ms * t], flat(data["sweep_"][0]))
        np.testing.assert_array_equal(rec[:, sweep + ms * t:cov], flat(data["sweep_"][1]))
    if c:
        np.testing.assert_array_equal(rec[:, cov:cov + m * c], flat(data["coverage_"][0]))
        np.testing.assert_array_equal(rec[:, cov + m * c:], flat(data["coverage_"][1]))

    # what comes back: (rows, counts[, band_rows, band_counts][, confusion][, sweep_rows, sweep_counts][, cov_rows, cov_counts])
    names = ["rows", "counts"] + ["band_rows", "band_counts"] * bool(b) + ["confusion"] * bool(l) \
        + ["sweep_rows", "sweep_counts"] * bool(t) + ["cov_rows", "cov_counts"] * bool(c)
    source = {"rows": data[""][0], "counts": data[""][1], "band_rows": data["band_"][0], "band_counts": data["band_"][1],
              "confusion": data["confusion"][1], "sweep_rows": data["sweep_"][0], "sweep_counts": data["sweep_"][1],
              "cov_rows": data["coverage_"][0], "cov_counts": data["coverage_"][1]}
    assert isinstance(out, tuple) and len(out) == len(names)
    for pos, name in enumerate(names):
        got, src = out[pos], source[name]
        assert getattr(out, name) is got, name
        if name.endswith("rows"):
            assert got.dtype == np.float64 and got.shape == (num_images,) + src.shape[1:]
            np.testing.assert_array_equal(got[mine], src)                   # row for row, the NaN included
            assert np.isnan(got[1]).all()                                   # the image no rank reported
        else:
            assert got.dtype == np.int64 and got.shape == src.shape[1:]
            assert np.array_equal(got, src.sum(axis=0))
    for name in source:
        if name not in names:
            assert getattr(out, name) is None, name
    first, *rest = out                                                      # it unpacks as the tuple it was
    assert first is out.rows and len(rest) == len(names) - 1
    back = pickle.loads(pickle.dumps(out))                                  # it crosses a process queue in the gloo tests
    assert type(back) is type(out) and len(back) == len(out)
    for pos, name in enumerate(names):
        assert getattr(back, name) is back[pos]
        np.testing.assert_array_equal(back[pos], out[pos])
