"""asr_threshold_sweep_iou_counts_f32 (ops.threshold_sweep_iou_counts): the IoU counts of K threshold factors in one pass,
bit for bit equal to K separate threshold + iou_counts launches and to a numpy restatement."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _np_counts(images, truth, factors, class_id, include_bg):
    """[S, K, 4] int64: threshold_image (v > f32(max) * f32(f)) then single_class_IOU's integer counts, in numpy."""
    s = images.shape[0]
    imgs = images.reshape(s, -1).astype(np.float32)
    tr = truth.reshape(-1, imgs.shape[1]).astype(np.int64)
    tr = np.broadcast_to(tr, imgs.shape) if tr.shape[0] == 1 else tr
    out = np.zeros((s, len(factors), 4), np.int64)
    for i in range(s):
        t = tr[i].copy()
        if include_bg:
            t[t != class_id] = 0
        mx = imgs[i].max()
        for k, f in enumerate(factors):
            th = np.float32(mx) * np.float32(f)
            p = np.where(imgs[i] > th, class_id, 0)
            tc, pc, tb, pb = t == class_id, p == class_id, t == 0, p == 0
            out[i, k] = [(tc & pc).sum(), (tc | pc).sum(), (tb & pb).sum(), (tb | pb).sum()]
    return out


def _separate(ops, imgs_dev, truth_dev, factors, class_id, include_bg):
    """K threshold launches + K IoU-count launches per image: what the sweep replaces."""
    import torch
    s = imgs_dev.shape[0]
    per = imgs_dev[0].numel()
    out = []
    for i in range(s):
        t = truth_dev if truth_dev.numel() == per else truth_dev.reshape(s, -1)[i].contiguous()
        row = []
        for f in factors:
            m = ops.threshold(imgs_dev[i].contiguous(), class_id, th_factor=float(f))
            row.append(ops.iou_counts(t.reshape(-1), m.reshape(-1), class_id, include_bg=include_bg)[0])
        out.append(torch.stack(row))
    return torch.stack(out).cpu().numpy()


def _images(rng, s, h, w, kind="random"):
    x = rng.standard_normal((s, h, w)).astype(np.float32)
    if kind == "negative":
        x = -np.abs(x) - 0.25
    elif kind == "zero":
        x = -np.abs(x)
        x[:, 0, 0] = 0.0
    elif kind == "equal":
        x[:] = 0.75
    return x


def _truth(rng, s, h, w, class_id, shared):
    n = 1 if shared else s
    t = rng.choice([0, class_id, 3, 255], size=(n, h, w), p=[0.4, 0.35, 0.15, 0.1]).astype(np.int32)
    return t[0] if shared else t


def _check(dev, images, truth, factors, class_id, include_bg):
    import torch
    from asr_amd import ops
    imgs = torch.as_tensor(images).to(dev).contiguous()
    tr = torch.as_tensor(truth).to(dev).contiguous()
    got = ops.threshold_sweep_iou_counts(imgs, tr, factors, class_id, include_bg=include_bg).cpu().numpy()
    assert got.shape == (images.shape[0], len(factors), 4) and got.dtype == np.int64
    np.testing.assert_array_equal(got, _np_counts(images, truth, factors, class_id, include_bg))
    np.testing.assert_array_equal(got, _separate(ops, imgs, tr, factors, class_id, include_bg))
    return got


FACTORS_17 = [round(v, 2) for v in np.arange(0.1, 0.95, 0.05)]


@pytest.mark.parametrize("hw", [(512, 512), (37, 53)])
@pytest.mark.parametrize("s,shared", [(1, True), (3, False), (16, True)])
@pytest.mark.parametrize("class_id", [8, 0])
def test_sweep_counts_match_separate_launches(dev, hw, s, shared, class_id):
    rng = np.random.default_rng(hw[0] * 1000 + s * 10 + class_id)
    images = _images(rng, s, *hw)
    truth = _truth(rng, s, *hw, class_id if class_id else 8, shared)
    for include_bg in (False, True):
        got = _check(dev, images, truth, FACTORS_17, class_id, include_bg)
        if class_id == 8:
            assert len(np.unique(got[..., 0])) > 3           # the factors really split the pixels differently


@pytest.mark.parametrize("k", [1, 17, 256])
def test_factor_counts_unsorted_and_repeated(dev, k):
    rng = np.random.default_rng(k)
    images = _images(rng, 3, 37, 53)
    truth = _truth(rng, 3, 37, 53, 8, False)
    factors = list(rng.uniform(-0.2, 1.1, size=k).astype(np.float32))
    if k > 1:
        factors[k // 2] = factors[0]                       # repeats
        factors[-1] = factors[1]
    for include_bg in (False, True):
        _check(dev, images, truth, factors, 8, include_bg)


def test_ties_on_the_threshold(dev):
    """Pixels exactly equal to f32(max) * f32(f) are off (strict >), their neighbours one ulp above are on."""
    rng = np.random.default_rng(3)
    x = _images(rng, 2, 64, 64)
    factors = [0.25, 0.5, 0.65, 0.65, 1.0]
    for i in range(2):
        mx = x[i].max()
        flat = x[i].reshape(-1)
        for j, f in enumerate(factors):
            th = np.float32(mx) * np.float32(f)
            flat[100 * j: 100 * j + 40] = th
            flat[100 * j + 40: 100 * j + 60] = np.nextafter(th, np.float32(np.inf))
            flat[100 * j + 60: 100 * j + 80] = np.nextafter(th, np.float32(-np.inf))
    truth = _truth(rng, 2, 64, 64, 8, False)
    for include_bg in (False, True):
        _check(dev, x, truth, factors, 8, include_bg)


@pytest.mark.parametrize("kind", ["equal", "negative", "zero"])
def test_special_maxima(dev, kind):
    """An all-equal image, a negative maximum (the threshold order reverses against the factor order) and a zero one."""
    rng = np.random.default_rng(11)
    images = _images(rng, 3, 37, 53, kind)
    truth = _truth(rng, 3, 37, 53, 8, True)
    for class_id in (8, 0):
        for include_bg in (False, True):
            _check(dev, images, truth, FACTORS_17 + [0.0, -0.5, 1.5], class_id, include_bg)


def test_superres_utils_threshold_sweep_IoU(dev):
    from asr_amd.superresolution_scripts.superres_utils import threshold_image, threshold_sweep_IoU
    from asr_amd.utils import compute_IoU
    rng = np.random.default_rng(5)
    img = rng.standard_normal((128, 128, 1)).astype(np.float32)
    truth = _truth(rng, 1, 128, 128, 8, True)[..., None]
    for include_bg in (False, True):
        got = threshold_sweep_IoU(truth, img, 8, FACTORS_17, include_bg=include_bg)
        expect = [compute_IoU(truth, threshold_image(img, 8, th_factor=f), img_size=(128, 128), class_id=8,
                              include_bg=include_bg) for f in FACTORS_17]
        assert got.dtype == np.float64 and got.shape == (17,)
        np.testing.assert_array_equal(got, np.array(expect))


def test_refusals_return_errors_without_launching(dev, lib):
    import torch
    from asr_amd import _lib, ops
    fake = 1 << 20                                           # non-null; refused on the host, never dereferenced
    ws = lib.asr_threshold_sweep_workspace_bytes(1, 17)
    assert ws == 8 * 4 * 18 + 8
    assert lib.asr_threshold_sweep_workspace_bytes(0, 17) == 0
    call = lambda *a: lib.asr_threshold_sweep_iou_counts_f32(fake, fake, fake, fake, *a, None)
    assert call(ws, fake, 100, 1, 0, 1, 8, 0) == -1 and b"threshold factors" in lib.asr_last_error()
    assert call(ws, fake, 100, 1, 257, 1, 8, 0) == -1 and b"threshold factors" in lib.asr_last_error()
    assert call(1 << 40, fake, 100, 65536, 17, 1, 8, 0) == -1 and b"65535" in lib.asr_last_error()
    assert call(ws - 1, fake, 100, 1, 17, 1, 8, 0) == -4 and b"workspace" in lib.asr_last_error()
    assert lib.asr_threshold_sweep_iou_counts_f32(None, fake, fake, fake, ws, fake, 100, 1, 17, 1, 8, 0, None) == -1
    imgs = torch.zeros((2, 10), device=dev)
    truth = torch.zeros(10, dtype=torch.int32, device=dev)
    with pytest.raises(_lib.AsrError, match="threshold factors"):
        ops.threshold_sweep_iou_counts(imgs, truth, np.zeros(257), 8)
    with pytest.raises(_lib.AsrError, match="truth"):
        ops.threshold_sweep_iou_counts(imgs, truth[:7], [0.5], 8)
    torch.cuda.synchronize()
