"""Counterparts of the reference's utils.py hot-path helpers: ``load_image`` (utils.py:94-112),
``create_mask`` (:115-119), ``single_class_IOU`` / ``compute_IoU`` (:180-230).  Plotting and
training losses are out of scope."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, ops


def _resize_nearest_host(arr, size):
    """tf.image.resize(method='nearest'), half-pixel centres: pure index selection on the host."""
    h, w = arr.shape[:2]
    ho, wo = int(size[0]), int(size[1])

    def idx(out_size, in_size):
        scale = np.float32(in_size) / np.float32(out_size)
        o = np.arange(out_size, dtype=np.float32)
        return np.minimum(np.floor((o + np.float32(0.5)) * scale).astype(np.int64), in_size - 1)

    return arr[idx(ho, h)][:, idx(wo, w)]


def load_image(img_path, image_size=None, normalize=True, is_png=False, resize_method="bilinear"):
    """Decode (PIL) -> optional resize -> float32 [H,W,C] host array (C = 3 for jpg, 1 for png).
    Bilinear resizing runs on the GPU (asr_resize_bilinear_f32, half-pixel, no antialias)."""
    from PIL import Image
    img = Image.open(img_path)
    if not is_png:
        arr = np.asarray(img.convert("RGB"))
    else:
        arr = np.asarray(img)
        arr = arr[..., :1] if arr.ndim == 3 else arr[..., None]
    if image_size is not None:
        if resize_method == "nearest":
            arr = _resize_nearest_host(arr, image_size)
        elif resize_method == "bilinear":
            dev = _lib.require_gpu()
            c = arr.shape[-1]
            cp = (c + 3) // 4 * 4
            x = torch.zeros((1,) + arr.shape[:2] + (cp,), dtype=torch.float32, device=dev)
            x[0, :, :, :c] = torch.as_tensor(arr.astype(np.float32)).to(dev)
            arr = ops.resize_bilinear(x, image_size)[0, :, :, :c].cpu().numpy()
        else:
            raise ValueError(f"unsupported resize_method {resize_method!r}")
    arr = arr.astype(np.float32)
    if normalize:
        arr = arr / np.float32(255.0)
    return arr


def create_mask(pred_mask):
    """argmax over the class axis with a trailing singleton axis (int64, like tf.argmax)."""
    if isinstance(pred_mask, torch.Tensor) and pred_mask.is_cuda:
        return ops.argmax(pred_mask.contiguous()).to(torch.int64).unsqueeze(-1)
    t = ops.to_device(np.asarray(pred_mask, dtype=np.float32))
    return ops.argmax(t).cpu().numpy().astype(np.int64)[..., None]


def get_prediction(model, input_image):
    """utils.py:122-127: predict one image and argmax it."""
    x = input_image if isinstance(input_image, torch.Tensor) else np.asarray(input_image, dtype=np.float32)
    prediction = model.predict(x[None, ...] if not isinstance(x, torch.Tensor) else x[None].cpu().numpy())
    return create_mask(prediction[0])


def print_labels(masks):
    """utils.py:144-148: label histograms of the (standard, super-resolved) mask pair."""
    title = ["Standard Labels: ", "Superres Labels: "]
    for i in range(2):
        m = masks[i].cpu().numpy() if isinstance(masks[i], torch.Tensor) else np.asarray(masks[i])
        values, count = np.unique(m, return_counts=True)
        print(title[i] + str(dict(zip(values, count))))


def _as_label_tensor(a, dev):
    if isinstance(a, torch.Tensor):
        return a.to(device=dev, dtype=torch.int32).contiguous().reshape(-1)
    return torch.as_tensor(np.asarray(a).astype(np.int32).reshape(-1)).to(dev)


def iou_from_counts(counts, include_bg):
    """counts: [inter_c, union_c, inter_bg, union_bg] -> float64 mean of the non-NaN class IoUs."""
    with np.errstate(divide="ignore", invalid="ignore"):
        ious = [np.float64(counts[0]) / np.float64(counts[1])]
        if include_bg:
            ious.append(np.float64(counts[2]) / np.float64(counts[3]))
    ious = np.array(ious)
    ious = ious[~np.isnan(ious)]
    return float(np.mean(ious)) if len(ious) else float("nan")


def single_class_IOU(y_true, y_pred, class_id, include_bg):
    dev = _lib.require_gpu()
    t = _as_label_tensor(y_true, dev)
    p = _as_label_tensor(y_pred, dev)
    counts = ops.iou_counts(t, p, class_id, include_bg=include_bg).cpu().numpy()[0]
    return iou_from_counts(counts, include_bg)


def mean_iou_from_counts(counts):
    """counts [3, 256] (ops.class_counts) -> Mean_IOU (utils.py:151-177): mean over the labels present in the ground
    truth, void (255) removed, of inter / union; like tf.reduce_mean of an empty list, NaN when no label qualifies."""
    c = np.asarray(counts, dtype=np.int64)
    labels = [l for l in range(255) if c[0, l] > 0]
    if not labels:
        return float("nan")
    ious = [np.float64(c[2, l]) / np.float64(c[0, l] + c[1, l] - c[2, l]) for l in labels]
    return float(np.mean(ious))


def Mean_IOU(y_true, y_pred):
    dev = _lib.require_gpu()
    counts = ops.class_counts(_as_label_tensor(y_true, dev), _as_label_tensor(y_pred, dev)).cpu().numpy()[0]
    return mean_iou_from_counts(counts)


def labelmap_threshold_sweep(scores, class_ids, y_true, th_factors):
    """The per-label counts of the fused label map at every threshold factor (include/asr_hip.h,
    asr_fuse_labels_sweep_counts_f32): host int64 [T, 3, 256], row j what ops.fuse_labels(scores, class_ids,
    th_factor=th_factors[j], truth=y_true) counts.  scores [K, ...] float32, numpy or tensor: plane k is the SR output of
    class_ids[k]; y_true: a label map of as many pixels; th_factors: 1..64 factors, any order."""
    dev = _lib.require_gpu()
    s = scores.to(device=dev, dtype=torch.float32).contiguous() if isinstance(scores, torch.Tensor) \
        else ops.to_device(np.asarray(scores, dtype=np.float32), device=dev)
    return ops.fuse_labels_sweep_counts(s, class_ids, _as_label_tensor(y_true, dev), th_factors).cpu().numpy()


def labelmap_threshold_mIoU(scores, class_ids, y_true, th_factors):
    """float64 [T]: Mean_IOU of the fused label map at every threshold factor (mean_iou_from_counts of
    labelmap_threshold_sweep)."""
    counts = labelmap_threshold_sweep(scores, class_ids, y_true, th_factors)
    return np.array([mean_iou_from_counts(c) for c in counts], dtype=np.float64)


def _label_map_shape(a, img_size):
    """(H, W) of a label map given as [H, W], [H, W, 1] or flat with img_size."""
    shape = tuple(a.shape)
    if len(shape) == 3 and shape[-1] == 1:
        shape = shape[:2]
    if img_size is not None:
        hw = (int(img_size[0]), int(img_size[1]))
        if int(np.prod(shape)) != hw[0] * hw[1]:
            raise ValueError(f"expected {hw[0] * hw[1]} pixels, got {int(np.prod(shape))}")
        return hw
    if len(shape) != 2:
        raise ValueError(f"a label map of shape {shape} needs img_size=(H, W): distances to a boundary are two-dimensional")
    return shape


def trimap_counts(y_true, y_pred, widths, ignore_label=255, img_size=None):
    """Band counts of one prediction against one ground truth (include/asr_hip.h, "trimap"): int64 [B, 3, 256], row b
    what ops.class_counts counts over the pixels within widths[b] pixels (Euclidean) of a ground-truth label boundary whose
    truth is not ignore_label (-1 or None: none ignored; ignored pixels still make boundaries).  widths: 1..16 integers in
    [1, 64], any order, repeats allowed.  numpy arrays or tensors, [H, W] / [H, W, 1], or flat with img_size."""
    ws = ops.check_band_widths(widths)
    ignore = -1 if ignore_label is None else int(ignore_label)
    h, w = _label_map_shape(y_true if hasattr(y_true, "shape") else np.asarray(y_true), img_size)
    dev = _lib.require_gpu()
    t = _as_label_tensor(y_true, dev)
    p = _as_label_tensor(y_pred, dev)
    if p.numel() != t.numel():
        raise ValueError(f"expected {t.numel()} predicted pixels, got {p.numel()}")
    r_max = max(ws)
    d2 = ops.boundary_dist2(t.view(h, w), r_max)
    return ops.band_class_counts(t, p, d2, ws, r_max, ignore)[0].cpu().numpy()


def trimap_IoU(y_true, y_pred, widths, class_id=None, ignore_label=255, img_size=None):
    """float64 [B]: Mean_IOU inside the band of each width (mean_iou_from_counts of trimap_counts), or with class_id the IoU
    of that label there (NaN where neither map holds it in the band)."""
    counts = trimap_counts(y_true, y_pred, widths, ignore_label=ignore_label, img_size=img_size)
    if class_id is None:
        return np.array([mean_iou_from_counts(c) for c in counts], dtype=np.float64)
    l = int(class_id)
    if not 0 <= l <= 255:
        raise ValueError(f"class_id {l} is not a label 0..255")
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.float64(counts[:, 2, l]) / np.float64(counts[:, 0, l] + counts[:, 1, l] - counts[:, 2, l])


def confusion_matrix(y_true, y_pred, num_labels):
    """The confusion matrix of one prediction against one ground truth (include/asr_hip.h, "confusion matrix"): a host int64
    [L+1, L+1], L = num_labels in [1, 64], truth in the rows; [i, j] = the pixels whose truth falls in bin i and whose
    prediction falls in bin j, where bin(v) = v for 0 <= v < L and L ("other": void, negative values, ids >= L) otherwise.
    numpy arrays or tensors, on the host or the device, any shape with equal pixel counts."""
    n = ops.check_confusion_labels(num_labels)
    dev = _lib.require_gpu()
    t = _as_label_tensor(y_true, dev)
    p = _as_label_tensor(y_pred, dev)
    if p.numel() != t.numel():
        raise ValueError(f"expected {t.numel()} predicted pixels, got {p.numel()}")
    return ops.confusion_counts(t, p, n)[0].cpu().numpy()


def _clean_on_device(label_map, min_area, connectivity):
    min_area, connectivity = ops.check_min_region((min_area, connectivity))
    shape = tuple(label_map.shape) if hasattr(label_map, "shape") else np.asarray(label_map).shape
    if len(shape) == 3 and shape[-1] == 1:
        shape = shape[:2]
    if len(shape) not in (2, 3):
        raise ValueError(f"a label map of shape {shape}: regions are two-dimensional, [H, W] or [M, H, W]")
    t = _as_label_tensor(label_map, _lib.require_gpu()).view(shape)
    return ops.clean_labels(t, min_area, connectivity, want_stats=True)


def remove_small_regions(label_map, min_area, connectivity=4):
    """The label map cleaned of its regions of fewer than min_area pixels (include/asr_hip.h, "regions"): each takes the one
    value of its non-small surround, or 0 when that is empty or mixed.  connectivity 4 or 8.  A numpy array or tensor, on the
    host or the device, [H, W] / [H, W, 1] or [M, H, W]; returns a host int32 array of shape [H, W] or [M, H, W]."""
    return _clean_on_device(label_map, min_area, connectivity)[0].cpu().numpy()


def region_stats(label_map, min_area, connectivity=4):
    """Host int64 [4] (or [M, 4]): the number of regions, of small regions (fewer than min_area pixels), of pixels in small
    regions, and of pixels whose value remove_small_regions changes."""
    return _clean_on_device(label_map, min_area, connectivity)[1].cpu().numpy()


def segment_counts(truth, pred, num_labels=21, connectivity=8, include_zero=False):
    """The region-by-region counts of a prediction against a ground truth (include/asr_hip.h, "segments"): host int64 [L, 4],
    per label TP, FP, FN and Q, the matched IoUs summed in units of 2^-30.  A numpy array or tensor each, on the host or the
    device, [H, W] / [H, W, 1]; pred may be [M, H, W], which gives [M, L, 4]."""
    num_labels, connectivity, include_zero = ops.check_segments((num_labels, connectivity, include_zero))
    shapes = []
    for m in (truth, pred):
        shape = tuple(m.shape) if hasattr(m, "shape") else np.asarray(m).shape
        shapes.append(shape[:2] if len(shape) == 3 and shape[-1] == 1 else shape)
    if len(shapes[0]) != 2 or len(shapes[1]) not in (2, 3) or shapes[1][-2:] != shapes[0]:
        raise ValueError(f"a truth of shape {shapes[0]} and a prediction of shape {shapes[1]}: segments are two-dimensional, "
                         f"[H, W] against [H, W] or [M, H, W]")
    dev = _lib.require_gpu()
    t = _as_label_tensor(truth, dev).view(shapes[0])
    p = _as_label_tensor(pred, dev).view(shapes[1])
    return ops.segment_match(t, p, num_labels, connectivity, include_zero).cpu().numpy()


def metrics_from_segments(counts):
    """Panoptic quality from segment counts [L, 4] (TP, FP, FN, Q; utils.segment_counts, or their sum over images).  Pure
    numpy, float64, NaN where a denominator is 0:

      RQ [L]         TP / (TP + FP / 2 + FN / 2)
      SQ [L]         Q / 2^30 / TP                   the mean IoU of the matches
      PQ [L]         SQ * RQ = Q / 2^30 / (TP + FP / 2 + FN / 2), taken in that second form: 0, not NaN, for a label that has
                     segments and no match
      precision [L]  TP / (TP + FP)
      recall [L]     TP / (TP + FN)
      mean_PQ, mean_SQ, mean_RQ   over the labels with TP + FP + FN > 0 (mean_SQ: those of them with a match; NaN when there
                     is none)"""
    c = np.asarray(counts, dtype=np.int64)
    if c.ndim != 2 or c.shape[1] != 4:
        raise ValueError(f"segment counts must be [L, 4], got {c.shape}")
    tp, fp, fn, q = (np.float64(c[:, k]) for k in range(4))
    with np.errstate(divide="ignore", invalid="ignore"):
        rq = tp / (tp + fp / 2 + fn / 2)
        sq = q / float(_lib.SEGMENTS_IOU_ONE) / tp
        res = {"PQ": q / float(_lib.SEGMENTS_IOU_ONE) / (tp + fp / 2 + fn / 2), "SQ": sq, "RQ": rq, "precision": tp / (tp + fp), "recall": tp / (tp + fn)}
    seen = (c[:, :3].sum(axis=1) > 0)
    for name in ("PQ", "SQ", "RQ"):
        vals = res[name][seen & ~np.isnan(res[name])]
        res["mean_" + name] = float(np.mean(vals)) if vals.size else float("nan")
    return res


def metrics_from_confusion(M, other="ignore"):
    """The usual result table of a segmentation from one confusion matrix M [L+1, L+1] (truth in the rows, the last row and
    column the "other" bin).  Pure numpy, float64.  With row_l, col_l the sums of row and column l and d_l = M[l, l]:

      precision [L]     d_l / col_l                       NaN where the label is never predicted
      recall [L]        d_l / row_l                       NaN where the truth does not hold the label
      iou [L]           d_l / (row_l + col_l - d_l)       NaN where neither map holds the label
      pixel_accuracy    the matrix's trace over its sum
      mean_accuracy     the mean of recall over the labels the truth holds
      Mean_IOU          the mean of iou over the labels the truth holds: NaN labels are dropped and, as Mean_IOU does, a label
                        that is predicted but absent from the truth (iou 0) is not among them
      fw_iou            sum of row_l * iou_l over the labels the truth holds, over the sum of their row_l
    (NaN for a mean over no label).  The per-label arrays and the three means cover the L labels, never the other bin.

    other="ignore": the other row and the other column are dropped before anything is computed -- the VOC protocol: a pixel
    that is void in the truth (or predicted outside 0..L-1) is scored nowhere.
    other="label": the other bin stays in the matrix as a label like any other: its pixels stay in the row sums, the column
    sums, the trace and the total, so a void pixel predicted as l enters l's union.  That is how Mean_IOU treats void (255),
    so when every value outside 0..L-1 that the truth holds is void, negative or above 255 (Mean_IOU never scores those as
    a label) Mean_IOU here equals utils.mean_iou_from_counts(ops.class_counts(truth, pred)) exactly."""
    m = np.asarray(M)
    if m.ndim != 2 or m.shape[0] != m.shape[1] or m.shape[0] < 2:
        raise ValueError(f"a confusion matrix is [L+1, L+1] with L >= 1, got shape {m.shape}")
    if other not in ("ignore", "label"):
        raise ValueError(f'other must be "ignore" or "label", got {other!r}')
    m = m.astype(np.int64)
    L = m.shape[0] - 1
    if other == "ignore":
        m = m[:L, :L]
    rows, cols, diag = m.sum(axis=1)[:L], m.sum(axis=0)[:L], np.diagonal(m)[:L]
    total, trace = int(m.sum()), int(np.trace(m))
    f64 = lambda a: a.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        precision = f64(diag) / f64(cols)
        recall = f64(diag) / f64(rows)
        iou = f64(diag) / f64(rows + cols - diag)
        present = rows > 0
        nan = float("nan")
        return {"pixel_accuracy": float(np.float64(trace) / np.float64(total)) if total else nan,
                "mean_accuracy": float(np.mean(recall[present])) if present.any() else nan,
                "precision": precision, "recall": recall, "iou": iou,
                "Mean_IOU": float(np.mean(iou[present])) if present.any() else nan,
                "fw_iou": float(np.sum(f64(rows[present]) * iou[present]) / np.float64(rows[present].sum()))
                if present.any() else nan}


def opm_scales(class_ids, mode, normalised=True):
    """s_k of uncertainty_map for the stacks of class_ids: what the stack holds where class k wins.  The argmax OPM writes the
    class id there (asr_opm_classes_f32), so a RAW argmax stack has s_k = ids[k]; the min-max normalisation the solver's
    stacks go through takes it to 1, and the slice and slice_max stacks are activations in [0, 1]: s_k = 1."""
    ids = [int(c) for c in class_ids]
    if mode == "argmax" and not normalised:
        return [float(c) for c in ids]
    return [1.0] * len(ids)


def uncertainty_map(var_planes, nv_planes, scales):
    """How far the realigned copies disagree at each pixel, over the classes: [H, W] float32 on the planes' device.
    var_planes, nv_planes [K, H, W]: the "var" and "nv" of ops.realign_moments for the K classes' stacks; scales: K values
    s_k, the value stack k holds where its class wins (opm_scales), so that var_k / s_k^2 is comparable between classes.
    u = max over k of var_k / (s_k * s_k), in f32; a pixel where any of the planes rests on fewer than two copies (nv < 2:
    a variance of nothing) gets +inf, so a risk-coverage curve retains it last.  Classes that were pruned take no part:
    pass only the planes of the classes that were solved."""
    if var_planes.dim() != 3 or tuple(nv_planes.shape) != tuple(var_planes.shape):
        raise ValueError(f"var_planes and nv_planes must both be [K, H, W], got {tuple(var_planes.shape)} and "
                         f"{tuple(nv_planes.shape)}")
    s = np.asarray(list(scales), dtype=np.float32).reshape(-1)
    if s.size != var_planes.shape[0] or s.size == 0:
        raise ValueError(f"{s.size} scales for {var_planes.shape[0]} planes (at least one)")
    if not (np.isfinite(s).all() and (s > 0).all()):
        raise ValueError(f"scales must be finite and > 0, got {s.tolist()}")
    s2 = torch.as_tensor(s * s).to(var_planes.device).view(-1, 1, 1)
    u = (var_planes.to(torch.float32) / s2).amax(dim=0)
    thin = (nv_planes < 2).any(dim=0)
    return torch.where(thin, torch.full_like(u, float("inf")), u)


def _flat_on(t, like, dtype):
    if isinstance(t, torch.Tensor):
        return t.to(device=like, dtype=dtype).contiguous().reshape(-1)
    return torch.as_tensor(np.asarray(t).astype({torch.int32: np.int32, torch.float32: np.float32}[dtype]).reshape(-1)).to(like)


def coverage_edges(u, truth, percents, ignore_label=255):
    """The edges of a risk-coverage curve: float32 [B] on u's device, nothing read back.  u: an uncertainty map (tensor, any
    shape; no NaN), truth: a label map of as many pixels, percents: ops.check_coverages.  M is the number of counted pixels
    (truth != ignore_label; -1 or None: all of them); for percent p the edge is the k-th smallest u among them,
    k = (p * M + 99) // 100 in int64 -- the least k with k / M >= p / 100 -- found by one sort with the ignored pixels sent
    to +inf.  Keeping u <= edge retains every pixel tied with the k-th, so the retained share is >= p %, and an edge of +inf
    (uncertainty_map's "nobody knows") retains everything.  M = 0 gives +inf edges."""
    ps = ops.check_coverages(percents)
    uu = u.to(torch.float32).contiguous().reshape(-1)
    t = _flat_on(truth, uu.device, torch.int32)
    if t.numel() != uu.numel() or uu.numel() == 0:
        raise ValueError(f"expected {uu.numel()} ground-truth pixels (at least one), got {t.numel()}")
    inf = torch.full_like(uu, float("inf"))
    ignore = -1 if ignore_label is None else int(ignore_label)
    counted = (t != ignore) if ignore != -1 else torch.ones_like(t, dtype=torch.bool)
    m = counted.sum(dtype=torch.int64)
    s = torch.sort(torch.where(counted, uu, inf)).values
    p = torch.as_tensor(ps, dtype=torch.int64).to(uu.device)
    k = (p * m + 99) // 100
    e = s[torch.clamp(k - 1, 0, uu.numel() - 1)]
    return torch.where(m > 0, e, torch.full_like(e, float("inf")))


def coverage_retained(u, truth, edges, ignore_label=255):
    """int64 [B + 1] on u's device: the counted pixels (truth != ignore_label) with u <= edges[b], then M, all of them."""
    uu = u.to(torch.float32).contiguous().reshape(-1)
    t = _flat_on(truth, uu.device, torch.int32)
    ignore = -1 if ignore_label is None else int(ignore_label)
    counted = (t != ignore) if ignore != -1 else torch.ones_like(t, dtype=torch.bool)
    kept = (counted[None] & (uu[None] <= edges.view(-1, 1))).sum(dim=1, dtype=torch.int64)
    return torch.cat([kept, counted.sum(dtype=torch.int64).view(1)])


def risk_coverage_counts(y_true, y_pred, u, percents, ignore_label=255, return_share=False):
    """The per-label counts of one prediction over its p % most certain pixels, for each p of percents: host int64
    [B, 3, 256], row b what ops.class_counts counts over the pixels with u <= coverage_edges(...)[b] whose truth is not
    ignore_label.  u: an uncertainty map of as many pixels (utils.uncertainty_map); numpy arrays or tensors.  With
    return_share also float64 [B]: the share of the counted pixels each row retained (>= p / 100: ties stay in)."""
    dev = _lib.require_gpu()
    t = _as_label_tensor(y_true, dev)
    p = _as_label_tensor(y_pred, dev)
    uu = _flat_on(u, dev, torch.float32)
    if p.numel() != t.numel() or uu.numel() != t.numel():
        raise ValueError(f"expected {t.numel()} pixels, got {p.numel()} predicted and {uu.numel()} of u")
    edges = coverage_edges(uu, t, percents, ignore_label=ignore_label)
    counts = ops.binned_class_counts(t, p, uu, edges, ignore_label=ignore_label)[0].cpu().numpy()
    if not return_share:
        return counts
    kept = coverage_retained(uu, t, edges, ignore_label=ignore_label).cpu().numpy()
    with np.errstate(divide="ignore", invalid="ignore"):
        return counts, np.float64(kept[:-1]) / np.float64(kept[-1])


def risk_coverage_mIoU(y_true, y_pred, u, percents, ignore_label=255):
    """float64 [B]: Mean_IOU of the prediction over its p % most certain pixels (mean_iou_from_counts of
    risk_coverage_counts).  A curve that rises as p falls says u knows where the prediction is wrong."""
    counts = risk_coverage_counts(y_true, y_pred, u, percents, ignore_label=ignore_label)
    return np.array([mean_iou_from_counts(c) for c in counts], dtype=np.float64)


def compute_IoU(true_image, image, img_size=(512, 512), class_id=None, include_bg=False):
    """IoU of two label maps (utils.py:207-230): single class (optionally with background) when class_id is given,
    otherwise the multi-class Mean_IOU.  Void (255) pixels are NOT excluded from the single-class form, exactly
    like the reference."""
    n = img_size[0] * img_size[1]
    size = lambda a: a.numel() if isinstance(a, torch.Tensor) else np.asarray(a).size
    if size(true_image) != n or size(image) != n:
        raise ValueError(f"expected {n} pixels, got {size(true_image)} and {size(image)}")
    if class_id is None:
        return Mean_IOU(true_image, image)
    return single_class_IOU(true_image, image, class_id, include_bg)
