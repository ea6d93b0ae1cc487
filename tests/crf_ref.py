"""The windowed CRF of include/asr_hip.h ("windowed CRF") restated in numpy, written from the rule and never from the library:
shifted slices for the clipped, dilated window, every step in one dtype (float64 is the yardstick; the same code in float32
gives the error scale e32).  Shared by the CRF tests; nothing here touches a GPU."""
import numpy as np

DEFAULTS = dict(radius=3, dilation=1, iterations=5, w_app=4.0, w_smooth=1.0, theta_pos=2.0, theta_rgb=0.1, theta_smooth=1.0)


def softmax(s):
    """Over axis 0, the maximum subtracted first, in s's dtype."""
    e = np.exp(s - s.max(axis=0))
    return e / e.sum(axis=0, dtype=s.dtype)


def _window(guide, cfg, dtype):
    """Per offset in ascending (dy, dx) order: (destination slices, source slices, a [h, w], g scalar) of the pixels whose
    neighbour at that offset lies inside the image."""
    H, W = guide.shape[:2]
    r, d = cfg["radius"], cfg["dilation"]
    two = dtype(2)
    tp, tr, ts = (dtype(np.float32(cfg[k])) for k in ("theta_pos", "theta_rgb", "theta_smooth"))
    out = []
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            oy, ox = d * dy, d * dx
            y0, y1, x0, x1 = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
            if (dy == 0 and dx == 0) or y1 <= y0 or x1 <= x0:
                continue
            dst, src = (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
            delta2 = dtype(oy * oy + ox * ox)
            diff2 = ((guide[dst] - guide[src]) ** 2).sum(axis=-1, dtype=dtype)
            a = np.exp(np.maximum(-delta2 / (two * tp * tp) - diff2 / (two * tr * tr), dtype(-80)))
            g = np.exp(np.maximum(-delta2 / (two * ts * ts), dtype(-80)))
            out.append((dst, src, a.astype(dtype), dtype(g)))
    return out


def crf(guide, z, dtype=np.float64, **params):
    """guide [H, W, 3], z [L, H, W] -> (final logits s [L, H, W], Q^T [L, H, W]), every step in `dtype`.  argmax_l of s (first
    maximum) is the label index.  params: fields of DEFAULTS."""
    cfg = dict(DEFAULTS, **params)
    guide, z = np.asarray(guide).astype(dtype), np.asarray(z).astype(dtype)
    L, H, W = z.shape
    w_app, w_smooth = dtype(np.float32(cfg["w_app"])), dtype(np.float32(cfg["w_smooth"]))
    window = _window(guide, cfg, dtype)
    s, Q = z, softmax(z)
    for _ in range(cfg["iterations"]):
        A, G = np.zeros((L, H, W), dtype), np.zeros((L, H, W), dtype)
        na, ng = np.zeros((H, W), dtype), np.zeros((H, W), dtype)
        for dst, src, a, g in window:
            qn = Q[(slice(None),) + src]
            A[(slice(None),) + dst] += a * qn
            G[(slice(None),) + dst] += g * qn
            na[dst] += a
            ng[dst] += g
        with np.errstate(divide="ignore", invalid="ignore"):
            app = np.where(na > 0, A / na, dtype(0))          # a pixel without neighbours (the 1 x 1 image): both terms 0
            smo = np.where(ng > 0, G / ng, dtype(0))
        s = (z + w_app * app + w_smooth * smo).astype(dtype)
        Q = softmax(s)
    assert s.dtype == dtype and Q.dtype == dtype
    return s, Q


def labels_of(s, ids):
    """The label map of logits s [L, H, W]: ids[l - 1] for the first maximum l >= 1, 0 for l = 0."""
    table = np.concatenate([[0], np.asarray(ids, dtype=np.int32)]).astype(np.int32)
    return table[np.argmax(s, axis=0)]


def top_two_margin(s):
    """The gap between the greatest and the second greatest logit, [H, W]."""
    top = np.sort(s, axis=0)
    return top[-1] - top[-2]


def unaries_scores(scores, th_factor, tau):
    """asr_crf_unaries_scores_f32 in numpy float32: z_0 = 0, z_{k+1} = (S_k - max(S_k) * th_factor) / tau."""
    scores = np.asarray(scores, dtype=np.float32)
    K = scores.shape[0]
    z = np.zeros((K + 1,) + scores.shape[1:], dtype=np.float32)
    for k in range(K):
        t = np.float32(scores[k].max()) * np.float32(th_factor)
        z[k + 1] = (scores[k] - t) / np.float32(tau)
    assert z.dtype == np.float32
    return z


def unaries_labels(labels, ids, conf):
    """asr_crf_unaries_labels_f32 in numpy: the two logarithms in double of the float32 conf, rounded once."""
    labels = np.asarray(labels)
    L = len(ids) + 1
    c = np.float64(np.float32(conf))
    hit, miss = np.float32(np.log(c)), np.float32(np.log((1.0 - c) / (L - 1)))
    z = np.zeros((L,) + labels.shape, dtype=np.float32)
    for l, v in enumerate([0] + list(ids)):
        at = labels == v
        z[:, at] = miss
        z[l, at] = hit
    return z
