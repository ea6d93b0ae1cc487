"""A numpy restatement of the "regions" definitions of include/asr_hip.h, written from the definitions and not from the kernels:
no tiles, no union-find forest, no atomics.

Labelling: every pixel starts with its own linear index; a pixel takes the smallest label among itself and its equal-valued
c-neighbours, hands that label to the pixel its old label named (so that a whole group drops at once, not one step per round),
and labels are then chased (L = L[L]) until they stop moving; repeated until nothing changes.  A label is always the index of a
pixel of the same region and never rises, so the fixed point holds, at every pixel, the smallest index of its region."""
import numpy as np

OFFSETS = {4: ((0, 1), (1, 0)), 8: ((0, 1), (1, 0), (1, 1), (1, -1))}              # (dy, dx), one of each opposite pair


def _pairs(h, w, c):
    """The c-adjacent pixel pairs inside an [h, w] image as two index arrays (each unordered pair once)."""
    idx = np.arange(h * w, dtype=np.int64).reshape(h, w)
    a, b = [], []
    for dy, dx in OFFSETS[c]:
        if dx >= 0:
            p, q = idx[:h - dy, :w - dx], idx[dy:, dx:]
        else:
            p, q = idx[:h - dy, -dx:], idx[dy:, :w + dx]
        a.append(p.ravel())
        b.append(q.ravel())
    return np.concatenate(a), np.concatenate(b)


def label_regions(labels, connectivity=4):
    """labels [h, w] -> (root, area) int32 [h, w]."""
    labels = np.asarray(labels)
    h, w = labels.shape
    flat = labels.ravel()
    a, b = _pairs(h, w, connectivity)
    same = flat[a] == flat[b]
    a, b = a[same], b[same]
    L = np.arange(h * w, dtype=np.int64)
    while True:
        m = L.copy()
        np.minimum.at(m, a, L[b])
        np.minimum.at(m, b, L[a])
        if np.array_equal(m, L):
            break
        np.minimum.at(m, L, m.copy())              # the pixel my label named learns what I learnt
        L = m
        while True:
            nxt = L[L]
            if np.array_equal(nxt, L):
                break
            L = nxt
    area = np.bincount(L, minlength=h * w)[L]
    return L.astype(np.int32).reshape(h, w), area.astype(np.int32).reshape(h, w)


def clean_labels(labels, min_area, connectivity=4, regions=None):
    """labels [h, w] -> (out int32 [h, w], stats int64 [4]), straight from the definition: per small region the set of the
    values of its adjacent pixels that lie in regions that are not small.  regions: label_regions(labels, connectivity), when
    the caller has it already."""
    labels = np.asarray(labels).astype(np.int32)
    h, w = labels.shape
    root, area = label_regions(labels, connectivity) if regions is None else regions
    r, ar, v = root.ravel().astype(np.int64), area.ravel().astype(np.int64), labels.ravel()
    a, b = _pairs(h, w, connectivity)
    a, b = np.concatenate([a, b]), np.concatenate([b, a])                         # ordered: q = b is a neighbour of p = a
    votes = (ar[a] < min_area) & (r[a] != r[b]) & (ar[b] >= min_area)
    surround = {}
    for region, value in zip(r[a][votes].tolist(), v[b][votes].tolist()):
        surround.setdefault(region, set()).add(value)
    out = v.copy()
    for p in np.nonzero(ar < min_area)[0].tolist():
        s = surround.get(int(r[p]), ())
        out[p] = next(iter(s)) if len(s) == 1 else 0
    is_root = r == np.arange(h * w)
    stats = np.array([is_root.sum(), (is_root & (ar < min_area)).sum(), (ar < min_area).sum(), (out != v).sum()], dtype=np.int64)
    return out.reshape(h, w), stats
