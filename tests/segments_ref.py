"""A numpy restatement of the "segments" rule of include/asr_hip.h, written from the rule and not from the kernels: no tiles, no
hash table, no atomics.  Regions come from tests/regions_ref.label_regions; the intersections are the counts of np.unique over
the (truth root, predicted root) pairs of the pixels both segments hold; Q is summed in Python integers."""
import numpy as np

import regions_ref as R

IOU_ONE = 1 << 30


def segment_match(truth, pred, num_labels=21, connectivity=8, include_zero=False, truth_regions=None, pred_regions=None):
    """truth, pred [h, w] -> (counts int64 [L, 4]: TP, FP, FN, Q per label; pred_match, truth_match int32 [h, w])."""
    T, P = np.asarray(truth).astype(np.int64), np.asarray(pred).astype(np.int64)
    h, w = T.shape
    n, L, v0 = h * w, int(num_labels), 0 if include_zero else 1
    t_root, t_area = R.label_regions(truth, connectivity) if truth_regions is None else truth_regions
    p_root = (R.label_regions(pred, connectivity) if pred_regions is None else pred_regions)[0]
    T, P = T.ravel(), P.ravel()
    t_root, t_area, p_root = (np.asarray(a).ravel().astype(np.int64) for a in (t_root, t_area, p_root))
    not_void = (T >= 0) & (T < L)
    seg_t, seg_p = (T >= v0) & (T < L), (P >= v0) & (P < L)
    a_p = np.bincount(p_root[seg_p & not_void], minlength=n)                       # by predicted root; void taken out
    both = seg_t & seg_p
    keys, inter = np.unique(t_root[both] * n + p_root[both], return_counts=True)
    counts = [[0, 0, 0, 0] for _ in range(L)]
    t_partner, p_partner = np.full(n, -1, np.int64), np.full(n, -1, np.int64)     # by root
    for key, i in zip(keys.tolist(), inter.tolist()):
        g, p = divmod(key, n)
        if T[g] != P[p]:
            continue
        a_g, ap = int(t_area[g]), int(a_p[p])
        if 3 * i > a_g + ap:
            assert t_partner[g] == -1 and p_partner[p] == -1, "a segment in two matches"
            t_partner[g], p_partner[p] = p, g
            counts[int(T[g])][0] += 1
            counts[int(T[g])][3] += (i * IOU_ONE) // (a_g + ap - i)
    idx = np.arange(n)
    for g in idx[seg_t & (t_root == idx) & (t_partner == -1)].tolist():
        counts[int(T[g])][2] += 1
    kept = seg_p & (a_p[p_root] > 0)                                               # A_p = 0: dropped, counted nowhere
    for p in idx[kept & (p_root == idx) & (p_partner == -1)].tolist():
        counts[int(P[p])][1] += 1
    pred_match = np.where(kept, p_partner[p_root], -2).astype(np.int32).reshape(h, w)
    truth_match = np.where(seg_t, t_partner[t_root], -2).astype(np.int32).reshape(h, w)
    return np.array(counts, dtype=np.int64).reshape(L, 4), pred_match, truth_match


def brute_force(truth, pred, num_labels=21, connectivity=8, include_zero=False):
    """The same rule with every (truth segment, predicted segment) pair tried, segments as Python sets of pixel indices.
    Returns (counts [L, 4] as a list of Python integers, the greatest number of matches any one segment was found in)."""
    T, P = np.asarray(truth).astype(np.int64).ravel(), np.asarray(pred).astype(np.int64).ravel()
    L, v0 = int(num_labels), 0 if include_zero else 1
    t_root = R.label_regions(truth, connectivity)[0].ravel()
    p_root = R.label_regions(pred, connectivity)[0].ravel()
    void = {i for i in range(T.size) if not 0 <= T[i] < L}
    t_segs = {r: set(np.nonzero(t_root == r)[0].tolist()) for r in np.unique(t_root).tolist() if v0 <= T[r] < L}
    p_segs = {r: set(np.nonzero(p_root == r)[0].tolist()) - void for r in np.unique(p_root).tolist() if v0 <= P[r] < L}
    p_segs = {r: s for r, s in p_segs.items() if s}
    counts = [[0, 0, 0, 0] for _ in range(L)]
    hits_t, hits_p = dict.fromkeys(t_segs, 0), dict.fromkeys(p_segs, 0)
    for g, gs in t_segs.items():
        for p, ps in p_segs.items():
            i = len(gs & ps)
            if T[g] == P[p] and 3 * i > len(gs) + len(ps):
                hits_t[g] += 1
                hits_p[p] += 1
                counts[int(T[g])][0] += 1
                counts[int(T[g])][3] += (i * IOU_ONE) // (len(gs) + len(ps) - i)
    for g, k in hits_t.items():
        counts[int(T[g])][2] += k == 0
    for p, k in hits_p.items():
        counts[int(P[p])][1] += k == 0
    return counts, max(list(hits_t.values()) + list(hits_p.values()) + [0])
