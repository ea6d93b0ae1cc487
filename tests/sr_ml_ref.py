"""The multi-label coupling of include/asr_hip.h ("multi-label coupling") restated in numpy float32: the projection rule, the
threshold-free fusion rule, the group stop rule, and a coupled primal-dual solve on top of tests/sr_pd_ref.py (step every
member, then project).  TEST INFRASTRUCTURE ONLY.  Every operation rounds by itself; sums run in explicit loops in index order,
never np.sum."""
import numpy as np

import sr_pd_ref as P

F = np.float32


def simplex_project(v):
    """v [G, ...] float32 -> the rule applied to the G values of every pixel, statement for statement."""
    v = np.asarray(v, dtype=np.float32)
    G = v.shape[0]
    a = np.where(v > 0, v, F(0.0)).astype(np.float32)
    s = a[0].copy()
    for j in range(1, G):
        s = (s + a[j]).astype(np.float32)
    over = s > F(1.0)
    u = -np.sort(-a, axis=0)                                   # descending; equal values are interchangeable
    c = np.zeros_like(s)
    theta = np.zeros_like(s)
    for k in range(1, G + 1):
        c = (c + u[k - 1]).astype(np.float32)
        t = ((c - F(1.0)) / F(k)).astype(np.float32)
        theta = np.where(u[k - 1] > t, t, theta).astype(np.float32)
    shrunk = np.where(a > theta[None], (a - theta[None]).astype(np.float32), F(0.0)).astype(np.float32)
    out = np.where(over[None], shrunk, a).astype(np.float32)
    assert out.dtype == np.float32
    return out


def project_groups(x, group):
    """x [B, ...] with B a multiple of group: the rule on every run of `group` consecutive planes."""
    x = np.asarray(x, dtype=np.float32)
    assert x.shape[0] % group == 0
    return np.concatenate([simplex_project(x[g:g + group]) for g in range(0, x.shape[0], group)], axis=0)


def exact_projection(v):
    """The Euclidean projection of each pixel's G values onto {x >= 0, sum x <= 1} in float64 (the sort-based algorithm)."""
    v = np.asarray(v, dtype=np.float64)
    G = v.shape[0]
    a = np.maximum(v, 0.0)
    over = a.sum(axis=0) > 1.0
    u = -np.sort(-a, axis=0)
    css = np.cumsum(u, axis=0) - 1.0
    ks = np.arange(1, G + 1, dtype=np.float64).reshape((G,) + (1,) * (v.ndim - 1))
    cond = u - css / ks > 0
    rho = G - 1 - np.argmax(cond[::-1], axis=0)                # the last k that holds
    theta = np.take_along_axis(css, rho[None], axis=0)[0] / (rho + 1.0)
    return np.where(over[None], np.maximum(a - theta[None], 0.0), a)


def fuse_labels_simplex(scores, ids):
    """scores [K, ...] float32, ids [K] -> int32 labels: the first class of greatest share where it beats bg = 1 - sum."""
    scores = np.asarray(scores, dtype=np.float32)
    s = scores[0].copy()
    for k in range(1, scores.shape[0]):
        s = (s + scores[k]).astype(np.float32)
    bg = (F(1.0) - s).astype(np.float32)
    best = scores[0].copy()
    lab = np.full(best.shape, int(ids[0]), np.int32)
    for k in range(1, scores.shape[0]):
        better = scores[k] > best
        best = np.where(better, scores[k], best)
        lab = np.where(better, np.int32(ids[k]), lab)
    return np.where(best > bg, lab, np.int32(0)).astype(np.int32)


def group_stop(losses, rel_tol, patience, every=1, min_iter=0):
    """The stop rule on a group: losses [E][G] float64, the members' scalar losses at the evaluations it = 0, every, ...
    -> the iteration at which the group stops, or None.  The group's loss is the members' added in index order."""
    best, stall = np.inf, 0
    for e, row in enumerate(losses):
        it = e * every
        loss = np.float64(row[0])
        for v in row[1:]:
            loss = loss + np.float64(v)
        bar = best if best == np.inf else best - np.float64(rel_tol) * abs(best)
        if loss < bar:
            best, stall = loss, 0
        else:
            stall += 1
        if patience >= 1 and stall >= patience and it >= min_iter:
            return it
    return None


def pd_solve(srs, x0, samples, tfs, taus, group, dual_ratio=P.DUAL_RATIO, wy=None, wx=None, trajectory=False):
    """The coupled solve of a batch of B = len(srs) planes in groups of `group`: every iteration steps each member by
    sr_pd_ref.pd_step from the old x and duals, then projects the new x group by group.  taus [iters, B].  -> (x, py, px)
    [B, H, W] each, or with trajectory the list of them after every iteration."""
    B = len(srs)
    x = np.asarray(x0, dtype=np.float32).copy()
    py, px = np.zeros_like(x), np.zeros_like(x)
    traj = []
    for row in taus:
        new = [P.pd_step(srs[i], x[i], py[i], px[i], samples[i], tfs[i], row[i], dual_ratio, None if wy is None else wy[i],
                         None if wx is None else wx[i]) for i in range(B)]
        x = project_groups(np.stack([s[0] for s in new]), group)
        py, px = np.stack([s[1] for s in new]), np.stack([s[2] for s in new])
        traj.append((x, py, px))
    return traj if trajectory else (x, py, px)
