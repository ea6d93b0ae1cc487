"""The convergence monitor of include/asr_hip.h ("convergence monitor") restated in numpy float64: the stop rule, the scalar
loss, and the float32 summands of the four loss terms (what the device accumulates, in whatever order).  TEST INFRASTRUCTURE
ONLY."""
import math

import numpy as np

from oracle.sr import btv_weight


def scalar_loss(terms, lambdas):
    """L = ((l_df*t0 + l_tv*t1) + l_L2*t2), then + l_L1*t3 only when l_L1 > 0: float64, every operation rounding by itself, the
    lambdas the float32 values widened.  terms [..., 4] -> [...]."""
    t = np.asarray(terms, dtype=np.float64)
    l = [np.float64(np.float32(v)) for v in lambdas]
    loss = (l[0] * t[..., 0] + l[1] * t[..., 1]) + l[2] * t[..., 2]
    if l[3] > 0.0:
        loss = loss + l[3] * t[..., 3]
    return loss


def stop_iterations(losses, every, rel_tol, patience, min_iter, num_iter=None):
    """losses [E] (one image) or [E, B]: the loss at evaluation e, that of iteration e * every; rows after an image's stop are
    not read.  -> iters_done, an int or an int array [B]: the iteration of the first evaluation with stall >= patience >= 1
    and iteration >= min_iter, or num_iter (default: as many iterations as the E evaluations can cover, E * every) when
    the image never stops."""
    a = np.asarray(losses, dtype=np.float64)
    if a.ndim == 1:
        return int(stop_iterations(a[:, None], every, rel_tol, patience, min_iter, num_iter)[0])
    E, B = a.shape
    num_iter = E * every if num_iter is None else int(num_iter)
    out = np.full(B, num_iter, dtype=np.int64)
    tol = np.float64(rel_tol)
    for b in range(B):
        best, stall = np.float64(np.inf), 0
        for e in range(E):
            it = e * every
            if it >= num_iter:
                break
            L = a[e, b]
            bar = best if best == np.inf else best - tol * abs(best)
            if L < bar:                      # False for NaN and for +inf
                best, stall = L, 0
            else:
                stall += 1
            if patience >= 1 and stall >= patience and it >= min_iter:
                out[b] = it
                break
    return out


# ---- the float32 summands of the loss terms ------------------------------------------------------------------------------------
def rho32(r, loss, delta=0.1, w=None):
    """w * rho(r) for every residual, one float32 operation per statement: r*r; |r|; Huber's tail delta * (2|r| - delta) where
    not |r| <= delta; then the weight."""
    f = np.float32
    r = np.asarray(r, dtype=np.float32)
    a = np.abs(r)
    if loss == "l1":
        rho = a
    else:
        rho = (r * r).astype(np.float32)
        if loss == "huber":
            d = f(delta)
            lin = (f(2.0) * a - d).astype(np.float32)
            rho = np.where(~(a <= d), (d * lin).astype(np.float32), rho)
    if w is not None:
        rho = (np.asarray(w, dtype=np.float32) * rho).astype(np.float32)
    return rho.astype(np.float32)


def _forward_diffs(x):
    x = np.asarray(x, dtype=np.float32)
    dy = np.zeros_like(x)
    dx = np.zeros_like(x)
    dy[:-1, :] = x[1:, :] - x[:-1, :]
    dx[:, :-1] = x[:, 1:] - x[:, :-1]
    return dy, dx


def tv_summands(x, wy=None, wx=None):
    """One float32 summand per pixel: |dy| + |dx|, or wy*|dy| + wx*|dx| (products and sum in float32)."""
    dy, dx = _forward_diffs(x)
    if wy is None:
        return (np.abs(dy) + np.abs(dx)).astype(np.float32)
    wy, wx = np.asarray(wy, dtype=np.float32), np.asarray(wx, dtype=np.float32)
    return ((wy * np.abs(dy)).astype(np.float32) + (wx * np.abs(dx)).astype(np.float32)).astype(np.float32)


def btv_summands(x, alpha, shift):
    """One float64 summand per pixel and pair (h, v), h in [-s, s], v in [0, s]: float32 alpha^(|h|+v) (oracle.sr.btv_weight) times
    the float32 |x(q) - x(q - p)| (zero outside), the product of the two in float64, which is exact."""
    x = np.asarray(x, dtype=np.float32)
    H, W = x.shape
    out = []
    for hh in range(-shift, shift + 1):
        for vv in range(0, shift + 1):
            wgt = btv_weight(alpha, hh, vv)             # the correctly rounded float32 power (numpy's own can be 1 ulp off)
            sv = np.zeros_like(x)
            ys, xs = slice(vv, H), slice(max(hh, 0), W + min(hh, 0))
            yq, xq = slice(0, H - vv), slice(max(-hh, 0), W - max(hh, 0))
            sv[ys, xs] = x[yq, xq]                      # sv(Y, X) = x(Y - vv, X - hh)
            out.append(np.float64(wgt) * np.abs(x - sv).astype(np.float32).astype(np.float64))
    return np.stack(out)


def l2_summands(x):
    x = np.asarray(x, dtype=np.float32)
    return (x * x).astype(np.float32)


def l1_summands(x):
    return np.abs(np.asarray(x, dtype=np.float32))


def exact_sum(summands):
    """(math.fsum of the summands as float64, their count)."""
    a = np.asarray(summands).astype(np.float64).ravel()
    return math.fsum(a.tolist()), a.size
