"""The data term of include/asr_hip.h ("data term": L1, Huber, per-measurement weights), restated in plain numpy / torch on top of
oracle.sr.  TEST INFRASTRUCTURE ONLY: the oracle itself stays what it is; the subclass below hands data_grad_copies_tf
q = w * psi(r) where the oracle hands it r, so that L2 without weights is the oracle's own arithmetic bit for bit
(test_sr_dt_host.py).  Also the synthetic construction on which the three losses are compared: a rotated rectangle seen
through the oracle's own forward model, a quarter of the copies replaced by a disc somewhere else."""
import numpy as np
import torch

from oracle import sr as o_sr

LOSSES = ("l2", "l1", "huber")


def psi(r, loss, delta=0.1):
    """psi = rho' / 2 on a float32 array, one float32 operation per statement; sgn(+-0) = +0 under L1."""
    r = np.asarray(r, dtype=np.float32)
    f = np.float32
    if loss == "l2":
        return r
    if loss == "l1":
        return np.where(r > 0, f(0.5), np.where(r < 0, f(-0.5), f(0.0))).astype(np.float32)
    assert loss == "huber" and np.isfinite(delta) and delta > 0
    d = f(delta)
    return np.where(r < -d, -d, np.where(r > d, d, r)).astype(np.float32)


def weighted_psi(r, loss, delta=0.1, w=None):
    """q = w * psi(r): ONE float32 multiply, left out without weights."""
    q = psi(r, loss, delta)
    return q if w is None else (np.asarray(w, dtype=np.float32) * q).astype(np.float32)


def rho64(r, loss, delta=0.1):
    """rho in float64, from the float32 residual and the float32 delta."""
    r = np.asarray(r, dtype=np.float32).astype(np.float64)
    if loss == "l2":
        return r * r
    if loss == "l1":
        return np.abs(r)
    d = float(np.float32(delta))
    a = np.abs(r)
    return np.where(a <= d, r * r, d * (2.0 * a - d))


def data_term64(r, loss, delta=0.1, w=None):
    """sum w * rho(r) in float64."""
    t = rho64(r, loss, delta)
    if w is not None:
        t = np.asarray(w, dtype=np.float32).astype(np.float64) * t
    return float(t.sum())


class DataTermSuperresolution(o_sr.Superresolution):
    """oracle.sr.Superresolution under the data term sum w * rho(r).  weights: None or float32 [num_aug, h, w]; under
    copy_dropout they lose the copies the oracle's frozen mask drops."""

    def __init__(self, *args, df_loss="l2", df_delta=0.1, weights=None, **kw):
        super().__init__(*args, **kw)
        assert df_loss in LOSSES
        self.df_loss, self.df_delta = df_loss, df_delta
        self.weights = None if weights is None else np.ascontiguousarray(weights, dtype=np.float32)

    def _weights_for(self, n):
        if self.weights is None or self.weights.shape[0] == n:
            return self.weights
        mask = self.drop_mask(int(self.num_aug * self.copy_dropout))
        assert int(mask.sum()) == n
        return self.weights[mask]

    def data_grad_copies_tf(self, resid, inv_rot_tf, inv_trans_tf):
        w = self._weights_for(resid.shape[0])
        if self.df_loss == "l2" and w is None:
            return super().data_grad_copies_tf(resid, inv_rot_tf, inv_trans_tf)
        q = weighted_psi(resid.numpy(), self.df_loss, self.df_delta, None if w is None else w[..., None])
        return super().data_grad_copies_tf(torch.from_numpy(np.ascontiguousarray(q)), inv_rot_tf, inv_trans_tf)

    def loss_terms_tf(self, target, samples, rot_tf, trans_tf):
        resid, dy, dx, df, tv, l2, l1 = super().loss_terms_tf(target, samples, rot_tf, trans_tf)
        w = self._weights_for(resid.shape[0])
        if not (self.df_loss == "l2" and w is None):
            df = torch.tensor(data_term64(resid.numpy(), self.df_loss, self.df_delta, None if w is None else w[..., None]),
                              dtype=torch.float32)
        return resid, dy, dx, df, tv, l2, l1


# ---- the construction -----------------------------------------------------------------------------------------------------
H_HR, H_LR, N_COPIES, N_BAD = 64, 16, 20, 5
ITERS, LR, LAMBDAS = 150, 1e-2, (1.0, 0.05, 0.0, 0.0)


def make_case(seed, H=H_HR, h=H_LR, n=N_COPIES, n_bad=N_BAD):
    """-> dict(truth [H,H] {0,1}, copies [n,h,h] {0,1}, angles [n], shifts [n,2], bad: the replaced copies).
    A rotated rectangle (centre in [0.4, 0.6] H, half-sizes 0.22 H x 0.12 H); n copies at h^2 from the oracle's forward model
    (angles +-0.3 rad, shifts +-0.12 H; copy 0 is the un-augmented view), binarised at 0.5; n_bad copies other than copy 0
    replaced by a disc of radius 0.22 h at a random place."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:H].astype(np.float64)
    cy, cx = H * rng.uniform(0.4, 0.6), H * rng.uniform(0.4, 0.6)
    th = rng.uniform(0.0, np.pi)
    u = (xx - cx) * np.cos(th) + (yy - cy) * np.sin(th)
    v = -(xx - cx) * np.sin(th) + (yy - cy) * np.cos(th)
    truth = ((np.abs(u) <= 0.22 * H) & (np.abs(v) <= 0.12 * H)).astype(np.float32)
    angles = rng.uniform(-0.3, 0.3, n).astype(np.float32)
    shifts = rng.uniform(-0.12 * H, 0.12 * H, (n, 2)).astype(np.float32)
    angles[0] = 0
    shifts[0] = 0
    sr = o_sr.Superresolution(1, 0, 0, 0, num_aug=n, feature_size=(h, h), output_size=(H, H))
    lr = sr.forward_model(torch.from_numpy(truth[None, :, :, None]), angles, shifts).numpy()[..., 0]
    copies = (lr > 0.5).astype(np.float32)
    bad = np.sort(rng.choice(np.arange(1, n), size=n_bad, replace=False))
    ly, lx = np.mgrid[0:h, 0:h].astype(np.float64)
    for i in bad:
        dy, dx = rng.uniform(0, h), rng.uniform(0, h)
        copies[i] = (((ly - dy) ** 2 + (lx - dx) ** 2) <= (0.22 * h) ** 2).astype(np.float32)
    return dict(truth=truth, copies=copies, angles=angles, shifts=shifts, bad=bad)


def iou(x, truth):
    """IoU of x > 0.5 * max x against the truth."""
    x = np.asarray(x, dtype=np.float32).reshape(truth.shape)
    m = x > np.float32(0.5) * x.max()
    t = truth > 0.5
    return float((m & t).sum()) / float(max((m | t).sum(), 1))


def solve_case(case, df_loss, df_delta=0.1, iters=ITERS, weights=None):
    """The construction solved on the CPU by the restatement: AMSGrad, lr 1e-2, lambda = (1, 0.05, 0, 0) -> x [H,H]."""
    h = case["copies"].shape[-1]
    H = case["truth"].shape[-1]
    opt = o_sr.Optimizer("adam", LR, amsgrad=True)
    sr = DataTermSuperresolution(*LAMBDAS, num_iter=iters, num_aug=len(case["copies"]), optimizer=opt, feature_size=(h, h),
                                 output_size=(H, H), df_loss=df_loss, df_delta=df_delta, weights=weights)
    x, _ = sr.augmented_superresolution(case["copies"][..., None], case["angles"], case["shifts"])
    return x[:, :, 0]
