"""The primal-dual update rule and the step bound of include/asr_hip.h ("primal-dual"), restated in numpy float32 on top of
oracle.sr.  TEST INFRASTRUCTURE ONLY.  The forward model and the registered-gradient data term are the oracle's own
(forward_model_tf, data_grad_copies_tf through tests/sr_dt_ref.DataTermSuperresolution, summed in copy order as
loss_and_grad_tf does); only the statements after the data-term gradient are new, one float32 operation per statement."""
import numpy as np
import torch

from oracle import sr as o_sr
from oracle import tf_ops

import sr_dt_ref as RD

F = np.float32
DUAL_RATIO = F(1.0 / 16.0)


def make_sr(lambdas, n, hw, HW, df_loss="l2", df_delta=0.1, weights=None):
    """The oracle object the restatement runs on: lambdas (df, tv, l2, l1), n copies of hw seen from HW."""
    return RD.DataTermSuperresolution(*[float(v) for v in lambdas], num_aug=n, feature_size=tuple(hw), output_size=tuple(HW),
                                      df_loss=df_loss, df_delta=df_delta, weights=weights)


def transforms(angles, shifts, HW):
    """(rot, trans, inv_rot, inv_trans) [n, 8] as the oracle builds them from angles and shifts."""
    rot = tf_ops.angles_to_projective_transforms(np.asarray(angles, dtype=np.float32), HW[0], HW[1])
    tr = tf_ops.translations_to_projective_transforms(np.asarray(shifts, dtype=np.float32))
    return rot, tr, tf_ops.invert_transforms(rot), tf_ops.invert_transforms(tr)


def data_grad(sr, x, samples, tfs):
    """g_df [H, W]: what the gather kernel hands the update.  x [H, W], samples [n, h, w], tfs = transforms(...)."""
    rot, tr, irot, itr = tfs
    target = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)[None, :, :, None])
    smp = torch.from_numpy(np.ascontiguousarray(samples, dtype=np.float32)[..., None])
    resid = sr.forward_model_tf(target, rot, tr) - smp
    g_x = sr.data_grad_copies_tf(resid, irot, itr)
    g_df = torch.zeros_like(target)
    for i in range(g_x.shape[0]):                       # fixed order n = 0..N-1
        g_df[0] += g_x[i]
    return g_df.numpy()[0, :, :, 0].copy()


def pd_step(sr, x, py, px, samples, tfs, tau, dual_ratio=DUAL_RATIO, wy=None, wx=None):
    """One iteration of ASR_OPT_PRIMAL_DUAL -> (x', py', px', g).  Everything is read from the old x, py, px."""
    return pd_update(sr, x, py, px, data_grad(sr, x, samples, tfs), tau, dual_ratio, wy, wx)


def pd_update(sr, x, py, px, g_df, tau, dual_ratio=DUAL_RATIO, wy=None, wx=None):
    """The statements of the rule after the data-term gradient g_df [H, W] -> (x', py', px', g)."""
    x, py, px, g_df = (np.asarray(a, dtype=np.float32) for a in (x, py, px, g_df))
    tau = F(tau)
    sigma = F(F(dual_ratio) / tau)
    lam_tv, two_l2, lam_l1 = F(sr.lambda_tv), F(F(2.0) * F(sr.lambda_L2)), F(sr.lambda_L1)
    dY = np.zeros_like(x)
    dX = np.zeros_like(x)
    dY[:-1] = x[1:] - x[:-1]
    dX[:, :-1] = x[:, 1:] - x[:, :-1]
    by = np.full_like(x, lam_tv) if wy is None else (lam_tv * np.asarray(wy, dtype=np.float32)).astype(np.float32)
    bx = np.full_like(x, lam_tv) if wx is None else (lam_tv * np.asarray(wx, dtype=np.float32)).astype(np.float32)
    py1 = np.minimum(np.maximum(py + sigma * dY, -by), by).astype(np.float32)
    px1 = np.minimum(np.maximum(px + sigma * dX, -bx), bx).astype(np.float32)
    qy = (F(2.0) * py1 - py).astype(np.float32)
    qx = (F(2.0) * px1 - px).astype(np.float32)
    div = (-qy - qx).astype(np.float32)
    div[1:] += qy[:-1]
    div[:, 1:] += qx[:, :-1]
    g = ((g_df + div) + two_l2 * x).astype(np.float32)
    u = (x - g * tau).astype(np.float32)
    if lam_l1 > 0:
        t = F(tau * lam_l1)
        u = np.where(u > t, u - t, np.where(u < -t, u + t, F(0.0))).astype(np.float32)
    assert u.dtype == py1.dtype == px1.dtype == g.dtype == np.float32
    return u, py1, px1, g


def pd_solve(sr, x0, samples, tfs, taus, dual_ratio=DUAL_RATIO, wy=None, wx=None, trajectory=False):
    """len(taus) iterations from x0 with zero duals -> (x, py, px) or, with trajectory, the list of them after each one."""
    x = np.asarray(x0, dtype=np.float32).copy()
    py, px = np.zeros_like(x), np.zeros_like(x)
    traj = []
    for tau in taus:
        x, py, px, _ = pd_step(sr, x, py, px, samples, tfs, tau, dual_ratio, wy, wx)
        traj.append((x, py, px))
    return traj if trajectory else (x, py, px)


def apply_m(sr, v, tfs):
    """M v: the data-term gradient at x = v for measurements y = 0 under L2 (with the object's weights)."""
    assert sr.df_loss == "l2"
    n = len(tfs[0])
    return data_grad(sr, v, np.zeros((n,) + tuple(sr.feature_size), np.float32), tfs)


def data_bound(sr, tfs, iters=6, all_iters=False):
    """The Collatz-Wielandt bound of asr_sr_data_bound_f32 for one image, float32 (all_iters: after 1 .. iters repetitions)."""
    H, W = sr.output_size
    v = np.ones((H, W), np.float32)
    out, B = [], F(0.0)
    for _ in range(iters):
        w = apply_m(sr, v, tfs)
        pos = v > 0
        B = F((w[pos] / v[pos]).max()) if pos.any() else F(0.0)
        s = F(w.max())
        out.append(B)
        if not s > 0:
            out += [B] * (iters - len(out))
            break
        v = (w / s).astype(np.float32)
    return out if all_iters else B


def pd_tau(bound, lambda_l2):
    """tau = 1 / (bound + 2 lambda_l2) in float32, 0 where the denominator is 0 (ops.pd_steps)."""
    den = F(F(bound) + F(2.0) * F(lambda_l2))
    return F(1.0) / den if den != 0 else F(0.0)


def case_problem(case):
    """tests/sr_dt_ref.make_case's dict -> (sr factory arguments, samples [n,h,w], tfs, x0 [H,W]): the start is the resize of
    copy 0, as augmented_superresolution takes it."""
    h = case["copies"].shape[-1]
    H = case["truth"].shape[-1]
    tfs = transforms(case["angles"], case["shifts"], (H, H))
    x0 = tf_ops.resize_bilinear(torch.from_numpy(case["copies"][0:1, :, :, None]), (H, H)).numpy()[0, :, :, 0].copy()
    return (len(case["copies"]), (h, h), (H, H)), case["copies"], tfs, x0


def scalar_loss(lambdas, case, x):
    """The reference's scalar loss of x on a case (oracle.sr.Superresolution.loss_function)."""
    n, hw, HW = case_problem(case)[0]
    sr = o_sr.Superresolution(*[float(v) for v in lambdas], num_aug=n, feature_size=hw, output_size=HW)
    return sr.loss_function(np.asarray(x, dtype=np.float32).reshape(1, *HW, 1), case["copies"][..., None], case["angles"],
                            case["shifts"])
