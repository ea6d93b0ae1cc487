"""The exact-adjoint gather of include/asr_hip.h ("exact adjoint"), restated in numpy float32, statement for statement with the
header's rule.  TEST INFRASTRUCTURE ONLY.  The forward model, the resize gradient and the translate stage's planes G_R are the
oracle's own (oracle.sr / oracle.tf_ops, as tests/sr_pd_ref.data_grad takes them); only the rotate stage is new: where the oracle
takes one bilinear tap of G_R at R^-1 p, this sums the forward's own tap weights over the window of positions that touch p."""
import numpy as np
import torch

from oracle import sr as o_sr
from oracle import tf_ops

F = np.float32
MARGIN = F(1.0 / 64.0)
MAX_HALF = F(8.0)
MAX_SHIFT = F(16384.0)


def _map(t, x, y):
    """The forward kernels' affine map: (a0*x + a1*y) + a2, every operation float32."""
    ix = (F(t[0]) * x + F(t[1]) * y) + F(t[2])
    iy = (F(t[3]) * x + F(t[4]) * y) + F(t[5])
    assert ix.dtype == np.float32 and iy.dtype == np.float32
    return ix, iy


def _half(a, b):
    return F(F(abs(F(a)) + abs(F(b))) + MARGIN)


def _axis_weight(i, p):
    """The forward's weight of integer coordinate p when it samples at i: (f + 1) - i at the floor tap, i - f at the next, else 0."""
    f = np.floor(i)
    c = (f + F(1.0)).astype(np.float32)
    return np.where(f == p, c - i, np.where(c == p, i - f, F(0.0))).astype(np.float32)


def exact_applies(rot_tf, trans_tf, inv_rot_tf):
    """flags of asr_sr_adjoint_flags_i32 for one image: transforms [N, 8] -> 1 (exact) or 0 (registered statements)."""
    rot, tr, inv = (np.asarray(t, dtype=np.float32).reshape(-1, 8) for t in (rot_tf, trans_tf, inv_rot_tf))
    with np.errstate(invalid="ignore"):
        for r, t, i in zip(rot, tr, inv):
            pure = t[0] == 1 and t[1] == 0 and t[3] == 0 and t[4] == 1 and t[6] == 0 and t[7] == 0
            ok = (i[6] == 0 and i[7] == 0 and pure and r[6] == 0 and r[7] == 0 and _half(i[0], i[1]) <= MAX_HALF and
                  _half(i[3], i[4]) <= MAX_HALF and abs(i[2]) <= MAX_SHIFT and abs(i[5]) <= MAX_SHIFT)
            if not ok:
                return 0
    return 1


def copy_contribution(g_r, rot, inv):
    """c_n [H, W] of one copy: g_r [H, W] its plane G_R (zero outside the image), rot / inv its rot_tf / inv_rot_tf [8]."""
    g_r = np.asarray(g_r, dtype=np.float32)
    H, W = g_r.shape
    X = np.arange(W, dtype=np.float32)[None, :].repeat(H, 0)
    Y = np.arange(H, dtype=np.float32)[:, None].repeat(W, 1)
    qx, qy = _map(inv, X, Y)
    ex, ey = _half(inv[0], inv[1]), _half(inv[3], inv[4])
    lox, hix = np.ceil(qx - ex), np.floor(qx + ex)
    loy, hiy = np.ceil(qy - ey), np.floor(qy + ey)
    nx = int(np.max(hix - lox)) + 1
    ny = int(np.max(hiy - loy)) + 1
    c = np.zeros((H, W), np.float32)
    for a in range(ny):                                   # y rising, then x rising
        y = (loy + F(a)).astype(np.float32)
        for k in range(nx):
            x = (lox + F(k)).astype(np.float32)
            ix, iy = _map(rot, x, y)
            wgt = (_axis_weight(iy, Y) * _axis_weight(ix, X)).astype(np.float32)
            inside = (x <= hix) & (y <= hiy) & (x >= 0) & (x < W) & (y >= 0) & (y < H)
            g = g_r[np.clip(y, 0, H - 1).astype(np.int64), np.clip(x, 0, W - 1).astype(np.int64)]
            c = np.where(inside, c + wgt * g, c).astype(np.float32)
    return c


def exact_gather(g_r, rot_tf, inv_rot_tf):
    """g_df [H, W]: the copies' contributions added in copy order from +0.  g_r [N, H, W], transforms [N, 8]."""
    g_r = np.asarray(g_r, dtype=np.float32)
    g_df = np.zeros(g_r.shape[1:], np.float32)
    for n in range(g_r.shape[0]):
        g_df = (g_df + copy_contribution(g_r[n], np.asarray(rot_tf[n], np.float32), np.asarray(inv_rot_tf[n], np.float32))).astype(np.float32)
    return g_df


def planes(resid, inv_trans_tf, HW, lambda_df):
    """G_R [N, H, W]: what the grad-translate kernel writes -- ResizeBilinearGrad of 2*lambda_df*resid, then the translate's
    registered gradient with the inverse vectors as given (oracle.sr.Superresolution.data_grad_copies_tf's first two stages)."""
    r = torch.from_numpy(np.ascontiguousarray(resid, dtype=np.float32)[..., None])
    g_t = tf_ops.resize_bilinear_grad((2.0 * float(lambda_df)) * r, tuple(HW))
    return tf_ops.projective_transform(g_t, np.asarray(inv_trans_tf, np.float32), output_shape=tuple(HW)).numpy()[..., 0].copy()


def registered_gather(g_r, inv_rot_tf):
    """The registered form on the same planes (one bilinear tap at R^-1 p per copy), copy order."""
    g = torch.from_numpy(np.ascontiguousarray(g_r, dtype=np.float32)[..., None])
    H, W = g_r.shape[1:]
    per = tf_ops.projective_transform(g, np.asarray(inv_rot_tf, np.float32), output_shape=(H, W)).numpy()[..., 0]
    out = np.zeros((H, W), np.float32)
    for n in range(per.shape[0]):
        out = (out + per[n]).astype(np.float32)
    return out


def data_grad_from_resid(resid, tfs, HW, lambda_df, adjoint="exact"):
    """g_df [H, W] from a residual [N, h, w] and tfs = (rot, trans, inv_rot, inv_trans) [N, 8]; an image the exact form does not
    apply to takes the registered statements, as the library does."""
    rot, tr, irot, itr = tfs
    g_r = planes(resid, itr, HW, lambda_df)
    if adjoint == "exact" and exact_applies(rot, tr, irot):
        return exact_gather(g_r, rot, irot)
    return registered_gather(g_r, irot)


class ExactAdjoint(o_sr.Superresolution):
    """A base to mix in BEHIND any oracle-based restatement (class X(TheRestatement, ExactAdjoint)): the per-copy data-term
    gradients that restatement sums in copy order become the exact contributions c_n.  The data term, the weights, the
    reweighting and the update rules of the classes in front are untouched -- only the gradient is swapped."""

    def loss_and_grad_tf(self, target, samples, rot_tf, trans_tf, inv_rot_tf, inv_trans_tf):
        self._adj_forward = (np.asarray(rot_tf, np.float32), np.asarray(trans_tf, np.float32))
        return super().loss_and_grad_tf(target, samples, rot_tf, trans_tf, inv_rot_tf, inv_trans_tf)

    def data_grad_copies_tf(self, resid, inv_rot_tf, inv_trans_tf):
        rot, tr = self._adj_forward
        if not exact_applies(rot, tr, inv_rot_tf):
            return super().data_grad_copies_tf(resid, inv_rot_tf, inv_trans_tf)
        g_r = planes(resid.numpy()[..., 0], inv_trans_tf, self.output_size, self.lambda_df)
        c = np.stack([copy_contribution(g_r[n], rot[n], np.asarray(inv_rot_tf[n], np.float32)) for n in range(len(rot))])
        return torch.from_numpy(np.ascontiguousarray(c[..., None]))


def data_grad(sr, x, samples, tfs, adjoint="exact"):
    """tests/sr_pd_ref.data_grad with the gather chosen by `adjoint`: sr an oracle Superresolution (its weights and data term are
    applied by its own forward statements when it has them), x [H, W], samples [N, h, w]."""
    rot, tr, irot, itr = tfs
    target = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)[None, :, :, None])
    smp = torch.from_numpy(np.ascontiguousarray(samples, dtype=np.float32)[..., None])
    resid = (sr.forward_model_tf(target, rot, tr) - smp).numpy()[..., 0]
    if getattr(sr, "df_loss", "l2") != "l2" or getattr(sr, "weights", None) is not None:      # q = w * psi(r), as sr_dt_ref hands it on
        import sr_dt_ref as RD
        resid = RD.weighted_psi(resid, sr.df_loss, sr.df_delta, sr.weights)
    return data_grad_from_resid(resid, tfs, sr.output_size, sr.lambda_df, adjoint)
