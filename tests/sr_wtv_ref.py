"""The edge-weighted TV prior of include/asr_hip.h ("edge-weighted TV"), restated in plain numpy / torch on top of oracle.sr.
TEST INFRASTRUCTURE ONLY: the oracle itself stays what it is; this file only replaces the TV statements of its loss and
gradient by their weighted form, so that unit weights give the oracle's own numbers bit for bit (test_sr_wtv_host.py)."""
import numpy as np
import torch

from oracle import sr as o_sr
from oracle import tf_ops


def edge_weights(I, beta):
    """I [H, W, 3] or [B, H, W, 3] float32 -> (wy, wx) float32 [H, W] / [B, H, W]: 1 / (1 + beta * d), d the squared forward
    difference of the guide summed over the channels as (a0*a0 + a1*a1) + a2*a2, every operation rounded to float32; the
    last row of wy and the last column of wx are 1."""
    I = np.asarray(I, dtype=np.float32)
    f = np.float32
    beta = f(beta)

    def w_of(a):
        d = (a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2]
        return (f(1.0) / (f(1.0) + beta * d)).astype(np.float32)

    wy = np.ones(I.shape[:-1], dtype=np.float32)
    wx = np.ones(I.shape[:-1], dtype=np.float32)
    wy[..., :-1, :] = w_of(I[..., 1:, :, :] - I[..., :-1, :, :])
    wx[..., :, :-1] = w_of(I[..., :, 1:, :] - I[..., :, :-1, :])
    return wy, wx


class WeightedSuperresolution(o_sr.Superresolution):
    """oracle.sr.Superresolution with the TV prior weighted by wy, wx [H, W] (float32 numpy)."""

    def __init__(self, *args, wy=None, wx=None, **kw):
        super().__init__(*args, **kw)
        assert not self.use_BTV
        self.wy = np.ascontiguousarray(wy, dtype=np.float32)
        self.wx = np.ascontiguousarray(wx, dtype=np.float32)

    def loss_terms_tf(self, target, samples, rot_tf, trans_tf):
        resid, dy, dx, df, _, l2, l1 = super().loss_terms_tf(target, samples, rot_tf, trans_tf)
        wy = torch.from_numpy(self.wy)[None, :, :, None]
        wx = torch.from_numpy(self.wx)[None, :, :, None]
        tv = torch.sum((wy * torch.abs(dy) + wx * torch.abs(dx)).double()).float()
        return resid, dy, dx, df, tv, l2, l1

    def tv(self, target):
        """sum (wy * |dy| + wx * |dx|): products and sum in float32, accumulated in float64."""
        dy, dx = tf_ops.image_gradients(target)
        wy = torch.from_numpy(self.wy)[None, :, :, None]
        wx = torch.from_numpy(self.wx)[None, :, :, None]
        return float(torch.sum((wy * torch.abs(dy) + wx * torch.abs(dx)).double()))

    def loss_and_grad_tf(self, target, samples, rot_tf, trans_tf, inv_rot_tf, inv_trans_tf):
        resid, dy, dx, df, tv, l2, l1 = self.loss_terms_tf(target, samples, rot_tf, trans_tf)
        loss = self.lambda_df * df + self.lambda_tv * tv
        loss = loss + self.lambda_L2 * l2
        if self.lambda_L1 > 0.0:
            loss = loss + self.lambda_L1 * l1
        g_x = self.data_grad_copies_tf(resid, inv_rot_tf, inv_trans_tf)
        g_df = torch.zeros_like(target)
        for i in range(g_x.shape[0]):
            g_df[0] += g_x[i]
        cy = torch.from_numpy(self.wy[None, :, :, None] * np.float32(self.lambda_tv))
        cx = torch.from_numpy(self.wx[None, :, :, None] * np.float32(self.lambda_tv))
        sy = torch.sign(dy) * cy
        sx = torch.sign(dx) * cx
        g_tv = -sy - sx
        g_tv[:, 1:] += sy[:, :-1]
        g_tv[:, :, 1:] += sx[:, :, :-1]
        grad = g_df + g_tv + (2.0 * self.lambda_L2) * target
        if self.lambda_L1 > 0.0:
            grad = grad + self.lambda_L1 * torch.sign(target)
        return loss, grad
