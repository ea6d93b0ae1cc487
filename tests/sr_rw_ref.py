"""The copy reweighting of include/asr_hip.h ("copy reweighting") restated in numpy, statement for statement: the per-copy energy
and mass in the header's fixed order of addition, the lower median by counting, the two weight functions, the apply step -- and
a reweighted solve over sr_dt_ref.DataTermSuperresolution: the oracle's loop with the weights replaced at the reweighting
iterations.  TEST INFRASTRUCTURE ONLY."""
import numpy as np
import torch

from oracle import sr as o_sr
from oracle import tf_ops

import sr_dt_ref as dtr
from sr_mon_ref import rho32

KINDS = ("cauchy", "hard")
MAX_COPIES = 640


def block_sum(v):
    """The float64 sum of v [P] in the order of one workgroup of 256 threads: thread t adds p = t, t + 256, ... in rising p from
    0.0; a wave adds its 64 lanes by the tree s[l] += s[l + o], o = 32 .. 1; the four waves add as ((w0 + w1) + w2) + w3."""
    v = np.asarray(v, dtype=np.float64).ravel()
    acc = np.zeros(256, dtype=np.float64)
    for k in range(0, v.size, 256):
        part = v[k:k + 256]
        acc[:part.size] = acc[:part.size] + part
    s = acc.reshape(4, 64).copy()
    o = 32
    while o >= 1:
        s[:, :o] = s[:, :o] + s[:, o:2 * o]
        o //= 2
    return np.float64(((s[0, 0] + s[1, 0]) + s[2, 0]) + s[3, 0])


def monitor_sum(v):
    """The float64 sum of v [P] in the order of the monitor's loss terms ("convergence monitor"): 256 workgroups of 256 threads,
    thread t of workgroup g adds p = g*256 + t + k*65536 in rising k from 0.0; the workgroup's tree as in block_sum; the 256
    partials added in index order from 0."""
    v = np.asarray(v, dtype=np.float64).ravel()
    K = max(1, -(-v.size // 65536))
    pad = np.zeros(K * 65536, dtype=np.float64)
    pad[:v.size] = v
    used = np.zeros(K * 65536, dtype=bool)
    used[:v.size] = True
    pad, used = pad.reshape(K, 256, 256), used.reshape(K, 256, 256)
    acc = np.zeros((256, 256), dtype=np.float64)
    for k in range(K):
        acc = np.where(used[k], acc + pad[k], acc)
    s = acc.reshape(256, 4, 64).copy()
    o = 32
    while o >= 1:
        s[:, :, :o] = s[:, :, :o] + s[:, :, o:2 * o]
        o //= 2
    parts = ((s[:, 0, 0] + s[:, 1, 0]) + s[:, 2, 0]) + s[:, 3, 0]
    total = np.float64(0.0)
    for g in range(256):
        total = total + parts[g]
    return total


def _base(u, b, shape):
    """The base weights of image b as [N, h*w] float32, or None."""
    if u is None:
        return None
    u = np.asarray(u, dtype=np.float32)
    B, N, h, w = shape
    if u.ndim == 3:
        return u.reshape(N, h * w)
    assert u.shape == tuple(shape)
    return u[b].reshape(N, h * w)


def copy_energy(r, loss="l2", delta=0.1, u=None):
    """r [B,N,h,w] float32, u None / [N,h,w] / [B,N,h,w] -> (energy, mass) float64 [B,N]."""
    r = np.asarray(r, dtype=np.float32)
    B, N, h, w = r.shape
    energy = np.zeros((B, N), dtype=np.float64)
    mass = np.zeros((B, N), dtype=np.float64)
    for b in range(B):
        ub = _base(u, b, r.shape)
        for i in range(N):
            ri = r[b, i].reshape(-1)
            energy[b, i] = block_sum(rho32(ri, loss, delta, None if ub is None else ub[i]))
            mass[b, i] = np.float64(h * w) if ub is None else block_sum(ub[i])
    return energy, mass


def copy_weights(energy, mass, kind="cauchy", kappa=2.0):
    """energy, mass float64 [B,N] -> (c float32 [B,N], scale float64 [B])."""
    assert kind in KINDS and np.isfinite(kappa) and kappa > 0
    energy = np.asarray(energy, dtype=np.float64)
    mass = np.asarray(mass, dtype=np.float64)
    B, N = energy.shape
    assert N <= MAX_COPIES
    c = np.zeros((B, N), dtype=np.float32)
    scale = np.zeros(B, dtype=np.float64)
    kappa = np.float64(kappa)
    with np.errstate(all="ignore"):
        for b in range(B):
            eb = energy[b] / mass[b]
            act = (mass[b] > 0.0) & np.isfinite(eb)
            idx = np.flatnonzero(act)
            A = idx.size
            s = np.float64(0.0)
            if A > 0:
                # rank by (value, index): a stable sort of the active values is the header's counting rank
                order = idx[np.argsort(eb[idx], kind="stable")]
                s = eb[order[(A - 1) // 2]]
            scale[b] = s
            if A == 0 or s == 0.0:
                c[b, idx] = np.float32(1.0)
                continue
            ks = kappa * s
            t = eb[idx] / ks
            if kind == "hard":
                c[b, idx] = np.where(t <= 1.0, np.float32(1.0), np.float32(0.0))
            else:
                tt = t * t
                den = 1.0 + tt
                c[b, idx] = (1.0 / den).astype(np.float32)
    return c, scale


def apply_copy_weights(r, c, loss="l2", delta=0.1, u=None):
    """-> (w_eff, q) float32 [B,N,h,w]: w_eff = u * c (c without weights), q = w_eff * psi(r)."""
    r = np.asarray(r, dtype=np.float32)
    c = np.asarray(c, dtype=np.float32)
    B, N, h, w = r.shape
    w_eff = np.empty_like(r)
    for b in range(B):
        ub = _base(u, b, r.shape)
        cb = np.broadcast_to(c[b][:, None], (N, h * w))
        w_eff[b] = (cb if ub is None else (ub * cb).astype(np.float32)).reshape(N, h, w)
    q = (w_eff * dtr.psi(r, loss, delta)).astype(np.float32)
    return w_eff, q


def reweight_iters(num_iter, every, start):
    return list(range(start, num_iter, every))


class ReweightedSuperresolution(dtr.DataTermSuperresolution):
    """DataTermSuperresolution whose loop replaces the weights at the reweighting iterations (one image, no copy dropout).
    After augmented_superresolution: copy_weights [N] (the last c, ones if the solve never reweighted), history [R, N],
    trajectory (the x after every update) and data_terms (iteration -> sum w_eff * rho(r), the float32 summands added in the
    monitor's order, under the weights in force at that iteration)."""

    def __init__(self, *args, rw_kind="cauchy", rw_kappa=2.0, rw_every=10, rw_start=10, **kw):
        super().__init__(*args, **kw)
        assert self.copy_dropout == 0.0
        self.rw = dict(kind=rw_kind, kappa=rw_kappa, every=rw_every, start=rw_start)
        self.base_weights = self.weights

    def augmented_superresolution(self, augmented_copies, angles, shifts, return_trajectory=False):
        samples = o_sr._stack(augmented_copies)
        angles = np.asarray(angles, dtype=np.float32)
        shifts = np.asarray(shifts, dtype=np.float32)
        n = samples.shape[0]
        target = tf_ops.resize_bilinear(samples[0:1], self.output_size).clone()
        opt = self.optimizer.optimizer
        slots = opt.new_slots(target)
        self.weights = self.base_weights
        self.copy_weights = np.ones(n, dtype=np.float32)
        self.history, self.trajectory, self.data_terms = [], [], {}
        points = set(reweight_iters(self.num_iter, self.rw["every"], self.rw["start"]))
        loss = None
        for i in range(self.num_iter):
            if self.optimizer.lr_scheduler:
                self.optimizer.lr_decay(i)
            if i in points:
                resid = o_sr.Superresolution.loss_terms(self, target, samples, angles, shifts)[0].numpy()[None, ..., 0]
                u = None if self.base_weights is None else self.base_weights
                e, a = copy_energy(resid, self.df_loss, self.df_delta, u)
                c, _ = copy_weights(e, a, self.rw["kind"], self.rw["kappa"])
                self.weights = apply_copy_weights(resid, c, self.df_loss, self.df_delta, u)[0][0]
                self.copy_weights = c[0]
                self.history.append(c[0].copy())
            if return_trajectory:
                resid = o_sr.Superresolution.loss_terms(self, target, samples, angles, shifts)[0].numpy()[..., 0]
                self.data_terms[i] = monitor_sum(rho32(resid, self.df_loss, self.df_delta, self.weights))
            loss, grad = self.loss_and_grad(target, samples, angles, shifts)
            opt.apply(target, grad, slots)
            if return_trajectory:
                self.trajectory.append(target[0].numpy().copy())
        self.history = np.stack(self.history) if self.history else np.zeros((0, n), dtype=np.float32)
        return target[0].numpy().copy(), float(loss)


def solve_case_rw(case, kind, df_loss="l2", df_delta=0.1, iters=dtr.ITERS, kappa=2.0, every=10, start=10):
    """sr_dt_ref's construction under the reweighted solve -> (x [H,H], the final copy weights [n])."""
    h = case["copies"].shape[-1]
    H = case["truth"].shape[-1]
    opt = o_sr.Optimizer("adam", dtr.LR, amsgrad=True)
    sr = ReweightedSuperresolution(*dtr.LAMBDAS, num_iter=iters, num_aug=len(case["copies"]), optimizer=opt, feature_size=(h, h),
                                   output_size=(H, H), df_loss=df_loss, df_delta=df_delta, rw_kind=kind, rw_kappa=kappa,
                                   rw_every=every, rw_start=start)
    x, _ = sr.augmented_superresolution(case["copies"][..., None], case["angles"], case["shifts"])
    return x[:, :, 0], sr.copy_weights
