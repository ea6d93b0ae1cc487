"""``Superresolution`` with the reference's surface (superresolution_scripts/superresolution.py:26-161):
``loss_function``, ``augmented_superresolution``, ``max_superresolution``, ``mean_superresolution``
-- plus batched variants that solve many images in one sequence of launches, and the robust one-pass fusions
``median_superresolution``, ``quantile_superresolution`` and ``trimmed_mean_superresolution`` (order statistics over the
realigned copies, ``realign_select_batch``), and their coverage-normalised forms ``covered_mean_superresolution``,
``covered_median_superresolution`` and ``coverage_map`` (``realign_covered_batch``), and ``variance_superresolution``, how
far the copies disagree at each pixel (``realign_moments_batch``).  All arithmetic
runs in the fused HIP kernels of csrc/sr.hip; this class only prepares float32 parameters.

``use_BTV`` swaps the TV prior for the bilateral TV of superresolution.py:8-23 (inside the same
kernels); ``copy_dropout`` drops a fixed random subset of the copies from the data term: the
reference draws the mask with np.random.shuffle inside a @tf.function (superresolution.py:44-53),
i.e. ONCE, when the function is traced on the first solve of a Superresolution object, and every
later iteration and image reuses it -- ``_drop_mask`` restates exactly that.

``tv_guide`` (not in the reference) puts the RGB image into the prior: the solves and ``loss_function`` take an image at
``output_size`` and weight every edge of the TV prior by 1 / (1 + tv_beta * |forward difference of the image|^2), so a jump
of the solution is cheap across an image edge and costs full price elsewhere (include/asr_hip.h: the rule).

``df_loss`` / ``df_delta`` (not in the reference, which carries the L1 line commented out) choose the data term sum w * rho(r):
"l2", "l1" or "huber"; ``df_weights`` on the solves and ``loss_function`` are its per-measurement weights w, [N,h,w] or
[B,N,h,w] on the device (include/asr_hip.h, "data term").  With "l2" and no weights the calls that ran before are made.

``Optimizer("primal_dual")`` (not in the reference) swaps the update rule for the primal-dual iteration of include/asr_hip.h,
"primal-dual": no learning rate; ``_solve_batch`` computes the step on the device from the transforms, weights and dropout
mask it solves (ops.sr_data_bound, ops.pd_steps).  It refuses ``use_BTV`` and ``df_loss="l1"``.

``reweight`` (not in the reference) down-weights whole unreliable copies inside the solve: "cauchy" or "hard", every
``reweight_every`` iterations from ``reweight_start`` each copy's residual energy against ``reweight_kappa`` times the median over
the copies of its image (include/asr_hip.h, "copy reweighting"); ``last_copy_weights`` then holds the ops.SrCopyWeights of the
last solve.  It multiplies ``df_weights`` and combines with every option above.

``adjoint`` (not in the reference) chooses the data-term gradient of the solves: "registered" is the reference's, TensorFlow's
registered gradient of the rotate (an inverse warp, not a gradient of the loss); "exact" is the transpose of the forward rotate
(include/asr_hip.h, "exact adjoint"), under which the primal-dual step bound is a true bound.  It combines with every option above.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib, ops, transforms as T
from .optimizer import Optimizer


def _stack_copies(copies, device):
    """list of [h,w,1] / [h,w] arrays, stacked ndarray or tensor -> device tensor [N,h,w]."""
    if isinstance(copies, torch.Tensor):
        t = copies.to(device=device, dtype=torch.float32)
    else:
        if isinstance(copies, (list, tuple)):
            if len(copies) and isinstance(copies[0], torch.Tensor):
                t = torch.stack([c.to(device=device, dtype=torch.float32) for c in copies])
            else:
                t = torch.as_tensor(np.stack([np.asarray(c, dtype=np.float32) for c in copies])).to(device)
        else:
            t = torch.as_tensor(np.asarray(copies, dtype=np.float32)).to(device)
    if t.dim() == 4 and t.shape[-1] == 1:
        t = t[..., 0]
    if t.dim() != 3:
        raise ValueError(f"augmented copies must be [N,h,w(,1)], got {tuple(t.shape)}")
    return t.contiguous()


def bilateral_tv(target_image, alpha=0.6, shift_factor=2):
    """The reference's module-level prior (superresolution.py:8-23): sum over the 15 integer shifts p = (h, v), h in
    [-s, s], v in [0, s], of alpha^(|h|+|v|) * || x - translate(x, p) ||_1 (zero fill).  target_image [1,H,W,1] / [H,W]
    (host array or device tensor) -> Python float; evaluated by the solver's own prior kernel (sr_loss_prior_kernel)."""
    import ctypes as C
    dev = _lib.require_gpu()
    t = target_image if isinstance(target_image, torch.Tensor) else torch.as_tensor(np.asarray(target_image, dtype=np.float32))
    t = t.to(device=dev, dtype=torch.float32)
    if t.dim() == 4:
        if t.shape[0] != 1 or t.shape[-1] != 1:
            raise ValueError(f"bilateral_tv expects [1,H,W,1] or [H,W], got {tuple(t.shape)}")
        t = t[0, :, :, 0]
    if t.dim() != 2:
        raise ValueError(f"bilateral_tv expects [1,H,W,1] or [H,W], got {tuple(t.shape)}")
    x = t.contiguous()[None]
    H, W = x.shape[1:]
    resid = torch.zeros(1, dtype=torch.float32, device=dev)                 # no data term: one zero residual
    terms = torch.empty((1, 4), dtype=torch.float64, device=dev)
    cfg = ops.sr_config(use_btv=True, btv_alpha=alpha, btv_shift=shift_factor)
    ops.call("asr_sr_loss_terms_cfg_f64", ops.ptr(x), ops.ptr(resid), ops.ptr(terms, torch.float64), 1, 1, H, W, 1, 1,
             C.byref(cfg), ops.stream_ptr())
    return float(terms[0, 1].item())


COVER_MODES = ("frame", "validity")


class Superresolution:
    def __init__(self, lambda_df, lambda_tv, lambda_L2, lambda_L1, num_iter=200, num_aug=100,
                 optimizer: Optimizer = None, feature_size=(64, 64), output_size=(512, 512), use_BTV=False,
                 verbose=False, copy_dropout=0.0, trim=0.1, cover="frame", cov_min=0.5, valid_min=0.5, tv_beta=100.0,
                 df_loss="l2", df_delta=0.1, stop_rel_tol=None, stop_patience=3, stop_every=1, stop_min_iter=0,
                 keep_history=False, reweight=None, reweight_kappa=2.0, reweight_every=10, reweight_start=10,
                 adjoint="registered"):
        # the data-term gradient of the solves: "registered" (the reference's: TensorFlow's registered gradient of the rotate, an
        # inverse warp; the calls and launches that always ran) or "exact" (its transpose; include/asr_hip.h, "exact adjoint")
        ops.check_adjoint(adjoint, "Superresolution: adjoint")
        self.adjoint = "registered" if adjoint is None else adjoint.lower()
        self.tv_beta = ops.check_tv_beta(tv_beta, "Superresolution: tv_beta")
        # the convergence monitor (include/asr_hip.h): with stop_rel_tol each image of a solve stops by itself once its loss
        # has not improved by that relative amount for stop_patience evaluations in a row (one every stop_every iterations,
        # none before stop_min_iter); keep_history alone records the loss terms and never stops.  Neither: the solves and
        # their launches are what they always were.  self.last_trace: the ops.SrTrace of the last monitored solve.
        self.monitor = self.check_stop(stop_rel_tol, stop_patience, stop_every, stop_min_iter, keep_history)
        if self.monitor is not None and verbose:
            raise ValueError("Superresolution: verbose prints by cutting the solve into calls and cannot be combined with "
                             "stop_rel_tol / keep_history (read last_trace instead)")
        self.last_trace = None
        # copy reweighting (include/asr_hip.h): None, or the reweight dict of ops.sr_solve.  self.last_copy_weights: the
        # ops.SrCopyWeights of the last solve, None when that solve did not reweight ([B, N] per solved plane; under copy_dropout
        # N counts the kept copies).
        self.reweight = self.check_reweight(reweight, reweight_kappa, reweight_every, reweight_start)
        if self.reweight is not None and verbose:
            raise ValueError("Superresolution: verbose prints by cutting the solve into calls and cannot be combined with "
                             "reweight (the weights would start over in every call)")
        self.last_copy_weights = None
        # the data term sum w * rho(r): "l2" (the reference's), "l1" or "huber" with threshold df_delta, in the units of the
        # stacks (the path normalises them to [0, 1]); the weights w come per solve (df_weights=)
        ops.check_data_term(df_loss, df_delta, "Superresolution: df_loss")
        self.df_loss = "l2" if df_loss is None else df_loss.lower()
        self.df_delta = float(df_delta) if self.df_loss == "huber" else df_delta
        if not 0.0 <= float(trim) < 0.5:
            raise ValueError(f"trim must be in [0, 0.5), got {trim}")
        if cover not in COVER_MODES:
            raise ValueError(f"cover must be one of {COVER_MODES}, got {cover!r}")
        for name, v in (("cov_min", cov_min), ("valid_min", valid_min)):
            if not (np.isfinite(float(v)) and float(v) > 0.0):
                raise ValueError(f"{name} must be finite and > 0, got {v}")
        self.lambda_df = lambda_df
        self.lambda_tv = lambda_tv
        self.lambda_L2 = lambda_L2
        self.lambda_L1 = lambda_L1
        self.num_iter = num_iter
        self.num_aug = num_aug
        self.optimizer = optimizer
        self.feature_size = tuple(feature_size)
        self.output_size = tuple(output_size)
        self.use_BTV = use_BTV
        self.verbose = verbose
        self.copy_dropout = copy_dropout
        self.trim = float(trim)      # trimmed-mean SR drops int(trim * n) copies at each end (scipy.stats.trim_mean's rule)
        # the covered fusions: "frame" counts only what the realign itself moved out of the output frame (a shared all-ones
        # weight plane), "validity" also what each copy lost when it was made (augmentation_utils.copy_validity)
        self.cover = cover
        self.cov_min = float(cov_min)
        self.valid_min = float(valid_min)
        self._drop_masks = {}        # n_drop -> bool [num_aug], frozen at first use (tf.function trace time)

    # -- parameter preparation ----------------------------------------------------------------
    @staticmethod
    def check_stop(stop_rel_tol=None, stop_patience=3, stop_every=1, stop_min_iter=0, keep_history=False):
        """The stop_* / keep_history keywords -> None (no monitor) or the monitor dict of ops.sr_solve; ValueError on a bad
        value, on the host.  With a tolerance the patience must be >= 1 (patience 0 never stops: say keep_history)."""
        if not isinstance(keep_history, (bool, np.bool_)):
            raise ValueError(f"keep_history must be True or False, got {keep_history!r}")
        if stop_rel_tol is None:
            mon = ops.check_sr_monitor(dict(every=stop_every, rel_tol=0.0, patience=0, min_iter=stop_min_iter, history=True),
                                       "Superresolution: stop")
            ops.check_sr_monitor(dict(patience=stop_patience), "Superresolution: stop")
            return mon if keep_history else None
        mon = ops.check_sr_monitor(dict(every=stop_every, rel_tol=stop_rel_tol, patience=stop_patience, min_iter=stop_min_iter,
                                        history=bool(keep_history)), "Superresolution: stop")
        if mon["patience"] < 1:
            raise ValueError(f"Superresolution: stop_patience must be >= 1 with stop_rel_tol, got {stop_patience!r}")
        return mon

    @staticmethod
    def check_reweight(reweight=None, reweight_kappa=2.0, reweight_every=10, reweight_start=10):
        """The reweight* keywords -> None (no reweighting) or the reweight dict of ops.sr_solve; ValueError on a bad value, on
        the host (the other three are checked even when reweight is None)."""
        p = ops.check_sr_reweight(dict(kind="cauchy" if reweight is None else reweight, kappa=reweight_kappa, every=reweight_every,
                                       start=reweight_start, history=False), "Superresolution: reweight")
        return None if reweight is None else p

    @staticmethod
    def reweight_keywords(reweight):
        """A reweight dict (kind and any of kappa, every, start; None: no reweighting) -> the constructor's reweight* keywords:
        what the scripts build from their --sr_reweight* flags."""
        if reweight is None:
            return {}
        unknown = sorted(set(reweight) - {"kind", "kappa", "every", "start"})
        if unknown or "kind" not in reweight:
            raise ValueError(f"Superresolution: reweight_keywords takes kind and any of kappa, every, start, got {reweight!r}")
        return dict({"reweight_" + k: v for k, v in reweight.items() if k != "kind"}, reweight=reweight["kind"])

    @property
    def _lambdas(self):
        return (self.lambda_df, self.lambda_tv, self.lambda_L2, self.lambda_L1)

    def _transforms(self, angles, shifts, device, inverse=False, negate=False):
        """angles [B,N], shifts [B,N,2] -> device [B,N,8] rotation and translation transforms."""
        H, Wd = self.output_size
        angles = np.asarray(angles, dtype=np.float32)
        shifts = np.asarray(shifts, dtype=np.float32)
        if negate:
            angles, shifts = -angles, -shifts
        b, n = angles.shape
        rot = T.rotation_transforms(angles.reshape(-1), H, Wd)
        tr = T.translation_transforms(shifts.reshape(-1, 2))
        if inverse:
            rot, tr = T.inverse_transforms(rot), T.inverse_transforms(tr)
        return ops.to_device(rot.reshape(b, n, 8), device=device), ops.to_device(tr.reshape(b, n, 8), device=device)

    def _drop_mask(self, n_drop):
        """superresolution.py:47-50; np.random.shuffle consumes the global numpy stream once per (object, n_drop)."""
        if n_drop not in self._drop_masks:
            mask = np.full(self.num_aug, fill_value=True)
            mask[:n_drop] = False
            np.random.shuffle(mask)
            self._drop_masks[n_drop] = mask
        return self._drop_masks[n_drop]

    def _config(self):
        """asr_sr_config of this solver: the optimizer's update rule + the TV / bilateral-TV choice."""
        if self.optimizer is None:
            return ops.sr_config(use_btv=self.use_BTV)
        return self.optimizer.optimizer.config(use_btv=self.use_BTV)

    def _check_tv_guide(self, tv_guide):
        """Host checks of a tv_guide argument, before anything touches the device: None, an RGB image [H,W,3] or a batch
        [B,H,W,3] at output_size (host array or device tensor), or a pair (wy, wx) of edge weights already on the device
        (ops.tv_edge_weights' output, [H,W] shared or [B,H,W]; ops checks their shape against the solve's)."""
        if tv_guide is None:
            return
        if self.use_BTV:
            raise ValueError("tv_guide: bilateral TV (use_BTV=True) has no edge-weighted form")
        if isinstance(tv_guide, (tuple, list)) and len(tv_guide) == 2 and all(isinstance(t, torch.Tensor) for t in tv_guide):
            return
        shape = tuple(tv_guide.shape) if hasattr(tv_guide, "shape") else tuple(np.shape(tv_guide))
        if len(shape) not in (3, 4) or shape[-1] != 3 or shape[-3:-1] != self.output_size:
            raise ValueError(f"tv_guide must be an RGB image [H,W,3] or [B,H,W,3] at output_size {self.output_size}, got "
                             f"{shape}")

    def _tv_weights(self, tv_guide, batch, dev):
        """tv_guide (checked) -> None or the (wy, wx) of ops.sr_solve / sr_backward / sr_loss_terms for `batch` images."""
        if tv_guide is None:
            return None
        if isinstance(tv_guide, (tuple, list)):
            return tuple(tv_guide)
        g = tv_guide if isinstance(tv_guide, torch.Tensor) else torch.as_tensor(np.asarray(tv_guide, dtype=np.float32))
        g = g.to(device=dev, dtype=torch.float32).contiguous()
        if g.dim() == 4 and g.shape[0] != batch:
            raise ValueError(f"tv_guide holds {g.shape[0]} images, the solve {batch}")
        return ops.tv_edge_weights(g, self.tv_beta)

    def _data_term(self):
        """The data_term argument of the ops calls: None for the reference's L2 (the calls that ran before data terms existed)."""
        return None if self.df_loss == "l2" else (self.df_loss, self.df_delta)

    def _check_df_weights(self, df_weights):
        """Host check of a df_weights argument, before anything touches the device: None, or a float32 tensor [N,h,w] (shared
        by the images / classes of the solve) or [B,N,h,w] at feature_size (ops checks N and B against the solve's)."""
        if df_weights is None:
            return
        if not isinstance(df_weights, torch.Tensor) or df_weights.dtype != torch.float32 or df_weights.dim() not in (3, 4) \
                or tuple(df_weights.shape[-2:]) != self.feature_size:
            got = tuple(df_weights.shape) if hasattr(df_weights, "shape") else type(df_weights).__name__
            raise ValueError(f"df_weights must be a float32 tensor [N,h,w] or [B,N,h,w] at feature_size {self.feature_size}, "
                             f"got {got}")

    def _masked_weights(self, df_weights, mask, dev):
        """df_weights (checked) on the device of the solve, without the copies that copy_dropout's mask drops (None: all)."""
        if df_weights is None:
            return None
        wts = df_weights.to(dev)
        if mask is not None:
            if wts.shape[-3] != len(mask):
                raise ValueError(f"copy_dropout needs weights for num_aug={len(mask)} copies, got {tuple(wts.shape)}")
            wts = wts.index_select(wts.dim() - 3, torch.as_tensor(np.flatnonzero(mask), device=dev))
        return wts.contiguous()

    @staticmethod
    def _batchify(angles, shifts):
        a = np.asarray(angles, dtype=np.float32)
        s = np.asarray(shifts, dtype=np.float32)
        return (a[None], s[None]) if a.ndim == 1 else (a, s)

    # -- superresolution.py:44-100 ------------------------------------------------------------------
    def loss_function(self, target_image, augmented_samples, angles, shifts, n_drop=0, tv_guide=None, df_weights=None):
        self._check_tv_guide(tv_guide)
        self._check_df_weights(df_weights)
        dev = _lib.require_gpu()
        y = _stack_copies(augmented_samples, dev)[None]
        a, s = self._batchify(angles, shifts)
        if n_drop != 0:
            keep = torch.as_tensor(self._drop_mask(n_drop), device=dev)
            y, a, s = y[:, keep].contiguous(), a[:, self._drop_mask(n_drop)], s[:, self._drop_mask(n_drop)]
        wts = self._masked_weights(df_weights, self._drop_mask(n_drop) if n_drop != 0 else None, dev)
        x = torch.as_tensor(np.asarray(target_image.cpu() if isinstance(target_image, torch.Tensor) else target_image,
                                       dtype=np.float32)).to(dev).reshape(1, *self.output_size).contiguous()
        rot, tr = self._transforms(a, s, dev)
        tvw = self._tv_weights(tv_guide, 1, dev)
        dt = self._data_term()
        if dt is None and wts is None:
            resid = ops.sr_forward_residual(x, y, rot, tr)
            return self._loss_from_terms(ops.sr_loss_terms(x, resid, self._config(), tv_weights=tvw).cpu().numpy()[0])
        _, raw = ops.sr_forward_residual(x, y, rot, tr, data_term=dt, weights=wts, want_raw=True)
        terms = ops.sr_loss_terms(x, raw, self._config(), tv_weights=tvw, data_term=dt, weights=wts)
        return self._loss_from_terms(terms.cpu().numpy()[0])

    def _loss_from_terms(self, t):
        f = np.float32
        loss = f(self.lambda_df) * f(t[0]) + f(self.lambda_tv) * f(t[1])
        loss = loss + f(self.lambda_L2) * f(t[2])
        if self.lambda_L1 > 0.0:
            loss = loss + f(self.lambda_L1) * f(t[3])
        return float(loss)

    # -- superresolution.py:102-137 -------------------------------------------------------------------
    def augmented_superresolution_batch(self, copies, angles, shifts, tv_guide=None, df_weights=None):
        """copies [B,N,h,w] device tensor, angles [B,N], shifts [B,N,2] -> (device [B,H,W], [B] losses).
        The global Adam step counter advances image by image (reference order), the device then
        iterates all images together.  tv_guide: one RGB image [H,W,3] shared by the batch or [B,H,W,3] (_check_tv_guide).
        df_weights: the weights of the data term, a device tensor [N,h,w] shared by the batch or [B,N,h,w] (_check_df_weights)."""
        self._check_tv_guide(tv_guide)
        self._check_df_weights(df_weights)
        return self._solve_batch(copies, angles, shifts,
                                 lambda b: np.stack([self.optimizer.schedule_alphas(self.num_iter) for _ in range(b)], axis=1),
                                 tv_guide, df_weights)

    def augmented_superresolution_classes(self, copies, angles, shifts, start_steps, tv_guide=None, df_weights=None,
                                          couple=False):
        """The copies of K classes of ONE image in one batched solve: copies [K,N,h,w] device tensor, angles [N], shifts [N,2]
        (the image's transforms, repeated for every class), start_steps [K] -> (device [K,H,W], [K] losses).  Class k's
        step scalars are those of a solve that starts at the global step counter start_steps[k]; the counter itself is left
        as it was (the caller decides what the classes' solves count as).  copy_dropout uses the object's frozen mask.
        tv_guide: the image's RGB [H,W,3], or its edge weights (wy, wx) [H,W], shared by the K classes.
        df_weights: the weights of the data term, [N,h,w] shared by the K classes (or [K,N,h,w]).
        couple: the K classes are one coupled solve (ops.sr_solve's coupling=K: x >= 0 and sum_k x_k <= 1 at every pixel, a
        monitor stops them together); needs Optimizer("primal_dual"), ValueError otherwise.  augmented_superresolution_batch
        solves different images and is never coupled."""
        self._check_tv_guide(tv_guide)
        self._check_df_weights(df_weights)
        if self.optimizer is None:
            raise Exception("You must provide an instance of the Optimizer class to compute the augmented SR")
        if couple:
            self.check_couple()
        k = copies.shape[0]
        starts = [int(s) for s in start_steps]
        if len(starts) != k:
            raise ValueError(f"{k} classes of copies but {len(starts)} start steps")
        state = self.optimizer.optimizer
        saved = state.iterations
        columns = []
        try:
            for s in starts:
                state.iterations = s
                columns.append(self.optimizer.schedule_alphas(self.num_iter))
        finally:
            state.iterations = saved
        a = np.repeat(np.asarray(angles, dtype=np.float32)[None], k, axis=0)
        s = np.repeat(np.asarray(shifts, dtype=np.float32)[None], k, axis=0)
        return self._solve_batch(copies, a, s, lambda b: np.stack(columns, axis=1).reshape(self.num_iter, b), tv_guide,
                                 df_weights, coupling=k if couple else None)

    def check_couple(self):
        """Host check of couple=True: the projection is the last prox step of the primal-dual iteration and of no other rule."""
        if self.optimizer is None or self.optimizer.optimizer.kind != _lib.OPT_PRIMAL_DUAL:
            raise ValueError("Superresolution: couple=True needs Optimizer('primal_dual') (the coupling is a prox step of that rule)")

    def _solve_batch(self, copies, angles, shifts, make_alphas, tv_guide=None, df_weights=None, coupling=None):
        """The batched solve; make_alphas(B) -> float32 [num_iter, B] step scalars.  coupling: ops.sr_solve's."""
        if self.optimizer is None:
            raise Exception("You must provide an instance of the Optimizer class to compute the augmented SR")
        if self.reweight is not None and self.verbose:      # also when a caller set self.reweight after construction (HotPath does)
            raise ValueError("Superresolution: verbose prints by cutting the solve into calls and cannot be combined with "
                             "reweight (the weights would start over in every call)")
        self.last_copy_weights = None                       # of THIS solve: None when it does not reweight (or num_iter = 0)
        dev = copies.device
        b, n, h, w = copies.shape
        if (h, w) != self.feature_size:
            raise ValueError(f"copies are {h}x{w} but feature_size is {self.feature_size}")
        x = ops.sr_init_target(copies, self.output_size)          # from copy 0 of the FULL stack (superresolution.py:112-114)
        n_drop = int(self.num_aug * self.copy_dropout)
        mask = None
        if n_drop != 0:
            if n != self.num_aug:
                raise ValueError(f"copy_dropout needs num_aug={self.num_aug} copies per image, got {n}")
            mask = self._drop_mask(n_drop)
            copies = copies[:, torch.as_tensor(mask, device=dev)].contiguous()
            angles, shifts = np.asarray(angles)[:, mask], np.asarray(shifts)[:, mask]
        wts = self._masked_weights(df_weights, mask, dev)      # copy_dropout masks the weights with the copies
        rot, tr = self._transforms(angles, shifts, dev)
        irot, itr = self._transforms(angles, shifts, dev, inverse=True)
        alphas = make_alphas(b)                                                                # [iter, B]
        if self.num_iter == 0:
            return x, [None] * b
        state = self.optimizer.optimizer
        if state.kind == _lib.OPT_PRIMAL_DUAL:
            # no learning rate: the step comes from the transforms, weights and dropout mask actually solved, on the device
            # (make_alphas above only advanced the step counter, by num_iter per image like every other rule)
            if self.optimizer.lr_scheduler:
                raise ValueError("Superresolution: primal_dual has no learning rate to schedule (lr_scheduler=True)")
            if self.df_loss == "l1":
                raise ValueError("Superresolution: primal_dual needs a smooth data term (df_loss 'l2' or 'huber')")
            bound = ops.sr_data_bound(rot, tr, irot, itr, self.output_size, (h, w), self.lambda_df, weights=wts,
                                      iters=state.bound_iters, adjoint="exact" if self.adjoint == "exact" else None)
            alphas_dev = ops.pd_steps(bound, self.lambda_L2, self.num_iter)
        else:
            alphas_dev = ops.to_device(alphas, device=dev)
        kw = dict(want_loss=True, cfg=state.config(use_btv=self.use_BTV), slot_init=state.slot_init)
        if tv_guide is not None:
            kw["tv_weights"] = self._tv_weights(tv_guide, b, dev)
        if self._data_term() is not None or wts is not None:
            kw.update(data_term=self._data_term(), weights=wts)
        if coupling is not None:
            kw["coupling"] = coupling
        if self.adjoint == "exact":                          # "registered": no keyword, the calls that always ran
            kw["adjoint"] = "exact"
        if self.reweight is not None:
            out = ops.sr_solve(x, copies, rot, tr, irot, itr, alphas_dev, self._lambdas, monitor=self.monitor,
                               reweight=self.reweight, **kw)
            self.last_copy_weights = out[-1]
            if self.monitor is not None:
                self.last_trace = out[2]
            return out[0], out[1]
        if self.monitor is not None:
            # the schedule above covers all num_iter iterations whether an image stops or not: the optimiser's step counter
            # never depends on a device result
            x, terms, self.last_trace = ops.sr_solve(x, copies, rot, tr, irot, itr, alphas_dev, self._lambdas,
                                                     monitor=self.monitor, **kw)
            return x, terms
        if not self.verbose:
            return ops.sr_solve(x, copies, rot, tr, irot, itr, alphas_dev, self._lambdas, **kw)
        # superresolution.py:130-131 prints the loss of iteration i (evaluated before that iteration's update) for
        # i % 10 == 0 and for the last one.  The solver reports the loss of the LAST iteration of a call, so the solve is
        # cut after each printing iteration; the slots and the workspace carry over (same updates as one call).
        carry, first, terms = {}, 0, None
        for i in range(self.num_iter):
            if i % 10 == 0 or i == self.num_iter - 1:
                x, terms = ops.sr_solve(x, copies, rot, tr, irot, itr, alphas_dev[first:i + 1].contiguous(), self._lambdas,
                                        state=carry, **kw)
                first = i + 1
                for bi, t in enumerate(terms.cpu().numpy()):
                    tag = f"[image {bi}] " if b > 1 else ""
                    print(f"{tag}{i + 1}/{self.num_iter} -- loss = {self._loss_from_terms(t)}")
        return x, terms

    def augmented_superresolution(self, augmented_copies, angles, shifts, tv_guide=None, df_weights=None):
        self._check_tv_guide(tv_guide)
        self._check_df_weights(df_weights)
        if self.optimizer is None:
            raise Exception(
                "You must provide an instance of the Optimizer class to compute the augmented SR")
        dev = _lib.require_gpu()
        y = _stack_copies(augmented_copies, dev)[None]
        a, s = self._batchify(angles, shifts)
        x, terms = self.augmented_superresolution_batch(y, a, s, tv_guide=tv_guide, df_weights=df_weights)
        loss = self._loss_from_terms(terms.cpu().numpy()[0]) if isinstance(terms, torch.Tensor) else None
        return x[0].cpu().numpy()[..., None], loss

    # -- superresolution.py:139-161 ---------------------------------------------------------------------
    def realign_batch(self, copies, angles, shifts, mode):
        """copies [B,N,h,w] device -> device [B,H,W]; translate(-shift) then rotate(-angle), max / mean
        (mode "both": the pair (max, mean) from one pass)."""
        rot, tr = self._transforms(angles, shifts, copies.device, negate=True)
        return ops.realign(copies, tr, rot, self.output_size, mode)

    def _realign_single(self, augmented_copies, angles, shifts, mode):
        dev = _lib.require_gpu()
        y = _stack_copies(augmented_copies, dev)[None]
        a, s = self._batchify(angles, shifts)
        return self.realign_batch(y, a, s, mode)[0].cpu().numpy()[..., None], None

    def max_superresolution(self, augmented_copies, angles, shifts):
        return self._realign_single(augmented_copies, angles, shifts, "max")

    def mean_superresolution(self, augmented_copies, angles, shifts):
        return self._realign_single(augmented_copies, angles, shifts, "mean")

    # -- order statistics over the realigned copies (not in the reference) -------------------------------------------
    def realign_select_batch(self, copies, angles, shifts, qs=(), trim=None):
        """copies [B,N,h,w] device, realigned as in realign_batch -> (device [len(qs),B,H,W] or None, device [B,H,W] or
        None): the pixel-wise quantiles qs (linear interpolation between the two nearest ranks, numpy's default; 0.5 is the
        median) and, with trim (a fraction in [0, 0.5)), the mean of the sorted copies without the int(trim * N) smallest
        and the int(trim * N) largest.  One launch; the N realigned planes are never written."""
        n = copies.shape[1]
        k = None
        if trim is not None:
            if not 0.0 <= float(trim) < 0.5:
                raise ValueError(f"trim must be in [0, 0.5), got {trim}")
            k = int(float(trim) * n)
        rot, tr = self._transforms(angles, shifts, copies.device, negate=True)
        ranks = [ops.quantile_ranks(n, q) for q in qs]
        return ops.realign_select(copies, tr, rot, self.output_size, ranks=ranks, trim_k=k)

    def _select_single(self, augmented_copies, angles, shifts, qs=(), trim=None):
        dev = _lib.require_gpu()
        y = _stack_copies(augmented_copies, dev)[None]
        a, s = self._batchify(angles, shifts)
        q_out, t_out = self.realign_select_batch(y, a, s, qs=qs, trim=trim)
        out = q_out[0, 0] if trim is None else t_out[0]
        return out.cpu().numpy()[..., None], None

    def quantile_superresolution(self, augmented_copies, angles, shifts, q):
        return self._select_single(augmented_copies, angles, shifts, qs=(q,))

    def median_superresolution(self, augmented_copies, angles, shifts):
        return self.quantile_superresolution(augmented_copies, angles, shifts, 0.5)

    def trimmed_mean_superresolution(self, augmented_copies, angles, shifts):
        return self._select_single(augmented_copies, angles, shifts, trim=self.trim)

    # -- coverage-normalised fusions over the realigned copies (not in the reference) --------------------------------
    def realign_covered_batch(self, copies, angles, shifts, want):
        """copies [B,N,h,w] device, realigned as in realign_batch -> dict of device [B,H,W] with the keys of want, any of
        "mean", "median", "cov" (ops.realign_covered): the weights go through the realign of the copies, the mean is the sum
        of the realigned values over the sum of the realigned weights (0 below cov_min), the median runs over the copies
        whose realigned weight reaches valid_min, and "cov" is the sum of the realigned weights: on how many copies any
        fusion of them rests at each pixel.  One launch."""
        wgt = self._cover_planes(copies, angles, shifts, self.cover)
        y = copies if self.cover == "frame" else (copies * wgt).contiguous()
        rot, tr = self._transforms(angles, shifts, copies.device, negate=True)
        return ops.realign_covered(y, wgt, tr, rot, self.output_size, want=want, cov_min=self.cov_min,
                                   valid_min=self.valid_min)

    def _cover_planes(self, copies, angles, shifts, cover):
        """The weight planes of copies [B,N,h,w] under a cover mode: one shared all-ones [h,w] plane ("frame"), or each
        copy's validity [B,N,h,w] ("validity")."""
        b, n, h, w = copies.shape
        if cover == "frame":
            return torch.ones((h, w), dtype=torch.float32, device=copies.device)
        from .augmentation_utils import copy_validity
        a, s = np.asarray(angles, dtype=np.float32), np.asarray(shifts, dtype=np.float32)
        return torch.stack([copy_validity(a[i], s[i], self.output_size, (h, w)) for i in range(b)]).contiguous()

    def _covered_single(self, augmented_copies, angles, shifts, key):
        dev = _lib.require_gpu()
        y = _stack_copies(augmented_copies, dev)[None]
        a, s = self._batchify(angles, shifts)
        return self.realign_covered_batch(y, a, s, (key,))[key][0].cpu().numpy()[..., None], None

    def covered_mean_superresolution(self, augmented_copies, angles, shifts):
        return self._covered_single(augmented_copies, angles, shifts, "mean")

    def covered_median_superresolution(self, augmented_copies, angles, shifts):
        return self._covered_single(augmented_copies, angles, shifts, "median")

    def coverage_map(self, augmented_copies, angles, shifts):
        return self._covered_single(augmented_copies, angles, shifts, "cov")

    # -- how far the realigned copies disagree (not in the reference) ------------------------------------------------
    _OBJECT_COVER = object()

    def realign_moments_batch(self, copies, angles, shifts, want=("mean", "var"), cover=_OBJECT_COVER):
        """copies [B,N,h,w] device, realigned as in realign_batch -> dict of device [B,H,W] with the keys of want, any of
        "mean", "var", "nv" (ops.realign_moments): the mean over the copies that saw the pixel, the population variance of
        those copies about it, and their number.  cover: the object's by default -- "frame" (a copy is valid where the realign
        kept it inside the output frame) or "validity" (where it also came from inside the image), a copy counting where
        its realigned weight reaches valid_min; the copies themselves are NOT multiplied by the weights -- or None: no
        weight plane at all, every copy is valid everywhere, zero fill included ("mean" is then realign_batch's mean bit for
        bit).  One launch."""
        cover = self.cover if cover is self._OBJECT_COVER else cover
        if cover is not None and cover not in COVER_MODES:
            raise ValueError(f"cover must be None or one of {COVER_MODES}, got {cover!r}")
        wgt = self._cover_planes(copies, angles, shifts, cover) if cover is not None else None
        rot, tr = self._transforms(angles, shifts, copies.device, negate=True)
        return ops.realign_moments(copies, tr, rot, self.output_size, want=want, wgt=wgt, valid_min=self.valid_min)

    def variance_superresolution(self, augmented_copies, angles, shifts):
        """([H, W, 1] float32 population variance of the realigned copies at each pixel, None): max_superresolution's
        arguments and return shape, under the object's cover and valid_min."""
        dev = _lib.require_gpu()
        y = _stack_copies(augmented_copies, dev)[None]
        a, s = self._batchify(angles, shifts)
        return self.realign_moments_batch(y, a, s, ("var",))["var"][0].cpu().numpy()[..., None], None
