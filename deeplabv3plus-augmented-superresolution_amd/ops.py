"""Thin tensor-level wrappers over the C ABI (include/asr_hip.h).

Every function takes contiguous float32 ROCm tensors, checks shapes on the host (a kernel that
indexes out of bounds can take the whole node down), launches on torch's current stream and
returns device tensors.  Nothing here computes on the CPU.
"""
from __future__ import annotations

import ctypes as C
import numbers
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._lib import AsrError, call, ptr, stream_ptr

f32 = torch.float32


def _dev(t):
    return t.device


def to_device(a, dtype=f32, device=None):
    """Host array -> device tensor on the CURRENT stream.  Small parameter arrays (transform vectors, step sizes) go
    through pinned memory with a non-blocking copy: a pageable copy makes the host wait for everything already queued
    on the stream (e.g. a whole forward pass), which would serialise the lanes of the pipelined hot path."""
    device = device or _lib.require_gpu()
    if isinstance(a, torch.Tensor):
        return a.to(device=device, dtype=dtype).contiguous()
    t = torch.as_tensor(np.ascontiguousarray(a), dtype=dtype)
    if t.numel() * t.element_size() <= (1 << 20):
        return t.pin_memory().to(device, non_blocking=True)      # the caching host allocator keeps the staging buffer alive
    return t.to(device)


# ---------------------------------------------------------------------------------------------
# warps
# ---------------------------------------------------------------------------------------------
def warp_affine(src, transforms, out_hw=None, n=None, interpolation="bilinear"):
    """src [N,H,W,C] or [H,W,C] (shared), transforms [N,8] or [8] (shared) -> [N,Ho,Wo,C]; interpolation
    "bilinear" or "nearest" (ImageProjectiveTransformV3, zero fill)."""
    if interpolation not in ("bilinear", "nearest"):
        raise AsrError("warp_affine: interpolation must be 'bilinear' or 'nearest'")
    src_b = src.dim() == 4
    tf_b = transforms.dim() == 2
    if src_b:
        n_src, h, w, c = src.shape
    else:
        h, w, c = src.shape
        n_src = None
    n_tf = transforms.shape[0] if tf_b else None
    n = n or n_src or n_tf or 1
    if (n_src is not None and n_src != n) or (n_tf is not None and n_tf != n):
        raise AsrError(f"warp_affine: batch mismatch src={n_src} transforms={n_tf} n={n}")
    if transforms.shape[-1] != 8:
        raise AsrError("warp_affine: transforms must have 8 coefficients")
    ho, wo = out_hw or (h, w)
    dst = torch.empty((n, ho, wo, c), dtype=f32, device=src.device)
    call("asr_warp_affine_f32" if interpolation == "bilinear" else "asr_warp_affine_nearest_f32", ptr(src), ptr(dst),
         ptr(transforms), n, int(src_b), int(tf_b), h, w, ho, wo, c, stream_ptr())
    return dst


def augment_copies(image, rot_tf, trans_tf, out=None):
    """image [H,W,C] -> [N,H,W,C] = translate(rotate(tile(image))); out: an [N,H,W,C] tensor to write into (e.g. the input
    buffer of a forward plan)."""
    h, w, c = image.shape
    n = rot_tf.shape[0]
    if rot_tf.shape != (n, 8) or trans_tf.shape != (n, 8):
        raise AsrError("augment_copies: transforms must be [N,8]")
    if out is None:
        out = torch.empty((n, h, w, c), dtype=f32, device=image.device)
    elif tuple(out.shape) != (n, h, w, c):
        raise AsrError(f"augment_copies: out must be [{n},{h},{w},{c}], got {tuple(out.shape)}")
    call("asr_augment_copies_f32", ptr(image), ptr(out), ptr(rot_tf), ptr(trans_tf), n, h, w, c, stream_ptr())
    return out


# ---------------------------------------------------------------------------------------------
# SR
# ---------------------------------------------------------------------------------------------
def _sr_dims(x, y):
    if x.dim() != 3 or y.dim() != 4 or x.shape[0] != y.shape[0]:
        raise AsrError(f"SR tensors: x [B,H,W] and y [B,N,h,w] expected, got {tuple(x.shape)} {tuple(y.shape)}")
    b, H, W = x.shape
    _, n, h, w = y.shape
    return b, n, H, W, h, w


def _check_tf(t, b, n, name):
    if tuple(t.shape) != (b, n, 8):
        raise AsrError(f"{name} must be [{b},{n},8], got {tuple(t.shape)}")


def sr_init_target(y, out_hw):
    b, n, h, w = y.shape
    x = torch.empty((b, out_hw[0], out_hw[1]), dtype=f32, device=y.device)
    call("asr_sr_init_target_f32", ptr(y), ptr(x), b, n, out_hw[0], out_hw[1], h, w, stream_ptr())
    return x


def check_data_term(loss, delta=0.1, name="data term"):
    """The data term's loss -> (ASR_DF_* code, delta): loss "l2", "l1" or "huber" (None is "l2"); under Huber delta must be
    a finite number > 0, elsewhere it is not read.  Host check, before any launch (include/asr_hip.h: the rule)."""
    import numbers
    if loss is None:
        loss = "l2"
    if not isinstance(loss, str) or loss.lower() not in _lib.DF_LOSSES:
        raise ValueError(f"{name}: loss must be one of {sorted(_lib.DF_LOSSES)}, got {loss!r}")
    code = _lib.DF_LOSSES[loss.lower()]
    if code != _lib.DF_HUBER:
        return code, 0.0
    ok = isinstance(delta, numbers.Real) and not isinstance(delta, bool) and np.isfinite(float(delta)) and float(delta) > 0.0
    if not ok:
        raise ValueError(f"{name}: Huber delta must be a finite number > 0, got {delta!r}")
    return code, float(delta)


def _data_term(data_term, weights, y, tvw, name, always=False):
    """data_term (None, a loss name, or a pair (loss, delta)) + weights ([N,h,w] shared by the batch or [B,N,h,w], on the device
    of y) + the checked tv_weights -> the asr_sr_data_term of a *_dt call, or None when the call that ran before data terms
    existed computes the same thing (L2, no weights; always=True: the struct then too, for the monitored solve, which has
    the *_dt form only).  The struct keeps its tensors alive."""
    if isinstance(data_term, (tuple, list)):
        if len(data_term) != 2:
            raise ValueError(f"{name}: data_term must be a loss name or a pair (loss, delta), got {data_term!r}")
        code, delta = check_data_term(data_term[0], data_term[1], name)
    else:
        code, delta = check_data_term(data_term, name=name)
    if weights is None and code == _lib.DF_L2 and not always:
        return None
    shared = 0
    if weights is not None:
        b, n, h, w = y.shape
        if not isinstance(weights, torch.Tensor) or weights.dtype != f32 or not weights.is_contiguous() or weights.device != y.device:
            raise AsrError(f"{name}: weights must be a contiguous float32 tensor on the device of the copies")
        if tuple(weights.shape) not in ((n, h, w), (b, n, h, w)):
            raise AsrError(f"{name}: weights must be [{n},{h},{w}] (shared) or [{b},{n},{h},{w}], got {tuple(weights.shape)}")
        shared = int(weights.dim() == 3)
    dt = _lib.SrDataTerm(code, delta, ptr(weights, allow_none=True), shared, ptr(tvw[0]) if tvw else None,
                         ptr(tvw[1]) if tvw else None, tvw[2] if tvw else 0)
    dt._keep = (weights, tvw)
    return dt


def sr_forward_residual(x, y, rot_tf, trans_tf, data_term=None, weights=None, want_raw=False):
    """The residual r = D(T(R(x))) - y, or under a data term q = w * psi(r), what the backward calls take as `resid`
    (include/asr_hip.h: the rule).  want_raw: the pair (q, r), from one launch."""
    b, n, H, W, h, w = _sr_dims(x, y)
    _check_tf(rot_tf, b, n, "rot_tf")
    _check_tf(trans_tf, b, n, "trans_tf")
    dt = _data_term(data_term, weights, y, None, "sr_forward_residual")
    resid = torch.empty_like(y)
    if dt is None:
        call("asr_sr_forward_residual_f32", ptr(x), ptr(y), ptr(rot_tf), ptr(trans_tf), ptr(resid), b, n, H, W, h, w,
             stream_ptr())
        return (resid, resid) if want_raw else resid
    raw = torch.empty_like(y) if want_raw else None
    call("asr_sr_forward_residual_dt_f32", ptr(x), ptr(y), ptr(rot_tf), ptr(trans_tf), ptr(resid), ptr(raw, allow_none=True),
         b, n, H, W, h, w, C.byref(dt), stream_ptr())
    return (resid, raw) if want_raw else resid


def sr_config(optimizer=_lib.OPT_ADAM, flag=False, c0=0.0, c1=0.0, c2=0.0, use_btv=False, btv_alpha=0.6, btv_shift=2,
              plane_chunk=0):
    """asr_sr_config for the *_cfg entry points (meaning of c0..c2 per optimizer: include/asr_hip.h).  plane_chunk: copies
    whose gradient planes the solver keeps alive at once (0 = library default: all of them up to 1 GiB of planes; results
    do not depend on it)."""
    return _lib.SrConfig(int(optimizer), int(bool(flag)), float(c0), float(c1), float(c2),
                         _lib.PRIOR_BTV if use_btv else _lib.PRIOR_TV, float(btv_alpha), int(btv_shift), int(plane_chunk))


def _adam_config(one_minus_beta1, one_minus_beta2, epsilon, amsgrad):
    return sr_config(_lib.OPT_ADAM, amsgrad, one_minus_beta1, one_minus_beta2, epsilon)


PD_DUAL_RATIO = 1.0 / 16.0          # the largest dual ratio of ASR_OPT_PRIMAL_DUAL, and the one its step rule is derived for


def check_pd(bound_iters=6, dual_ratio=PD_DUAL_RATIO, name="primal-dual"):
    """The two parameters of the primal-dual rule -> (int, float): bound_iters an integer in 1..64, dual_ratio a finite number
    in (0, 1/16].  Host check, before any launch (include/asr_hip.h: the rule)."""
    import numbers
    if not isinstance(bound_iters, numbers.Integral) or isinstance(bound_iters, bool) or not 1 <= int(bound_iters) <= _lib.MAX_BOUND_ITERS:
        raise ValueError(f"{name}: bound iterations must be an integer in 1..{_lib.MAX_BOUND_ITERS}, got {bound_iters!r}")
    ok = isinstance(dual_ratio, numbers.Real) and not isinstance(dual_ratio, bool) and np.isfinite(float(dual_ratio)) \
        and 0.0 < float(np.float32(dual_ratio)) <= PD_DUAL_RATIO
    if not ok:
        raise ValueError(f"{name}: dual ratio must be a finite number in (0, 1/16], got {dual_ratio!r}")
    return int(bound_iters), float(dual_ratio)


def check_adjoint(name, what="adjoint"):
    """The data-term gradient's form -> ASR_ADJ_* code: "registered" (None too: TensorFlow's registered gradient of the rotate,
    an inverse warp) or "exact" (the transpose of the forward rotate; include/asr_hip.h, "exact adjoint").  Host check, before
    any launch."""
    if name is None:
        return _lib.ADJ_REGISTERED
    if not isinstance(name, str) or name.lower() not in _lib.ADJOINTS:
        raise ValueError(f"{what}: must be one of {sorted(_lib.ADJOINTS)}, got {name!r}")
    return _lib.ADJOINTS[name.lower()]


def sr_adjoint_flags(rot_tf, trans_tf, inv_rot_tf):
    """device int32 [B]: 1 where the exact adjoint applies to the image (affine rotations, pure translations, a window the
    kernel serves), 0 where adjoint="exact" takes the registered statements (include/asr_hip.h, "exact adjoint")."""
    if rot_tf.dim() != 3 or rot_tf.shape[-1] != 8:
        raise AsrError(f"sr_adjoint_flags: transforms must be [B,N,8], got {tuple(rot_tf.shape)}")
    b, n = rot_tf.shape[:2]
    for t, name in ((rot_tf, "rot_tf"), (trans_tf, "trans_tf"), (inv_rot_tf, "inv_rot_tf")):
        _check_tf(t, b, n, name)
    flags = torch.empty((b,), dtype=torch.int32, device=rot_tf.device)
    call("asr_sr_adjoint_flags_i32", ptr(rot_tf), ptr(trans_tf), ptr(inv_rot_tf), ptr(flags, torch.int32), b, n, stream_ptr())
    return flags


def sr_data_bound(rot_tf, trans_tf, inv_rot_tf, inv_trans_tf, out_hw, lr_hw, lambda_df, weights=None, iters=6, cfg=None,
                  adjoint=None):
    """device [B]: an upper bound on the spectral radius of the data term's gradient map, the step bound of the primal-dual
    rule (include/asr_hip.h, "primal-dual").  The transforms [B,N,8] of the solve, out_hw = (H, W), lr_hw = (h, w); weights:
    the data term's, [N,h,w] shared or [B,N,h,w]; cfg: its plane_chunk alone is read.  Nothing is read back.
    adjoint="exact": the map of the exact gradient, symmetric, for which the bound is a bound (asr_sr_data_bound_adj_f32);
    None: the call below, unchanged."""
    adj = check_adjoint(adjoint, "sr_data_bound: adjoint") if adjoint is not None else None
    iters, _ = check_pd(iters, name="sr_data_bound")
    if rot_tf.dim() != 3 or rot_tf.shape[-1] != 8:
        raise AsrError(f"sr_data_bound: transforms must be [B,N,8], got {tuple(rot_tf.shape)}")
    b, n = rot_tf.shape[:2]
    for t, name in ((rot_tf, "rot_tf"), (trans_tf, "trans_tf"), (inv_rot_tf, "inv_rot_tf"), (inv_trans_tf, "inv_trans_tf")):
        _check_tf(t, b, n, name)
    (H, W), (h, w) = (int(v) for v in out_hw), (int(v) for v in lr_hw)
    shared = 0
    if weights is not None:
        if not isinstance(weights, torch.Tensor) or weights.dtype != f32 or not weights.is_contiguous() or weights.device != rot_tf.device:
            raise AsrError("sr_data_bound: weights must be a contiguous float32 tensor on the device of the transforms")
        if tuple(weights.shape) not in ((n, h, w), (b, n, h, w)):
            raise AsrError(f"sr_data_bound: weights must be [{n},{h},{w}] (shared) or [{b},{n},{h},{w}], got {tuple(weights.shape)}")
        shared = int(weights.dim() == 3)
    cfg = cfg if cfg is not None else sr_config()
    ws_bytes = _lib.load().asr_sr_data_bound_workspace_bytes(b, n, H, W, h, w, C.byref(cfg))
    ws = torch.empty((ws_bytes + 3) // 4, dtype=f32, device=rot_tf.device)
    bound = torch.empty((b,), dtype=f32, device=rot_tf.device)
    if adj is not None:
        call("asr_sr_data_bound_adj_f32", ptr(bound), ptr(rot_tf), ptr(trans_tf), ptr(inv_rot_tf), ptr(inv_trans_tf),
             ptr(weights, allow_none=True), shared, iters, ptr(ws), C.c_size_t(ws_bytes), b, n, H, W, h, w, float(lambda_df),
             C.byref(cfg), adj, stream_ptr())
        return bound
    call("asr_sr_data_bound_f32", ptr(bound), ptr(rot_tf), ptr(trans_tf), ptr(inv_rot_tf), ptr(inv_trans_tf),
         ptr(weights, allow_none=True), shared, iters, ptr(ws), C.c_size_t(ws_bytes), b, n, H, W, h, w, float(lambda_df),
         C.byref(cfg), stream_ptr())
    return bound


def pd_steps(bound, lambda_l2, num_iter):
    """device [num_iter, B]: the alphas of a primal-dual solve, tau = 1 / (bound + 2 lambda_l2) in float32 for every iteration,
    0 where that denominator is 0.  Built on the device of bound; nothing is read back."""
    if not isinstance(bound, torch.Tensor) or bound.dtype != f32 or bound.dim() != 1:
        raise AsrError("pd_steps: bound must be a float32 tensor [B]")
    den = bound + float(np.float32(2.0) * np.float32(lambda_l2))
    tau = torch.where(den != 0, 1.0 / den, torch.zeros_like(den))
    return tau[None].expand(int(num_iter), -1).contiguous()


def check_tv_beta(beta, name="tv_edge_weights"):
    """beta of the edge weights: a finite number >= 0 (host check, before any launch)."""
    import numbers
    ok = isinstance(beta, numbers.Real) and not isinstance(beta, bool) and np.isfinite(float(beta)) and float(beta) >= 0.0
    if not ok:
        raise ValueError(f"{name}: beta must be a finite number >= 0, got {beta!r}")
    return float(beta)


def tv_edge_weights(guide, beta):
    """guide [H,W,3] or [B,H,W,3] (RGB in [0, 1]) -> (wy, wx), each [H,W] or [B,H,W]: the edge weights of the weighted TV
    prior, w = 1 / (1 + beta * |forward difference of the guide|^2), 1 in the last row (wy) / column (wx)
    (include/asr_hip.h: the rule)."""
    beta = check_tv_beta(beta)
    if not isinstance(guide, torch.Tensor) or guide.dim() not in (3, 4) or guide.shape[-1] != 3:
        raise AsrError(f"tv_edge_weights: guide must be a [H,W,3] or [B,H,W,3] tensor, got "
                       f"{tuple(guide.shape) if hasattr(guide, 'shape') else type(guide).__name__}")
    if guide.dtype != f32 or not guide.is_contiguous():
        raise AsrError("tv_edge_weights: guide must be contiguous float32")
    shape = tuple(guide.shape[:-1])
    if min(shape) < 1:
        raise AsrError(f"tv_edge_weights: empty guide {tuple(guide.shape)}")
    b = shape[0] if guide.dim() == 4 else 1
    wy = torch.empty(shape, dtype=f32, device=guide.device)
    wx = torch.empty(shape, dtype=f32, device=guide.device)
    call("asr_tv_edge_weights_f32", ptr(guide), ptr(wy), ptr(wx), b, shape[-2], shape[-1], beta, stream_ptr())
    return wy, wx


def _tv_weights(tv_weights, x, name):
    """(wy, wx) of a weighted-TV call -> (wy, wx, shared): [H,W] planes are shared by the batch, [B,H,W] are per image."""
    if not isinstance(tv_weights, (tuple, list)) or len(tv_weights) != 2:
        raise AsrError(f"{name}: tv_weights must be a pair (wy, wx)")
    wy, wx = tv_weights
    b, H, W = x.shape
    for t, nm in ((wy, "wy"), (wx, "wx")):
        if not isinstance(t, torch.Tensor) or t.dtype != f32 or not t.is_contiguous() or t.device != x.device:
            raise AsrError(f"{name}: tv_weights {nm} must be a contiguous float32 tensor on the device of x")
    if tuple(wy.shape) != tuple(wx.shape) or tuple(wy.shape) not in ((H, W), (b, H, W)):
        raise AsrError(f"{name}: tv_weights must both be [{H},{W}] (shared) or [{b},{H},{W}], got {tuple(wy.shape)} "
                       f"{tuple(wx.shape)}")
    return wy, wx, int(wy.dim() == 2)


def sr_backward(x, resid, inv_rot_tf, inv_trans_tf, lambdas, cfg, state=None, want_grad=False, tv_weights=None, rot_tf=None,
                trans_tf=None, adjoint=None):
    """One step with the update rule / prior of cfg.  state = dict(m, v, vhat, alphas[B]) (slots the optimizer
    does not use may be None) or None for the gradient only.  tv_weights = (wy, wx): the edge-weighted TV prior
    (tv_edge_weights, or any finite weights >= 0).  Returns (x_new | None, grad | None).
    adjoint ("registered" / "exact", with rot_tf and trans_tf [B,N,8]): the call goes through asr_sr_backward_adj_f32, whose
    exact form takes the data-term gradient as the transpose of the forward rotate (include/asr_hip.h, "exact adjoint").
    None: the calls below, unchanged."""
    b, n, H, W, h, w = _sr_dims(x, resid)
    adj = check_adjoint(adjoint, "sr_backward: adjoint") if adjoint is not None else None
    if adj is not None:
        if rot_tf is None or trans_tf is None:
            raise AsrError("sr_backward: adjoint needs rot_tf and trans_tf")
        _check_tf(rot_tf, b, n, "rot_tf")
        _check_tf(trans_tf, b, n, "trans_tf")
    tvw = _tv_weights(tv_weights, x, "sr_backward") if tv_weights is not None else None
    _check_tf(inv_rot_tf, b, n, "inv_rot_tf")
    _check_tf(inv_trans_tf, b, n, "inv_trans_tf")
    grad = torch.empty_like(x) if (want_grad or state is None) else None
    x_new = torch.empty_like(x) if state is not None else None
    st = state or {}
    if state is not None:
        for k in ("m", "v", "vhat"):
            if st.get(k) is not None and st[k].shape != x.shape:
                raise AsrError(f"state['{k}'] shape mismatch")
        if st["alphas"].numel() != b:
            raise AsrError("state['alphas'] must hold one value per image")
    args = (ptr(x), ptr(x_new, allow_none=True), ptr(resid), ptr(inv_rot_tf),
            ptr(inv_trans_tf), ptr(st.get("m"), allow_none=True), ptr(st.get("v"), allow_none=True),
            ptr(st.get("vhat"), allow_none=True), ptr(st.get("alphas"), allow_none=True), ptr(grad, allow_none=True),
            b, n, H, W, h, w, float(lambdas[0]), float(lambdas[1]), float(lambdas[2]), float(lambdas[3]), C.byref(cfg))
    if adj is not None:
        ws_bytes = _lib.load().asr_sr_backward_adj_workspace_bytes(b, n, H, W, C.byref(cfg)) if adj == _lib.ADJ_EXACT else 0
        ws = torch.empty((ws_bytes + 3) // 4, dtype=f32, device=x.device) if ws_bytes else None
        call("asr_sr_backward_adj_f32", *args[:3], ptr(rot_tf), ptr(trans_tf), *args[3:],
             ptr(tvw[0]) if tvw else None, ptr(tvw[1]) if tvw else None, tvw[2] if tvw else 0, adj,
             ptr(ws, allow_none=True), C.c_size_t(ws_bytes), stream_ptr())
        return x_new, grad
    if tvw is None:
        call("asr_sr_backward_cfg_f32", *args, stream_ptr())
    else:
        call("asr_sr_backward_wtv_f32", *args, ptr(tvw[0]), ptr(tvw[1]), tvw[2], stream_ptr())
    return x_new, grad


def sr_backward_adam(x, resid, inv_rot_tf, inv_trans_tf, lambdas, adam=None, want_grad=False):
    """One Adam / AMSGrad step with the TV prior.  adam = dict(m, v, vhat, alphas[B], one_minus_beta1,
    one_minus_beta2, epsilon, amsgrad) or None for gradient only.  Returns (x_new | None, grad | None)."""
    b, n, H, W, h, w = _sr_dims(x, resid)
    _check_tf(inv_rot_tf, b, n, "inv_rot_tf")
    _check_tf(inv_trans_tf, b, n, "inv_trans_tf")
    grad = torch.empty_like(x) if (want_grad or adam is None) else None
    x_new = torch.empty_like(x) if adam is not None else None
    if adam is not None:
        for k in ("m", "v"):
            if adam[k].shape != x.shape:
                raise AsrError(f"adam['{k}'] shape mismatch")
        if adam["alphas"].numel() != b:
            raise AsrError("adam['alphas'] must hold one value per image")
    a = adam or {}
    call("asr_sr_backward_adam_f32", ptr(x), ptr(x_new, allow_none=True), ptr(resid), ptr(inv_rot_tf),
         ptr(inv_trans_tf), ptr(a.get("m"), allow_none=True), ptr(a.get("v"), allow_none=True),
         ptr(a.get("vhat"), allow_none=True), ptr(a.get("alphas"), allow_none=True), ptr(grad, allow_none=True),
         b, n, H, W, h, w, float(lambdas[0]), float(lambdas[1]), float(lambdas[2]), float(lambdas[3]),
         float(a.get("one_minus_beta1", 0.0)), float(a.get("one_minus_beta2", 0.0)), float(a.get("epsilon", 0.0)),
         int(bool(a.get("amsgrad", False))), stream_ptr())
    return x_new, grad


def sr_loss_terms(x, resid, cfg=None, tv_weights=None, data_term=None, weights=None):
    """[B,4] float64 {sum resid^2, TV or bilateral TV (cfg) or the edge-weighted TV (tv_weights), sum x^2, sum |x|}.
    Under a data term (data_term, weights: as for sr_forward_residual) resid is the RAW residual and the first entry is
    sum weights * rho(resid)."""
    b, n, H, W, h, w = _sr_dims(x, resid)
    tvw = _tv_weights(tv_weights, x, "sr_loss_terms") if tv_weights is not None else None
    dt = _data_term(data_term, weights, resid, tvw, "sr_loss_terms")
    terms = torch.empty((b, 4), dtype=torch.float64, device=x.device)
    if dt is not None:
        call("asr_sr_loss_terms_dt_f64", ptr(x), ptr(resid), ptr(terms, torch.float64), b, n, H, W, h, w,
             C.byref(cfg if cfg is not None else sr_config()), C.byref(dt), stream_ptr())
    elif tvw is not None:
        call("asr_sr_loss_terms_wtv_f64", ptr(x), ptr(resid), ptr(terms, torch.float64), b, n, H, W, h, w,
             C.byref(cfg if cfg is not None else sr_config()), ptr(tvw[0]), ptr(tvw[1]), tvw[2], stream_ptr())
    elif cfg is None:
        call("asr_sr_loss_terms_f64", ptr(x), ptr(resid), ptr(terms, torch.float64), b, n, H, W, h, w, stream_ptr())
    else:
        call("asr_sr_loss_terms_cfg_f64", ptr(x), ptr(resid), ptr(terms, torch.float64), b, n, H, W, h, w, C.byref(cfg),
             stream_ptr())
    return terms


SR_MONITOR_DEFAULTS = dict(every=1, rel_tol=1e-4, patience=3, min_iter=0, history=True)


def check_sr_monitor(params, name="sr monitor"):
    """The monitor of a solve (include/asr_hip.h: asr_sr_monitor) as a complete dict: a mapping with any of the keys every
    (int >= 1), rel_tol (finite number >= 0), patience (int >= 0; 0 = never stop), min_iter (int >= 0) and history (bool),
    the others from SR_MONITOR_DEFAULTS.  Host only; ValueError on anything else."""
    import numbers
    if not isinstance(params, dict):
        raise ValueError(f"{name}: a dict with keys among {sorted(SR_MONITOR_DEFAULTS)} expected, got {params!r}")
    unknown = sorted(set(params) - set(SR_MONITOR_DEFAULTS))
    if unknown:
        raise ValueError(f"{name}: unknown keys {unknown} (known: {sorted(SR_MONITOR_DEFAULTS)})")
    p = dict(SR_MONITOR_DEFAULTS, **params)
    for key, low in (("every", 1), ("patience", 0), ("min_iter", 0)):
        v = p[key]
        if not isinstance(v, numbers.Integral) or isinstance(v, bool) or not low <= int(v) < 2 ** 31:
            raise ValueError(f"{name}: {key} must be an integer >= {low}, got {v!r}")
        p[key] = int(v)
    t = p["rel_tol"]
    if not isinstance(t, numbers.Real) or isinstance(t, bool) or not np.isfinite(float(t)) or float(t) < 0.0:
        raise ValueError(f"{name}: rel_tol must be a finite number >= 0, got {t!r}")
    p["rel_tol"] = float(t)
    if not isinstance(p["history"], (bool, np.bool_)):
        raise ValueError(f"{name}: history must be True or False, got {p['history']!r}")
    p["history"] = bool(p["history"])
    return p


def check_coupling(coupling, batch=None, cfg=None, name="coupling"):
    """The group size of a coupled solve (include/asr_hip.h, "multi-label coupling") as an int: an integer in
    0.._lib.MAX_CLASS_SET (0: the entry point runs the uncoupled solve); with batch, a divisor of it; with cfg, G >= 1 needs the
    primal-dual rule.  Host only; ValueError on anything else."""
    if not isinstance(coupling, numbers.Integral) or isinstance(coupling, bool) or not 0 <= int(coupling) <= _lib.MAX_CLASS_SET:
        raise ValueError(f"{name}: an integer in 0..{_lib.MAX_CLASS_SET} expected, got {coupling!r}")
    g = int(coupling)
    if g >= 1 and batch is not None and int(batch) % g != 0:
        raise ValueError(f"{name}: the batch of {batch} planes is no multiple of the group size {g}")
    if g >= 1 and (cfg is None or cfg.optimizer != _lib.OPT_PRIMAL_DUAL):
        raise ValueError(f"{name}: the coupled solve needs the primal-dual rule (sr_config(optimizer=_lib.OPT_PRIMAL_DUAL))")
    return g


def simplex_project(x, group):
    """x [B, ...] float32, B a multiple of group: every pixel's `group` values of each run of `group` consecutive planes are
    projected onto {v >= 0, sum v <= 1}, in place (asr_simplex_project_f32; the rule: include/asr_hip.h).  Returns x."""
    if x.dim() < 2 or x.shape[0] == 0 or x.numel() == 0:
        raise AsrError(f"simplex_project: x must be [B, ...] with B >= 1, got {tuple(x.shape)}")
    if not isinstance(group, numbers.Integral) or isinstance(group, bool) or int(group) < 1 or x.shape[0] % int(group):
        raise AsrError(f"simplex_project: group must be an integer >= 1 that divides the {x.shape[0]} planes, got {group!r}")
    call("asr_simplex_project_f32", ptr(x), x.shape[0] // int(group), int(group), x.numel() // x.shape[0], stream_ptr())
    return x


def sr_loss_from_terms(terms, lambdas):
    """The scalar loss of the monitor from its four terms [..., 4], in float64: ((l_df*t0 + l_tv*t1) + l_L2*t2), then
    + l_L1*t3 only when l_L1 > 0, the lambdas the float32 arguments widened, every operation rounding by itself."""
    t = np.asarray(terms, dtype=np.float64)
    l = [np.float64(np.float32(v)) for v in lambdas]
    loss = (l[0] * t[..., 0] + l[1] * t[..., 1]) + l[2] * t[..., 2]
    if l[3] > 0.0:
        loss = loss + l[3] * t[..., 3]
    return loss


class SrTrace:
    """What a monitored solve leaves behind.  history: device float64 [E, B, 4], the four loss terms of every image at
    every evaluation (NaN after the image stopped), or None; eval_iters: the E iterations that were evaluations;
    iters_done: device int32 [B], the updates applied to each image.  Reading either tensor on the host synchronises."""

    def __init__(self, history, eval_iters, iters_done):
        self.history, self.eval_iters, self.iters_done = history, list(eval_iters), iters_done

    def losses(self, lambdas):
        """numpy float64 [E, B]: the scalar loss the stop rule saw at every evaluation (sr_loss_from_terms)."""
        if self.history is None:
            raise AsrError("SrTrace.losses: the solve kept no history (monitor history=False)")
        return sr_loss_from_terms(self.history.cpu().numpy(), lambdas)


SR_REWEIGHT_DEFAULTS = dict(kind="cauchy", kappa=2.0, every=10, start=10, history=False)


def check_sr_reweight(params, name="sr reweight"):
    """The copy reweighting of a solve (include/asr_hip.h: asr_sr_reweight) as a complete dict: a mapping with any of the keys
    kind ("cauchy" or "hard"), kappa (finite number > 0), every (int >= 1), start (int >= 0) and history (bool), the others from
    SR_REWEIGHT_DEFAULTS; a bare kind name stands for dict(kind=name).  Host only; ValueError on anything else."""
    if isinstance(params, str):
        params = dict(kind=params)
    if not isinstance(params, dict):
        raise ValueError(f"{name}: a dict with keys among {sorted(SR_REWEIGHT_DEFAULTS)} expected, got {params!r}")
    unknown = sorted(set(params) - set(SR_REWEIGHT_DEFAULTS))
    if unknown:
        raise ValueError(f"{name}: unknown keys {unknown} (known: {sorted(SR_REWEIGHT_DEFAULTS)})")
    p = dict(SR_REWEIGHT_DEFAULTS, **params)
    if not isinstance(p["kind"], str) or p["kind"].lower() not in _lib.RW_KINDS:
        raise ValueError(f"{name}: kind must be one of {sorted(_lib.RW_KINDS)}, got {p['kind']!r}")
    p["kind"] = p["kind"].lower()
    k = p["kappa"]
    if not isinstance(k, numbers.Real) or isinstance(k, bool) or not np.isfinite(float(k)) or float(k) <= 0.0:
        raise ValueError(f"{name}: kappa must be a finite number > 0, got {k!r}")
    p["kappa"] = float(k)
    for key, low in (("every", 1), ("start", 0)):
        v = p[key]
        if not isinstance(v, numbers.Integral) or isinstance(v, bool) or not low <= int(v) < 2 ** 31:
            raise ValueError(f"{name}: {key} must be an integer >= {low}, got {v!r}")
        p[key] = int(v)
    if not isinstance(p["history"], (bool, np.bool_)):
        raise ValueError(f"{name}: history must be True or False, got {p['history']!r}")
    p["history"] = bool(p["history"])
    return p


def sr_reweight_iters(params, num_iter):
    """The iterations below num_iter at which a solve under check_sr_reweight's dict reweights."""
    return list(range(params["start"], int(num_iter), params["every"]))


class SrCopyWeights:
    """What a reweighted solve leaves behind.  weights: device float32 [B, N], the last weight of every copy (1 where the solve
    never reweighted); history: device float32 [R, B, N], the weights after each of the R reweightings (NaN for an image the
    monitor had stopped), or None; iters: the R iterations that reweighted.  Reading a tensor on the host synchronises."""

    def __init__(self, weights, history, iters):
        self.weights, self.history, self.iters = weights, history, list(iters)


def _rw_residual(r, name):
    if not isinstance(r, torch.Tensor) or r.dim() != 4 or r.dtype != f32 or not r.is_contiguous() or r.numel() == 0:
        raise AsrError(f"{name}: r must be a contiguous float32 tensor [B,N,h,w]")
    if r.shape[1] > _lib.RW_MAX_COPIES:
        raise AsrError(f"{name}: at most {_lib.RW_MAX_COPIES} copies, got {r.shape[1]}")
    return tuple(r.shape)


def sr_copy_energy(r, data_term=None, weights=None):
    """r [B,N,h,w], the RAW residual (sr_forward_residual's second output) -> (energy, mass), float64 [B,N]: per copy
    sum weights * rho(r) and sum weights (h*w without weights), in the fixed order of include/asr_hip.h, "copy reweighting"."""
    b, n, h, w = _rw_residual(r, "sr_copy_energy")
    dt = _data_term(data_term, weights, r, None, "sr_copy_energy", always=True)
    energy = torch.empty((b, n), dtype=torch.float64, device=r.device)
    mass = torch.empty((b, n), dtype=torch.float64, device=r.device)
    call("asr_sr_copy_energy_f64", ptr(r), C.byref(dt), ptr(energy, torch.float64), ptr(mass, torch.float64), b, n, h, w,
         stream_ptr())
    return energy, mass


def sr_copy_weights(energy, mass, kind="cauchy", kappa=2.0, want_scale=False):
    """energy, mass float64 [B,N] -> the copy weights c, float32 [B,N] (and, want_scale, the scale s, float64 [B]): each copy's
    energy per unit mass against kappa times the lower median over the active copies of its image (include/asr_hip.h)."""
    p = check_sr_reweight(dict(kind=kind, kappa=kappa), "sr_copy_weights")
    for t in (energy, mass):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype != torch.float64 or not t.is_contiguous() or t.numel() == 0:
            raise AsrError("sr_copy_weights: energy and mass must be contiguous float64 tensors [B,N]")
    if energy.shape != mass.shape or energy.device != mass.device:
        raise AsrError(f"sr_copy_weights: energy {tuple(energy.shape)} and mass {tuple(mass.shape)} differ")
    b, n = energy.shape
    if n > _lib.RW_MAX_COPIES:
        raise AsrError(f"sr_copy_weights: at most {_lib.RW_MAX_COPIES} copies, got {n}")
    c = torch.empty((b, n), dtype=f32, device=energy.device)
    scale = torch.empty((b,), dtype=torch.float64, device=energy.device) if want_scale else None
    call("asr_sr_copy_weights_f32", ptr(energy, torch.float64), ptr(mass, torch.float64), _lib.RW_KINDS[p["kind"]], p["kappa"],
         ptr(c), ptr(scale, torch.float64, allow_none=True), b, n, stream_ptr())
    return (c, scale) if want_scale else c


def sr_apply_copy_weights(r, c, data_term=None, weights=None):
    """r [B,N,h,w] (raw residual), c [B,N] -> (w_eff, q), each [B,N,h,w]: w_eff = weights * c (c without weights) and
    q = w_eff * psi(r), bit for bit what sr_forward_residual(..., weights=w_eff) returns for the x that gave r."""
    b, n, h, w = _rw_residual(r, "sr_apply_copy_weights")
    if not isinstance(c, torch.Tensor) or tuple(c.shape) != (b, n) or c.dtype != f32 or not c.is_contiguous() or c.device != r.device:
        raise AsrError(f"sr_apply_copy_weights: c must be a contiguous float32 tensor [{b},{n}] on the device of r")
    dt = _data_term(data_term, weights, r, None, "sr_apply_copy_weights", always=True)
    w_eff = torch.empty_like(r)
    q = torch.empty_like(r)
    call("asr_sr_apply_copy_weights_f32", ptr(r), C.byref(dt), ptr(c), ptr(w_eff), ptr(q), b, n, h, w, stream_ptr())
    return w_eff, q


def sr_solve(x, y, rot_tf, trans_tf, inv_rot_tf, inv_trans_tf, alphas, lambdas, one_minus_beta1=None, one_minus_beta2=None,
             epsilon=None, amsgrad=False, want_loss=True, cfg=None, slot_init=None, state=None, tv_weights=None,
             data_term=None, weights=None, monitor=None, coupling=None, reweight=None, adjoint=None):
    """Runs alphas.shape[0] iterations in place on x.  alphas [num_iter, B] (device).  Either the Adam
    hyper-parameters (asr_sr_solve_f32) or cfg (+ slot_init = {"m"/"v"/"vhat": initial value}) for
    asr_sr_solve_cfg_f32.  state: a dict that carries the optimiser slots and the workspace from one call to the next --
    a solve cut into several calls (the verbose loss print-outs) then performs exactly the updates of a single call.
    tv_weights = (wy, wx): the edge-weighted TV prior; with the Adam hyper-parameters instead of cfg the call goes through
    the equivalent {Adam, TV} config.  data_term, weights: the data term sum weights * rho(r) (sr_forward_residual; combines
    freely with tv_weights); with L2 / None and no weights the calls above are made, unchanged.
    monitor (check_sr_monitor's dict): the solve goes through asr_sr_solve_mon_f32 -- the loss terms of every `every`-th
    iteration, each image stopped by itself when its loss stalls (include/asr_hip.h: the rule) -- and the return value is
    (x, terms, SrTrace); nothing is read back here.  Without it: the calls and the pair above, unchanged.
    cfg with _lib.OPT_PRIMAL_DUAL (sr_config(optimizer=_lib.OPT_PRIMAL_DUAL, c0=1/16)): alphas are the steps tau of pd_steps,
    the slots m and v come back as the dual planes p_y and p_x (include/asr_hip.h, "primal-dual").
    coupling = G (check_coupling; primal-dual only): the batch is groups of G consecutive planes, the classes of one image, and
    every iteration ends in the projection of each pixel's G values onto {x >= 0, sum <= 1}; a monitor then stops a group as a
    whole (include/asr_hip.h, "multi-label coupling"; asr_sr_solve_ml_f32).  None: the calls below, unchanged.
    reweight (check_sr_reweight's dict, or a kind name): every `every` iterations from `start` each copy's residual energy is
    compared with the median over the copies of its image and the whole copy is scaled by a robust weight, on top of `weights`
    (include/asr_hip.h, "copy reweighting"; asr_sr_solve_rw_f32); combines with everything above.  The return value gains one
    last element, an SrCopyWeights.  None: the calls below and their return values, unchanged.
    adjoint ("registered" / "exact"): the solve goes through asr_sr_solve_adj_f32; "exact" takes the data-term gradient as the
    transpose of the forward rotate instead of TensorFlow's registered inverse warp (include/asr_hip.h, "exact adjoint") and
    combines with everything above; return values are those of the same call without it.  None: the calls below, unchanged."""
    b, n, H, W, h, w = _sr_dims(x, y)
    adj = check_adjoint(adjoint, "sr_solve: adjoint") if adjoint is not None else None
    rwp = check_sr_reweight(reweight, "sr_solve: reweight") if reweight is not None else None
    if rwp is not None and n > _lib.RW_MAX_COPIES:
        raise AsrError(f"sr_solve: reweight ranks at most {_lib.RW_MAX_COPIES} copies, got {n}")
    group = None if coupling is None else check_coupling(coupling, b, cfg, "sr_solve: coupling")
    mon = check_sr_monitor(monitor, "sr_solve: monitor") if monitor is not None else None
    tvw = _tv_weights(tv_weights, x, "sr_solve") if tv_weights is not None else None
    dt = _data_term(data_term, weights, y, tvw, "sr_solve", always=mon is not None or group is not None or rwp is not None or adj is not None)
    if (tvw is not None or dt is not None) and cfg is None:
        cfg = _adam_config(one_minus_beta1, one_minus_beta2, epsilon, amsgrad)
    for t, name in ((rot_tf, "rot_tf"), (trans_tf, "trans_tf"), (inv_rot_tf, "inv_rot_tf"), (inv_trans_tf, "inv_trans_tf")):
        _check_tf(t, b, n, name)
    if alphas.dim() != 2 or alphas.shape[1] != b:
        raise AsrError(f"alphas must be [num_iter,{b}]")
    num_iter = alphas.shape[0]
    lib = _lib.load()
    ws_bytes = (lib.asr_sr_solve_workspace_bytes_rw(b, n, H, W, h, w, C.byref(cfg), int(mon is not None)) if rwp is not None else
                lib.asr_sr_solve_workspace_bytes_ml(b, n, H, W, h, w, C.byref(cfg), int(mon is not None)) if group is not None else
                lib.asr_sr_solve_workspace_bytes_mon(b, n, H, W, h, w, C.byref(cfg)) if mon is not None else
                lib.asr_sr_solve_workspace_bytes(b, n, H, W, h, w) if cfg is None else
                lib.asr_sr_solve_workspace_bytes_dt(b, n, H, W, h, w, C.byref(cfg)) if dt is not None else
                lib.asr_sr_solve_workspace_bytes_cfg(b, n, H, W, h, w, C.byref(cfg)))
    if state is not None and "ws" in state:
        ws, m, v, vhat = state["ws"], state["m"], state["v"], state["vhat"]
        if m.shape != x.shape:
            raise AsrError(f"sr_solve: state holds optimiser slots of shape {tuple(m.shape)}, x is {tuple(x.shape)}")
        if ws.numel() * 4 < ws_bytes:       # another plane_chunk / copy count than the call that sized it
            ws = state["ws"] = torch.empty((ws_bytes + 3) // 4, dtype=f32, device=x.device)
    else:
        ws = torch.empty((ws_bytes + 3) // 4, dtype=f32, device=x.device)
        init = slot_init or {}
        m = torch.full_like(x, float(init.get("m", 0.0)))
        v = torch.full_like(x, float(init.get("v", 0.0)))
        vhat = torch.full_like(x, float(init.get("vhat", 0.0)))
        if state is not None:
            state.update(ws=ws, m=m, v=v, vhat=vhat)
    terms = torch.zeros((b, 4), dtype=torch.float64, device=x.device) if want_loss else None
    ms = trace = None
    if mon is not None:
        eval_iters = list(range(0, num_iter, mon["every"]))
        history = (torch.empty((len(eval_iters), b, 4), dtype=torch.float64, device=x.device) if mon["history"] else None)
        iters_done = torch.empty((b,), dtype=torch.int32, device=x.device)
        ms = _lib.SrMonitor(mon["every"], mon["rel_tol"], mon["patience"], mon["min_iter"],
                            history.data_ptr() if history is not None and history.numel() else None, ptr(iters_done, torch.int32))
        trace = SrTrace(history, eval_iters, iters_done)
    rs = cw = cw_hist = rw_iters = None
    if rwp is not None:
        rw_iters = sr_reweight_iters(rwp, num_iter)
        cw = torch.empty((b, n), dtype=f32, device=x.device)
        cw_hist = torch.empty((len(rw_iters), b, n), dtype=f32, device=x.device) if rwp["history"] else None
        rs = _lib.SrReweight(_lib.RW_KINDS[rwp["kind"]], rwp["kappa"], rwp["every"], rwp["start"], ptr(cw),
                             cw_hist.data_ptr() if cw_hist is not None and cw_hist.numel() else None)
    if adj is not None:
        call("asr_sr_solve_adj_f32", ptr(x), ptr(y), ptr(rot_tf), ptr(trans_tf), ptr(inv_rot_tf), ptr(inv_trans_tf), ptr(m),
             ptr(v), ptr(vhat), ptr(alphas), num_iter, ptr(terms, torch.float64, allow_none=True), ptr(ws),
             C.c_size_t(ws_bytes), b, n, H, W, h, w, float(lambdas[0]), float(lambdas[1]), float(lambdas[2]),
             float(lambdas[3]), C.byref(cfg), C.byref(dt), C.byref(ms) if ms is not None else None,
             group if group is not None else 0, C.byref(rs) if rs is not None else None, adj, stream_ptr())
        out = (x, terms) if trace is None else (x, terms, trace)
        return out + (SrCopyWeights(cw, cw_hist, rw_iters),) if rs is not None else out
    if rwp is not None:
        call("asr_sr_solve_rw_f32", ptr(x), ptr(y), ptr(rot_tf), ptr(trans_tf), ptr(inv_rot_tf), ptr(inv_trans_tf), ptr(m),
             ptr(v), ptr(vhat), ptr(alphas), num_iter, ptr(terms, torch.float64, allow_none=True), ptr(ws),
             C.c_size_t(ws_bytes), b, n, H, W, h, w, float(lambdas[0]), float(lambdas[1]), float(lambdas[2]),
             float(lambdas[3]), C.byref(cfg), C.byref(dt), C.byref(ms) if ms is not None else None,
             group if group is not None else 0, C.byref(rs), stream_ptr())
        out = SrCopyWeights(cw, cw_hist, rw_iters)
        return (x, terms, out) if trace is None else (x, terms, trace, out)
    if group is not None:
        call("asr_sr_solve_ml_f32", ptr(x), ptr(y), ptr(rot_tf), ptr(trans_tf), ptr(inv_rot_tf), ptr(inv_trans_tf), ptr(m),
             ptr(v), ptr(vhat), ptr(alphas), num_iter, ptr(terms, torch.float64, allow_none=True), ptr(ws),
             C.c_size_t(ws_bytes), b, n, H, W, h, w, float(lambdas[0]), float(lambdas[1]), float(lambdas[2]),
             float(lambdas[3]), C.byref(cfg), C.byref(dt), C.byref(ms) if ms is not None else None, group, stream_ptr())
        return (x, terms) if trace is None else (x, terms, trace)
    if mon is not None:
        call("asr_sr_solve_mon_f32", ptr(x), ptr(y), ptr(rot_tf), ptr(trans_tf), ptr(inv_rot_tf), ptr(inv_trans_tf), ptr(m),
             ptr(v), ptr(vhat), ptr(alphas), num_iter, ptr(terms, torch.float64, allow_none=True), ptr(ws),
             C.c_size_t(ws_bytes), b, n, H, W, h, w, float(lambdas[0]), float(lambdas[1]), float(lambdas[2]),
             float(lambdas[3]), C.byref(cfg), C.byref(dt), C.byref(ms), stream_ptr())
        return x, terms, trace
    if dt is not None:
        call("asr_sr_solve_dt_f32", ptr(x), ptr(y), ptr(rot_tf), ptr(trans_tf), ptr(inv_rot_tf), ptr(inv_trans_tf), ptr(m),
             ptr(v), ptr(vhat), ptr(alphas), num_iter, ptr(terms, torch.float64, allow_none=True), ptr(ws),
             C.c_size_t(ws_bytes), b, n, H, W, h, w, float(lambdas[0]), float(lambdas[1]), float(lambdas[2]),
             float(lambdas[3]), C.byref(cfg), C.byref(dt), stream_ptr())
    elif tvw is not None:
        call("asr_sr_solve_wtv_f32", ptr(x), ptr(y), ptr(rot_tf), ptr(trans_tf), ptr(inv_rot_tf), ptr(inv_trans_tf), ptr(m),
             ptr(v), ptr(vhat), ptr(alphas), num_iter, ptr(terms, torch.float64, allow_none=True), ptr(ws),
             C.c_size_t(ws_bytes), b, n, H, W, h, w, float(lambdas[0]), float(lambdas[1]), float(lambdas[2]),
             float(lambdas[3]), C.byref(cfg), ptr(tvw[0]), ptr(tvw[1]), tvw[2], stream_ptr())
    elif cfg is None:
        call("asr_sr_solve_f32", ptr(x), ptr(y), ptr(rot_tf), ptr(trans_tf), ptr(inv_rot_tf), ptr(inv_trans_tf), ptr(m),
             ptr(v), ptr(vhat), ptr(alphas), num_iter, ptr(terms, torch.float64, allow_none=True), ptr(ws),
             C.c_size_t(ws_bytes), b, n, H, W, h, w, float(lambdas[0]), float(lambdas[1]), float(lambdas[2]),
             float(lambdas[3]), float(one_minus_beta1), float(one_minus_beta2), float(epsilon), int(bool(amsgrad)),
             stream_ptr())
    else:
        call("asr_sr_solve_cfg_f32", ptr(x), ptr(y), ptr(rot_tf), ptr(trans_tf), ptr(inv_rot_tf), ptr(inv_trans_tf), ptr(m),
             ptr(v), ptr(vhat), ptr(alphas), num_iter, ptr(terms, torch.float64, allow_none=True), ptr(ws),
             C.c_size_t(ws_bytes), b, n, H, W, h, w, float(lambdas[0]), float(lambdas[1]), float(lambdas[2]),
             float(lambdas[3]), C.byref(cfg), stream_ptr())
    return x, terms


def class_counts(truth, pred, segments=1):
    """int32 label tensors -> int64 [segments, 3, 256]: per label |truth|, |pred|, |truth & pred| (Mean_IOU)."""
    per = truth.numel() // segments
    if per * segments != truth.numel() or pred.numel() != truth.numel():
        raise AsrError("class_counts: truth / pred sizes do not split into equal segments")
    out = torch.empty((segments, 3, 256), dtype=torch.int64, device=truth.device)
    call("asr_class_counts_i32", ptr(truth, torch.int32), ptr(pred, torch.int32), ptr(out, torch.int64), per, segments,
         stream_ptr())
    return out


def check_band_widths(widths, r_max=None):
    """The widths of a trimap as a list of ints: 1..16 of them, each in [1, 64] (and <= r_max when given); any order, repeats
    allowed.  Host only; ValueError otherwise."""
    try:
        ws = [int(v) for v in widths]
        same = all(float(v) == float(k) for v, k in zip(widths, ws))
    except TypeError:
        raise ValueError(f"band widths must be a sequence of integers, got {widths!r}") from None
    if not same:
        raise ValueError(f"band widths must be integers, got {list(widths)}")
    if not 1 <= len(ws) <= _lib.MAX_BAND_WIDTHS:
        raise ValueError(f"{len(ws)} band widths (1..{_lib.MAX_BAND_WIDTHS})")
    bad = [v for v in ws if not 1 <= v <= _lib.MAX_BAND_WIDTH]
    if bad:
        raise ValueError(f"band widths must lie in [1, {_lib.MAX_BAND_WIDTH}], got {bad}")
    if r_max is not None and max(ws) > int(r_max):
        raise ValueError(f"band width {max(ws)} > r_max {int(r_max)} of the distance map")
    return ws


def boundary_dist2(truth, r_max, segments=1):
    """int32 label maps [H, W] (segments == 1) or [segments, H, W] -> uint16 of the same shape: the squared distance to the
    nearest label boundary where it is <= r_max^2, else 0xFFFF (asr_boundary_dist2_u16; 1 <= r_max <= 64)."""
    if not ((truth.dim() == 2 and segments == 1) or (truth.dim() == 3 and truth.shape[0] == segments)):
        raise AsrError(f"boundary_dist2: truth must be [H, W] or [{segments}, H, W], got {tuple(truth.shape)}")
    h, w = truth.shape[-2:]
    out = torch.empty(tuple(truth.shape), dtype=torch.uint16, device=truth.device)
    call("asr_boundary_dist2_u16", ptr(truth, torch.int32), ptr(out, torch.uint16), segments, h, w, int(r_max), stream_ptr())
    return out


def band_class_counts(truth, preds, dist2, widths, r_max, ignore_label=255, out=None):
    """One int32 truth and its dist2 (boundary_dist2 with this r_max), P <= 8 int32 predictions [P, ...] of the same size ->
    int64 [P, B, 3, 256]: class_counts restricted to the pixels within widths[b] of a label boundary whose truth is not
    ignore_label (-1: none), in the caller's width order (asr_band_class_counts_i32).  out: a contiguous int64 tensor of
    that size to write into."""
    ws = list(widths)
    per = truth.numel()
    p = preds.numel() // per if per else 0
    if per == 0 or p * per != preds.numel() or dist2.numel() != per:
        raise AsrError("band_class_counts: truth / preds / dist2 size mismatch")
    if out is None:
        out = torch.empty((p, len(ws), 3, 256), dtype=torch.int64, device=truth.device)
    elif out.numel() != p * len(ws) * 768:
        raise AsrError("band_class_counts: out size mismatch")
    arr = (C.c_int * max(len(ws), 1))(*[int(v) for v in ws])
    call("asr_band_class_counts_i32", ptr(truth, torch.int32), ptr(preds, torch.int32), ptr(dist2, torch.uint16), arr,
         ptr(out, torch.int64), per, p, len(ws), int(r_max), int(ignore_label), stream_ptr())
    return out.view(p, len(ws), 3, 256)


def check_confusion_labels(num_labels):
    """num_labels of a confusion matrix as an int in [1, 64].  Host only; ValueError otherwise."""
    try:
        n = int(num_labels)
        same = not isinstance(num_labels, (bool, str, bytes)) and float(num_labels) == float(n)
    except (TypeError, ValueError):
        raise ValueError(f"num_labels must be an integer, got {num_labels!r}") from None
    if not same:
        raise ValueError(f"num_labels must be an integer, got {num_labels!r}")
    if not 1 <= n <= _lib.MAX_CONFUSION_LABELS:
        raise ValueError(f"num_labels {n} (1..{_lib.MAX_CONFUSION_LABELS})")
    return n


def confusion_counts(truth, preds, num_labels, out=None):
    """One int32 truth, P <= 8 int32 predictions [P, ...] of the same size -> int64 [P, L+1, L+1], L = num_labels in [1, 64]:
    [p, i, j] = the pixels whose truth falls in bin i and whose prediction p falls in bin j, bin(v) = v for 0 <= v < L and L
    ("other": void, negative values, ids >= L) otherwise (asr_confusion_counts_i32).  out: a contiguous int64 tensor of that
    size to write into."""
    n = check_confusion_labels(num_labels)
    per = truth.numel()
    p = preds.numel() // per if per else 0
    if per == 0 or p * per != preds.numel():
        raise AsrError("confusion_counts: truth / preds size mismatch")
    if not 1 <= p <= _lib.MAX_CONFUSION_PREDS:
        raise AsrError(f"confusion_counts: {p} predictions (1..{_lib.MAX_CONFUSION_PREDS})")
    side = n + 1
    if out is None:
        out = torch.empty((p, side, side), dtype=torch.int64, device=truth.device)
    elif out.numel() != p * side * side:
        raise AsrError("confusion_counts: out size mismatch")
    call("asr_confusion_counts_i32", ptr(truth, torch.int32), ptr(preds, torch.int32), ptr(out, torch.int64), per, p, n,
         stream_ptr())
    return out.view(p, side, side)


MAX_COVERAGE_BINS = 16


def check_coverages(percents):
    """The coverages of a risk-coverage curve as a list of ints: 1..16 of them, each a whole percentage in [1, 100]; any order,
    repeats allowed.  Host only; ValueError otherwise."""
    if isinstance(percents, (str, bytes)):
        raise ValueError(f"coverages must be a sequence of integers, got {percents!r}")
    try:
        vals = list(percents)
        if any(isinstance(v, (bool, str, bytes)) for v in vals):
            raise TypeError
        ps = [int(v) for v in vals]
        same = all(float(v) == float(k) for v, k in zip(vals, ps))
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"coverages must be a sequence of integers, got {percents!r}") from None
    if not same:
        raise ValueError(f"coverages must be integers, got {vals}")
    if not 1 <= len(ps) <= MAX_COVERAGE_BINS:
        raise ValueError(f"{len(ps)} coverages (1..{MAX_COVERAGE_BINS})")
    bad = [v for v in ps if not 1 <= v <= 100]
    if bad:
        raise ValueError(f"coverages are percentages in [1, 100], got {bad}")
    return ps


def binned_class_counts(truth, preds, u, edges, ignore_label=255, out=None):
    """One int32 truth and one f32 map u of the same size, P <= 8 int32 predictions [P, ...], B <= 16 f32 edges ON THE DEVICE
    -> int64 [P, B, 3, 256]: class_counts restricted to the pixels with u <= edges[b] whose truth is not ignore_label (-1 or
    None: none), in the caller's edge order (asr_binned_class_counts_f32).  A NaN is in no bin; +inf as an edge holds every
    pixel.  out: a contiguous int64 tensor of that size to write into."""
    per = truth.numel()
    p = preds.numel() // per if per else 0
    if per == 0 or p * per != preds.numel() or u.numel() != per:
        raise AsrError("binned_class_counts: truth / preds / u size mismatch")
    if not 1 <= p <= _lib.MAX_BINNED_PREDS:
        raise AsrError(f"binned_class_counts: {p} predictions (1..{_lib.MAX_BINNED_PREDS})")
    nb = edges.numel()
    if edges.dim() != 1 or not 1 <= nb <= MAX_COVERAGE_BINS:
        raise AsrError(f"binned_class_counts: edges must be a vector of 1..{MAX_COVERAGE_BINS} values, got {tuple(edges.shape)}")
    if out is None:
        out = torch.empty((p, nb, 3, 256), dtype=torch.int64, device=truth.device)
    elif out.numel() != p * nb * 768:
        raise AsrError("binned_class_counts: out size mismatch")
    call("asr_binned_class_counts_f32", ptr(truth, torch.int32), ptr(preds, torch.int32), ptr(u), ptr(edges),
         ptr(out, torch.int64), per, p, nb, -1 if ignore_label is None else int(ignore_label), stream_ptr())
    return out.view(p, nb, 3, 256)


def realign(y, trans_tf, rot_tf, out_hw, mode):
    """mode "max" | "mean" -> [B,H,W]; "both" -> (max, mean) from one pass over the copies."""
    if y.dim() != 4:
        raise AsrError("realign: y must be [B,N,h,w]")
    b, n, h, w = y.shape
    _check_tf(trans_tf, b, n, "trans_tf")
    _check_tf(rot_tf, b, n, "rot_tf")
    out = torch.empty((b, out_hw[0], out_hw[1]), dtype=f32, device=y.device)
    if mode == "both":
        out_mean = torch.empty_like(out)
        call("asr_realign_max_mean_f32", ptr(y), ptr(out), ptr(out_mean), ptr(trans_tf), ptr(rot_tf), b, n, out_hw[0],
             out_hw[1], h, w, stream_ptr())
        return out, out_mean
    fn = {"max": "asr_realign_max_f32", "mean": "asr_realign_mean_f32"}[mode]
    call(fn, ptr(y), ptr(out), ptr(trans_tf), ptr(rot_tf), b, n, out_hw[0], out_hw[1], h, w, stream_ptr())
    return out


def quantile_ranks(n, q):
    """The linear-interpolation quantile q in [0, 1] of n sorted values as (lo, hi, t): p = q * (n - 1) in float64,
    lo = floor(p), hi = ceil(p), t = float32(p - lo), to be read as s[lo] + (s[hi] - s[lo]) * t (numpy's default rule).
    The median of an even n is (n/2 - 1, n/2, 0.5)."""
    n = int(n)
    q = float(q)
    if n < 1:
        raise ValueError(f"quantile_ranks: n={n} (>= 1)")
    if not 0.0 <= q <= 1.0:
        raise ValueError(f"quantile_ranks: q={q} outside [0, 1]")
    p = np.float64(q) * np.float64(n - 1)
    lo, hi = int(np.floor(p)), int(np.ceil(p))
    return lo, hi, float(np.float32(p - lo))


def realign_select(y, trans_tf, rot_tf, out_hw, ranks=None, trim_k=None):
    """Order statistics over the realigned copies in one launch (asr_realign_select_f32; the rule: include/asr_hip.h).
    y [B,N,h,w]; ranks: a list of up to 8 (lo, hi, t) -- plane j is s[lo] + (s[hi] - s[lo]) * t of the N sorted values of a
    pixel, s[lo] itself when lo == hi (quantile_ranks builds them); trim_k: None for no trimmed mean, else k >= 0, the mean
    of s[k] .. s[N-1-k] (k = 0: the mean of all N sorted values).  Returns (q [Q,B,H,W] or None, trim [B,H,W] or None)."""
    if y.dim() != 4:
        raise AsrError("realign_select: y must be [B,N,h,w]")
    b, n, h, w = y.shape
    _check_tf(trans_tf, b, n, "trans_tf")
    _check_tf(rot_tf, b, n, "rot_tf")
    ranks = list(ranks or [])
    nq = len(ranks)
    if nq > _lib.MAX_SELECT_PLANES:
        raise AsrError(f"realign_select: {nq} rank triples (at most {_lib.MAX_SELECT_PLANES})")
    want_trim = trim_k is not None
    H, W = int(out_hw[0]), int(out_hw[1])
    q = torch.empty((nq, b, H, W), dtype=f32, device=y.device) if nq else None
    trim = torch.empty((b, H, W), dtype=f32, device=y.device) if want_trim else None
    lo = (C.c_int * max(nq, 1))(*[int(r[0]) for r in ranks])
    hi = (C.c_int * max(nq, 1))(*[int(r[1]) for r in ranks])
    t = (C.c_float * max(nq, 1))(*[float(r[2]) for r in ranks])
    call("asr_realign_select_f32", ptr(y), ptr(q, allow_none=True), ptr(trim, allow_none=True), lo, hi, t, nq,
         int(trim_k) if want_trim else 0, ptr(trans_tf), ptr(rot_tf), b, n, H, W, h, w, stream_ptr())
    return q, trim


COVERED_OUTPUTS = ("mean", "median", "cov")


def realign_covered(y, wgt, trans_tf, rot_tf, out_hw, want=("mean",), cov_min=0.5, valid_min=0.5):
    """Coverage-normalised fusions of the realigned copies in one launch (asr_realign_covered_f32; the rule:
    include/asr_hip.h).  y [B,N,h,w]; wgt [B,N,h,w], or [h,w]: one plane shared by every copy.  Both go through the same
    realign; y is NOT multiplied by wgt here (pass y already weighted for sum R(w y) / sum R(w)).  want: any of "mean"
    (sum of the realigned values / sum of the realigned weights where that sum is >= cov_min, else 0), "median" (over the
    copies whose realigned weight is >= valid_min at the pixel, 0 where there is none) and "cov" (the sum of the realigned
    weights).  Returns a dict of [B,H,W] tensors with the keys asked for."""
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or len(set(want)) != len(want) or any(k not in COVERED_OUTPUTS for k in want):
        raise AsrError(f"realign_covered: want must be a non-empty selection of {COVERED_OUTPUTS} without repeats, got {want!r}")
    for name, v in (("cov_min", cov_min), ("valid_min", valid_min)):
        if not (np.isfinite(float(v)) and float(v) > 0.0):
            raise AsrError(f"realign_covered: {name}={v} must be finite and > 0")
    if y.dim() != 4:
        raise AsrError("realign_covered: y must be [B,N,h,w]")
    b, n, h, w = y.shape
    if wgt.dim() == 2:
        shared = 1
        if tuple(wgt.shape) != (h, w):
            raise AsrError(f"realign_covered: the shared wgt plane must be [{h},{w}], got {tuple(wgt.shape)}")
    elif wgt.dim() == 4:
        shared = 0
        if tuple(wgt.shape) != (b, n, h, w):
            raise AsrError(f"realign_covered: wgt must be [{b},{n},{h},{w}] like y, got {tuple(wgt.shape)}")
    else:
        raise AsrError(f"realign_covered: wgt must be [B,N,h,w] or [h,w], got {tuple(wgt.shape)}")
    _check_tf(trans_tf, b, n, "trans_tf")
    _check_tf(rot_tf, b, n, "rot_tf")
    H, W = int(out_hw[0]), int(out_hw[1])
    out = {k: torch.empty((b, H, W), dtype=f32, device=y.device) for k in want}
    call("asr_realign_covered_f32", ptr(y), ptr(wgt), shared, ptr(out.get("mean"), allow_none=True),
         ptr(out.get("median"), allow_none=True), ptr(out.get("cov"), allow_none=True), float(cov_min), float(valid_min),
         ptr(trans_tf), ptr(rot_tf), b, n, H, W, h, w, stream_ptr())
    return out


MOMENT_OUTPUTS = ("mean", "var", "nv")


def realign_moments(y, trans_tf, rot_tf, out_hw, want=("mean", "var"), wgt=None, valid_min=0.5):
    """Mean, population variance and valid count over the realigned copies in one launch (asr_realign_moments_f32; the rule:
    include/asr_hip.h).  y [B,N,h,w]; wgt None (every copy is valid), [B,N,h,w], or [h,w]: one plane shared by every copy;
    a copy is valid at a pixel where its realigned weight is >= valid_min.  want: any of "mean" (over the valid copies, 0
    where there is none; without wgt it is realign(..., "mean") bit for bit), "var" (the population variance about that
    mean, 0 where nv is 0, exactly 0 where it is 1) and "nv" (the number of valid copies, as f32).  Returns a dict of [B,H,W]
    tensors with the keys asked for."""
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or len(set(want)) != len(want) or any(k not in MOMENT_OUTPUTS for k in want):
        raise AsrError(f"realign_moments: want must be a non-empty selection of {MOMENT_OUTPUTS} without repeats, got {want!r}")
    if wgt is not None and not (np.isfinite(float(valid_min)) and float(valid_min) > 0.0):
        raise AsrError(f"realign_moments: valid_min={valid_min} must be finite and > 0")
    if y.dim() != 4:
        raise AsrError("realign_moments: y must be [B,N,h,w]")
    b, n, h, w = y.shape
    shared = 0
    if wgt is None:
        pass
    elif wgt.dim() == 2:
        shared = 1
        if tuple(wgt.shape) != (h, w):
            raise AsrError(f"realign_moments: the shared wgt plane must be [{h},{w}], got {tuple(wgt.shape)}")
    elif wgt.dim() == 4:
        if tuple(wgt.shape) != (b, n, h, w):
            raise AsrError(f"realign_moments: wgt must be [{b},{n},{h},{w}] like y, got {tuple(wgt.shape)}")
    else:
        raise AsrError(f"realign_moments: wgt must be None, [B,N,h,w] or [h,w], got {tuple(wgt.shape)}")
    _check_tf(trans_tf, b, n, "trans_tf")
    _check_tf(rot_tf, b, n, "rot_tf")
    H, W = int(out_hw[0]), int(out_hw[1])
    out = {k: torch.empty((b, H, W), dtype=f32, device=y.device) for k in want}
    call("asr_realign_moments_f32", ptr(y), ptr(wgt, allow_none=True), shared, ptr(out.get("mean"), allow_none=True),
         ptr(out.get("var"), allow_none=True), ptr(out.get("nv"), allow_none=True), float(valid_min) if wgt is not None else 0.0,
         ptr(trans_tf), ptr(rot_tf), b, n, H, W, h, w, stream_ptr())
    return out


# ---------------------------------------------------------------------------------------------
# OPM / threshold / IoU
# ---------------------------------------------------------------------------------------------
def minmax(x, segments=1):
    per = x.numel() // segments
    if per * segments != x.numel() or per == 0:
        raise AsrError("minmax: tensor does not split into equal non-empty segments")
    out = torch.empty((segments, 2), dtype=f32, device=x.device)
    call("asr_minmax_f32", ptr(x), ptr(out), per, segments, stream_ptr())
    return out


def minmax_normalize(x, segments=1, new_min=0.0, new_max=1.0):
    """min_max_normalization of each of ``segments`` equal parts of x with its own global extrema (device, one call)."""
    per = x.numel() // segments
    if per * segments != x.numel() or per == 0:
        raise AsrError("minmax_normalize: tensor does not split into equal non-empty segments")
    out = torch.empty_like(x)
    ws = torch.empty((segments, 2), dtype=f32, device=x.device)
    call("asr_minmax_normalize_f32", ptr(x), ptr(out), ptr(ws), per, segments, float(new_min), float(new_max), stream_ptr())
    return out


def standard_mask(logits0, out_hw, class_id, out=None):
    """logits0 [h,w,C] of the un-augmented image -> int32 mask [H,W] in {0, class_id}: bilinear upsample + argmax + class
    filter in one kernel (generate_standard_output.py:52-65)."""
    h, w, c = logits0.shape
    out_hw = (int(out_hw[0]), int(out_hw[1]))
    if out is None:
        out = torch.empty(out_hw, dtype=torch.int32, device=logits0.device)
    elif tuple(out.shape) != out_hw:
        raise AsrError(f"standard_mask: out must be {out_hw}, got {tuple(out.shape)}")
    call("asr_standard_mask_i32", ptr(logits0), ptr(out, torch.int32), h, w, c, int(out_hw[0]), int(out_hw[1]), int(class_id),
         stream_ptr())
    return out


def class_activation(logits, kind):
    """softmax / sigmoid over the last (class) axis, in a new tensor."""
    classes = logits.shape[-1]
    out = torch.empty_like(logits)
    call("asr_class_activation_f32", ptr(logits), ptr(out), logits.numel() // classes, classes,
         {"softmax": 1, "sigmoid": 2}[kind], stream_ptr())
    return out


def opm_confidence(logits, kind, out=None):
    """logits [..., C] -> [...] float32: the network's confidence per pixel, "maxprob" (the largest softmax entry) or "margin"
    (the difference of the two largest); the weights of the SR data term (include/asr_hip.h: the rule).  out: a contiguous
    float32 tensor of that shape to write into."""
    if kind not in _lib.CONF_KINDS:
        raise ValueError(f"opm_confidence: kind must be one of {sorted(_lib.CONF_KINDS)}, got {kind!r}")
    if not isinstance(logits, torch.Tensor) or logits.dim() < 1 or logits.numel() == 0:
        raise AsrError("opm_confidence: logits must be a non-empty tensor [..., classes]")
    shape = tuple(logits.shape[:-1])
    if out is None:
        out = torch.empty(shape, dtype=f32, device=logits.device)
    elif (not isinstance(out, torch.Tensor) or tuple(out.shape) != shape or out.device != logits.device or out.dtype != f32
          or not out.is_contiguous()):
        raise AsrError(f"opm_confidence: out must be a contiguous float32 tensor {shape} on the device of the logits, got "
                       f"{tuple(out.shape) if isinstance(out, torch.Tensor) else type(out).__name__}")
    call("asr_opm_confidence_f32", ptr(logits), ptr(out), logits.numel() // logits.shape[-1], logits.shape[-1],
         _lib.CONF_KINDS[kind], stream_ptr())
    return out


def argmax(logits):
    classes = logits.shape[-1]
    pixels = logits.numel() // classes
    out = torch.empty(logits.shape[:-1], dtype=torch.int32, device=logits.device)
    call("asr_argmax_i32", ptr(logits), ptr(out, torch.int32), pixels, classes, stream_ptr())
    return out


def _opm_out(out, logits, name):
    """out: optional contiguous [N,h,w] float32 destination (a slice of a per-image stack), else a new tensor."""
    if out is None:
        return torch.empty(logits.shape[:-1], dtype=f32, device=logits.device)
    if tuple(out.shape) != tuple(logits.shape[:-1]) or not out.is_contiguous():
        raise AsrError(f"{name}: out must be a contiguous {tuple(logits.shape[:-1])} tensor, got {tuple(out.shape)}")
    return out


def opm_argmax(logits, class_id, out=None):
    classes = logits.shape[-1]
    pixels = logits.numel() // classes
    out = _opm_out(out, logits, "opm_argmax")
    call("asr_opm_argmax_f32", ptr(logits), ptr(out), pixels, classes, class_id, stream_ptr())
    return out


def opm_slice_max(logits, class_id, out=None, out_max=None):
    classes = logits.shape[-1]
    pixels = logits.numel() // classes
    cls = _opm_out(out, logits, "opm_slice_max")
    mx = _opm_out(out_max, logits, "opm_slice_max")
    call("asr_opm_slice_max_f32", ptr(logits), ptr(cls), ptr(mx), pixels, classes, class_id, stream_ptr())
    return cls, mx


def opm_slice(logits, class_id, new_min=0.0, new_max=1.0, out=None):
    """logits [N,h,w,C]: per-copy global min/max normalisation of the class slice."""
    n = logits.shape[0]
    classes = logits.shape[-1]
    per_copy = logits.numel() // (n * classes)
    out = _opm_out(out, logits, "opm_slice")
    ws = torch.empty((n, 2), dtype=f32, device=logits.device)
    call("asr_opm_slice_f32", ptr(logits), ptr(out), ptr(ws), n, per_copy, classes, class_id, float(new_min),
         float(new_max), stream_ptr())
    return out


def threshold(image, th_value, th_factor=0.15, th_mask=None, segments=1, out=None):
    per = image.numel() // segments if segments > 0 else 0
    if per * segments != image.numel() or per == 0:
        raise AsrError("threshold: image does not split into equal non-empty segments")
    if out is None:
        out = torch.empty(image.shape, dtype=torch.int32, device=image.device)
    elif out.numel() != image.numel():
        raise AsrError("threshold: out size mismatch")
    elif out.dtype != torch.int32 or not out.is_contiguous():
        raise AsrError(f"threshold: out must be a contiguous int32 tensor, got {out.dtype}"
                       f"{'' if out.is_contiguous() else ' (not contiguous)'}")
    ws = torch.empty((segments, 2), dtype=f32, device=image.device)
    if th_mask is not None and th_mask.shape != image.shape:
        raise AsrError("threshold: th_mask shape mismatch")
    call("asr_threshold_f32", ptr(image), ptr(th_mask, allow_none=True), ptr(ws), ptr(out, torch.int32), per, segments,
         float(np.float32(th_factor)), int(th_value), stream_ptr())
    return out


def iou_counts_shared_truth(truth, preds, class_id, include_bg=False):
    """preds [K, ...] int32 masks against ONE int32 label map of the same pixel count -> int64 [K, 4]."""
    k = preds.shape[0]
    per = preds.numel() // k
    if truth.numel() != per:
        raise AsrError("iou_counts_shared_truth: size mismatch")
    counts = torch.empty((k, 4), dtype=torch.int64, device=truth.device)
    call("asr_iou_counts_shared_truth_i32", ptr(truth, torch.int32), ptr(preds, torch.int32), ptr(counts, torch.int64), per, k,
         int(class_id), int(bool(include_bg)), stream_ptr())
    return counts


def iou_counts(truth, pred, class_id, include_bg=False, segments=1):
    if truth.numel() != pred.numel():
        raise AsrError("iou_counts: size mismatch")
    per = truth.numel() // segments if segments > 0 else 0
    if per * segments != truth.numel() or per == 0:
        raise AsrError("iou_counts: truth / pred do not split into equal non-empty segments")
    counts = torch.empty((segments, 4), dtype=torch.int64, device=truth.device)
    call("asr_iou_counts_i32", ptr(truth, torch.int32), ptr(pred, torch.int32), ptr(counts, torch.int64), per, segments,
         int(class_id), int(bool(include_bg)), stream_ptr())
    return counts


# ---------------------------------------------------------------------------------------------
# class sets: K classes of one image, each equal bit for bit to its single-class call
# ---------------------------------------------------------------------------------------------
def class_set(class_ids):
    """Host int array of a class set for the *_classes entry points (the library checks count, range and repeats)."""
    ids = [int(c) for c in np.asarray(class_ids, dtype=np.int64).reshape(-1)]
    return (C.c_int * max(len(ids), 1))(*ids), len(ids)


def _planes(out, k, plane_shape, dtype, device, name):
    """[K, *plane_shape] destination: a new tensor, or a view whose planes are each contiguous and lie a uniform stride
    apart (rows [i, i+b) of per-class [K, N, h, w] stacks).  Returns (tensor, element stride between planes)."""
    if out is None:
        out = torch.empty((k,) + tuple(plane_shape), dtype=dtype, device=device)
    if tuple(out.shape) != (k,) + tuple(plane_shape) or out.dtype != dtype or not out.is_cuda:
        raise AsrError(f"{name}: out must be a {dtype} device tensor of shape {(k,) + tuple(plane_shape)}, got "
                       f"{out.dtype} {tuple(out.shape)}")
    if not out[0].is_contiguous() or (k > 1 and out.stride(0) < out[0].numel()):
        raise AsrError(f"{name}: every plane of out must be contiguous and the planes must not overlap")
    return out, (out.stride(0) if k > 1 else out[0].numel())


def opm_classes(logits, class_ids, mode, out=None, out_max=None, new_min=0.0, new_max=1.0):
    """logits [N,h,w,C] -> (class masks [K,N,h,w], max masks [K,N,h,w] | None): plane k equals opm_argmax / opm_slice /
    opm_slice_max of class_ids[k], from one read of the logits.  out / out_max may be views of rows of larger stacks."""
    if mode not in _lib.OPM_MODES:
        raise AsrError(f"opm_classes: mode must be one of {sorted(_lib.OPM_MODES)}, got {mode!r}")
    if logits.dim() < 2 or not logits.is_contiguous():
        raise AsrError("opm_classes: logits must be a contiguous [N, ..., C] tensor")
    ids, k = class_set(class_ids)
    classes = logits.shape[-1]
    n = logits.shape[0]
    per_copy = logits.numel() // (n * classes)
    plane = tuple(logits.shape[:-1])
    cls, stride = _planes(out, k, plane, f32, logits.device, "opm_classes")
    mx = None
    if mode == "slice_max":
        mx, stride_max = _planes(out_max, k, plane, f32, logits.device, "opm_classes")
        if stride_max != stride:
            raise AsrError("opm_classes: out and out_max must have the same plane stride")
    ws = torch.empty((n, 2), dtype=f32, device=logits.device) if mode == "slice" else None
    call("asr_opm_classes_f32", ptr(logits), ids, k, _lib.OPM_MODES[mode], cls.data_ptr(),
         mx.data_ptr() if mx is not None else None, ptr(ws, allow_none=True), n, per_copy, classes, stride, float(new_min),
         float(new_max), stream_ptr())
    return cls, mx


def threshold_classes(image, class_ids, th_factor=0.15, th_mask=None, out=None):
    """image [K, ...]: segment k thresholded like threshold(image[k], class_ids[k], th_factor, th_mask[k]) -> int32 [K, ...]."""
    ids, k = class_set(class_ids)
    if image.shape[0] != k or image.numel() % k:
        raise AsrError(f"threshold_classes: image must have one segment per class ({k}), got {tuple(image.shape)}")
    per = image.numel() // k
    if out is None:
        out = torch.empty(image.shape, dtype=torch.int32, device=image.device)
    elif out.numel() != image.numel():
        raise AsrError("threshold_classes: out size mismatch")
    if th_mask is not None and th_mask.shape != image.shape:
        raise AsrError("threshold_classes: th_mask shape mismatch")
    ws = torch.empty((k, 2), dtype=f32, device=image.device)
    call("asr_threshold_classes_f32", ptr(image), ptr(th_mask, allow_none=True), ptr(ws), ptr(out, torch.int32), per, k,
         float(np.float32(th_factor)), ids, stream_ptr())
    return out


def iou_counts_classes(truth, preds, class_ids, include_bg=False):
    """preds [K, M, ...] int32 (the M masks of class_ids[k] in row k) against ONE int32 label map -> int64 [K, M, 4]."""
    ids, k = class_set(class_ids)
    if preds.dim() < 2 or preds.shape[0] != k:
        raise AsrError(f"iou_counts_classes: preds must be [K={k}, M, ...], got {tuple(preds.shape)}")
    m = preds.shape[1]
    per = preds.numel() // (k * m) if m else 0
    if per == 0 or truth.numel() != per:
        raise AsrError("iou_counts_classes: size mismatch")
    counts = torch.empty((k, m, 4), dtype=torch.int64, device=truth.device)
    call("asr_iou_counts_classes_i32", ptr(truth, torch.int32), ptr(preds, torch.int32), ptr(counts, torch.int64), per, k, m,
         ids, int(bool(include_bg)), stream_ptr())
    return counts


def standard_mask_classes(logits0, out_hw, class_ids, out=None):
    """logits0 [h,w,C] -> int32 masks [K,H,W], mask k = standard_mask(logits0, out_hw, class_ids[k])."""
    h, w, c = logits0.shape
    ids, k = class_set(class_ids)
    if out is None:
        out = torch.empty((k,) + tuple(out_hw), dtype=torch.int32, device=logits0.device)
    elif tuple(out.shape) != (k,) + tuple(out_hw):
        raise AsrError(f"standard_mask_classes: out must be {(k,) + tuple(out_hw)}, got {tuple(out.shape)}")
    call("asr_standard_mask_classes_i32", ptr(logits0), ptr(out, torch.int32), h, w, c, int(out_hw[0]), int(out_hw[1]), ids, k,
         stream_ptr())
    return out


# ---------------------------------------------------------------------------------------------
# label maps: the K single-class results of one image fused into one label map
# ---------------------------------------------------------------------------------------------
def fuse_labels(scores, class_ids, th_factor=0.15, max_scores=None, truth=None, out=None, classes=0):
    """scores [K, ...] float32 (plane k: the SR output of class_ids[k]) -> int32 label map [...]: class_ids[k*] where k* is
    the class with the greatest rank value among those whose single-class mask is set at the pixel (scores[k] > th_factor *
    max(scores[k]) ranked by scores[k]; with max_scores [K, ...]: scores[k] >= max_scores[k] ranked by their difference), the
    lowest k on equal values, 0 where none passes (asr_fuse_labels_f32).  truth (int32 label map): returns (labels, int64
    [3, 256] counts equal to class_counts(truth, labels)[0]) from the same pass; else (labels, None).  Ids lie in
    [1, classes) (classes = 0: any id >= 1)."""
    ids, k = class_set(class_ids)
    if scores.dim() < 2 or scores.shape[0] != k:
        raise AsrError(f"fuse_labels: scores must have one plane per class ({k}), got {tuple(scores.shape)}")
    per = scores.numel() // k
    if max_scores is not None and max_scores.shape != scores.shape:
        raise AsrError("fuse_labels: max_scores shape mismatch")
    if out is None:
        out = torch.empty(tuple(scores.shape[1:]), dtype=torch.int32, device=scores.device)
    elif out.numel() != per:
        raise AsrError("fuse_labels: out size mismatch")
    counts = None
    if truth is not None:
        if truth.numel() != per:
            raise AsrError(f"fuse_labels: truth has {truth.numel()} pixels, expected {per}")
        counts = torch.empty((3, 256), dtype=torch.int64, device=scores.device)
    ws = torch.empty((k, 2), dtype=f32, device=scores.device) if max_scores is None else None
    call("asr_fuse_labels_f32", ptr(scores), ptr(max_scores, allow_none=True), ptr(ws, allow_none=True),
         ptr(truth, torch.int32, allow_none=True), ptr(out, torch.int32), ptr(counts, torch.int64, allow_none=True), per, k,
         float(np.float32(th_factor)), ids, int(classes), stream_ptr())
    return out, counts


def fuse_labels_simplex(scores, class_ids, out=None):
    """scores [K, ...] float32, the planes of a coupled solve (shares of each pixel) -> int32 label map [...]: class_ids[k*],
    k* the first class of greatest share, where that share exceeds the background's 1 - sum_k scores[k] (float32, index
    order), else 0 (asr_fuse_labels_simplex_f32).  No threshold; counts come from class_counts."""
    ids, k = class_set(class_ids)
    if scores.dim() < 2 or scores.shape[0] != k:
        raise AsrError(f"fuse_labels_simplex: scores must have one plane per class ({k}), got {tuple(scores.shape)}")
    per = scores.numel() // k
    if out is None:
        out = torch.empty(tuple(scores.shape[1:]), dtype=torch.int32, device=scores.device)
    elif out.numel() != per:
        raise AsrError("fuse_labels_simplex: out size mismatch")
    call("asr_fuse_labels_simplex_f32", ptr(scores), ids, k, ptr(out, torch.int32), per, stream_ptr())
    return out


MAX_LABEL_SWEEP_FACTORS = 64


def fuse_labels_sweep_counts(scores, class_ids, truth, factors, classes=0, out=None):
    """scores [K, ...] float32, truth int32 label map, factors: T threshold factors (1..64, any order, repeats allowed; a host
    sequence or a float32 device tensor) ->
    device int64 [T, 3, 256]: counts[j] = fuse_labels(scores, class_ids, th_factor=factors[j], truth=truth, classes=classes)[1]
    bit for bit, from one pass over the planes for all factors and without writing a label map
    (asr_fuse_labels_sweep_counts_f32).  There is no max_scores form: the threshold plays no part there.  out: int64 with
    T * 768 elements."""
    ids, k = class_set(class_ids)
    if scores.dim() < 2 or scores.shape[0] != k:
        raise AsrError(f"fuse_labels_sweep_counts: scores must have one plane per class ({k}), got {tuple(scores.shape)}")
    per = scores.numel() // k
    if truth is None or truth.numel() != per:
        raise AsrError(f"fuse_labels_sweep_counts: truth has {0 if truth is None else truth.numel()} pixels, expected {per}")
    if isinstance(factors, torch.Tensor):           # already on the device: one upload serves several calls
        f = factors.to(device=scores.device, dtype=f32).contiguous().reshape(-1)
    else:
        f = to_device(np.asarray(factors, dtype=np.float32).reshape(-1), device=scores.device)
    t = f.numel()
    if not 1 <= t <= MAX_LABEL_SWEEP_FACTORS:
        raise AsrError(f"fuse_labels_sweep_counts: {t} threshold factors (1..{MAX_LABEL_SWEEP_FACTORS})")
    if out is None:
        out = torch.empty((t, 3, 256), dtype=torch.int64, device=scores.device)
    elif out.numel() != t * 768:
        raise AsrError("fuse_labels_sweep_counts: out size mismatch")
    lib = _lib.load()
    ws_bytes = lib.asr_fuse_labels_sweep_workspace_bytes(k, t)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=scores.device)
    call("asr_fuse_labels_sweep_counts_f32", ptr(scores), ptr(truth, torch.int32), ptr(f), ptr(ws, torch.uint8), ws_bytes,
         ptr(out, torch.int64), per, k, t, ids, int(classes), stream_ptr())
    return out.view(t, 3, 256)


def standard_labels(logits0, out_hw, class_ids, out=None):
    """logits0 [h,w,C] -> int32 label map [H,W]: the upsampled argmax where it is one of class_ids, else 0 -- the sum of
    standard_mask_classes' K masks (asr_standard_labels_i32)."""
    h, w, c = logits0.shape
    ids, k = class_set(class_ids)
    if out is None:
        out = torch.empty(tuple(out_hw), dtype=torch.int32, device=logits0.device)
    elif tuple(out.shape) != tuple(out_hw):
        raise AsrError(f"standard_labels: out must be {tuple(out_hw)}, got {tuple(out.shape)}")
    call("asr_standard_labels_i32", ptr(logits0), ptr(out, torch.int32), h, w, c, int(out_hw[0]), int(out_hw[1]), ids, k,
         stream_ptr())
    return out


# ---------------------------------------------------------------------------------------------
# guided filter: score planes refined against the image (asr_guided_prepare_f32 / asr_guided_apply_f32)
# ---------------------------------------------------------------------------------------------
MAX_GUIDED_RADIUS = 32


def check_guided(radius, eps):
    """(radius, eps) of a guided filter as (int, float32-rounded float): 0 <= radius <= MAX_GUIDED_RADIUS, eps finite and > 0."""
    if isinstance(radius, bool) or int(radius) != radius:
        raise ValueError(f"guided filter: the radius must be an integer, got {radius!r}")
    radius = int(radius)
    if not 0 <= radius <= MAX_GUIDED_RADIUS:
        raise ValueError(f"guided filter: radius {radius} outside 0..{MAX_GUIDED_RADIUS}")
    eps = float(np.float32(eps))
    if not (np.isfinite(eps) and eps > 0.0):
        raise ValueError(f"guided filter: eps must be finite and > 0, got {eps!r}")
    return radius, eps


class GuidedState:
    """What asr_guided_prepare_f32 leaves for one guide: the state tensor with the H, W, radius (and eps) it belongs to."""
    __slots__ = ("tensor", "H", "W", "radius", "eps")

    def __init__(self, tensor, H, W, radius, eps):
        self.tensor, self.H, self.W, self.radius, self.eps = tensor, H, W, radius, eps


def _check_guide(guide, name):
    if not isinstance(guide, torch.Tensor) or guide.dim() != 3 or guide.shape[2] != 3 or guide.shape[0] < 1 or guide.shape[1] < 1:
        shape = tuple(guide.shape) if isinstance(guide, torch.Tensor) else type(guide)
        raise ValueError(f"{name}: the guide must be an [H, W, 3] tensor, got {shape}")
    return int(guide.shape[0]), int(guide.shape[1])


def guided_prepare(guide, radius, eps):
    """guide [H, W, 3] float32 -> GuidedState: the guide-only pass of the guided filter (window means of the guide and the
    factorised 3x3 covariances), run once per image and shared by every plane filtered against it."""
    H, W = _check_guide(guide, "guided_prepare")
    radius, eps = check_guided(radius, eps)
    lib = _lib.load()
    state = torch.empty(lib.asr_guided_state_bytes(H, W) // 4, dtype=f32, device=guide.device)
    call("asr_guided_prepare_f32", ptr(guide), ptr(state), H, W, radius, eps, stream_ptr())
    return GuidedState(state, H, W, radius, eps)


def guided_apply(state, guide, p, out=None):
    """p [H, W] or [P, H, W] float32 -> q of the same shape: the guided filter of include/asr_hip.h with the guide that
    `state` was prepared from.  out may be p itself (in place).  The workspace (16 bytes per pixel and plane) comes from
    torch's caching allocator, which hands the same block back for the same shape on the same stream."""
    if not isinstance(state, GuidedState):
        raise ValueError(f"guided_apply: state must come from guided_prepare, got {type(state)}")
    H, W = _check_guide(guide, "guided_apply")
    if (H, W) != (state.H, state.W):
        raise ValueError(f"guided_apply: the state was prepared for {state.H} x {state.W}, the guide is {H} x {W}")
    if not isinstance(p, torch.Tensor) or p.dim() not in (2, 3) or tuple(p.shape[-2:]) != (H, W) or p.shape[0] < 1:
        shape = tuple(p.shape) if isinstance(p, torch.Tensor) else type(p)
        raise ValueError(f"guided_apply: p must be [{H}, {W}] or [P, {H}, {W}], got {shape}")
    planes = 1 if p.dim() == 2 else int(p.shape[0])
    if out is None:
        out = torch.empty_like(p)
    elif tuple(out.shape) != tuple(p.shape):
        raise ValueError(f"guided_apply: out must be {tuple(p.shape)}, got {tuple(out.shape)}")
    lib = _lib.load()
    ws = torch.empty(lib.asr_guided_workspace_bytes(planes, H, W) // 4, dtype=f32, device=p.device)
    call("asr_guided_apply_f32", ptr(state.tensor), ptr(guide), ptr(p), ptr(out), ptr(ws), planes, H, W, state.radius,
         stream_ptr())
    return out


def guided_filter(guide, p, radius=8, eps=1e-3, out=None):
    """guided_apply(guided_prepare(guide, radius, eps), guide, p, out): one-shot use."""
    return guided_apply(guided_prepare(guide, radius, eps), guide, p, out=out)


# ---------------------------------------------------------------------------------------------
# windowed CRF: label maps decided jointly over classes and image (asr_crf_unaries_* / asr_crf_refine_f32)
# ---------------------------------------------------------------------------------------------
MAX_CRF_LABELS = _lib.MAX_CRF_LABELS
CrfParams = namedtuple("CrfParams", "radius dilation iterations w_app w_smooth theta_pos theta_rgb theta_smooth")
CRF_DEFAULTS = CrfParams(radius=3, dilation=1, iterations=5, w_app=4.0, w_smooth=1.0, theta_pos=2.0, theta_rgb=0.1,
                         theta_smooth=1.0)


def _crf_int(v, name):
    whole = isinstance(v, (int, np.integer)) or (isinstance(v, (float, np.floating)) and np.isfinite(v) and v == int(v))
    if isinstance(v, (bool, np.bool_, str, bytes)) or not whole:
        raise ValueError(f"crf: {name} must be an integer, got {v!r}")
    return int(v)


def check_crf(params):
    """The config of the windowed CRF (include/asr_hip.h) as a CrfParams: a dict of any of its fields, or None, over
    CRF_DEFAULTS; floats rounded to float32.  ValueError with the wording of asr_crf_refine_f32's own checks for an unknown
    field, a bad value or a value beyond a cap."""
    params = {} if params is None else dict(params)
    unknown = sorted(set(params) - set(CrfParams._fields))
    if unknown:
        raise ValueError(f"crf: unknown field(s) {unknown} (the fields are {list(CrfParams._fields)})")
    p = CRF_DEFAULTS._replace(**params)
    r, d, t = (_crf_int(getattr(p, f), f) for f in ("radius", "dilation", "iterations"))
    if r < 1:
        raise ValueError(f"crf: radius {r} below 1")
    if d < 1:
        raise ValueError(f"crf: dilation {d} below 1")
    if t < 0:
        raise ValueError(f"crf: {t} iterations")
    fl = {}
    for f in ("w_app", "w_smooth"):
        fl[f] = float(np.float32(getattr(p, f)))
        if not (np.isfinite(fl[f]) and fl[f] >= 0.0):
            raise ValueError(f"crf: {f} must be finite and >= 0 (got {fl[f]!r})")
    for f in ("theta_pos", "theta_rgb", "theta_smooth"):
        fl[f] = float(np.float32(getattr(p, f)))
        if not (np.isfinite(fl[f]) and fl[f] > 0.0):
            raise ValueError(f"crf: {f} must be finite and > 0 (got {fl[f]!r})")
    if r > _lib.MAX_CRF_RADIUS:
        raise ValueError(f"crf: radius {r} above the cap of {_lib.MAX_CRF_RADIUS}")
    if r * d > _lib.MAX_CRF_HALO:
        raise ValueError(f"crf: radius {r} x dilation {d} above the cap of {_lib.MAX_CRF_HALO}")
    if t > _lib.MAX_CRF_ITERATIONS:
        raise ValueError(f"crf: {t} iterations above the cap of {_lib.MAX_CRF_ITERATIONS}")
    return CrfParams(r, d, t, **fl)


def check_crf_tau(tau):
    """tau of crf_unaries as a float32-rounded float: finite and > 0."""
    tau = float(np.float32(tau))
    if not (np.isfinite(tau) and tau > 0.0):
        raise ValueError(f"crf: tau must be finite and > 0 (got {tau!r})")
    return tau


def check_crf_conf(conf, num_labels):
    """conf of crf_unaries_from_labels as a float32-rounded float: inside (1 / num_labels, 1), compared in float32 as the
    library compares it."""
    conf = float(np.float32(conf))
    if not np.float32(1) / np.float32(num_labels) < np.float32(conf) < np.float32(1):
        raise ValueError(f"crf: conf must lie in (1/{num_labels}, 1) (got {conf!r})")
    return conf


def crf_unaries(scores, th_factor, tau=0.1):
    """scores [K, H, W] float32 (plane k: the SR output of class k, what fuse_labels reads) -> unaries z [K + 1, H, W]:
    z[0] = 0, z[k + 1] = (scores[k] - th_factor * max(scores[k])) / tau (asr_crf_unaries_scores_f32): the margin by which
    class k passes fuse_labels' threshold, in units of tau."""
    if not isinstance(scores, torch.Tensor) or scores.dim() < 2 or not 1 <= scores.shape[0] <= _lib.MAX_CRF_LABELS - 1:
        shape = tuple(scores.shape) if isinstance(scores, torch.Tensor) else type(scores)
        raise ValueError(f"crf_unaries: scores must be [K, ...] with K in 1..{_lib.MAX_CRF_LABELS - 1}, got {shape}")
    tau = check_crf_tau(tau)
    k = int(scores.shape[0])
    z = torch.empty((k + 1,) + tuple(scores.shape[1:]), dtype=f32, device=scores.device)
    ws = torch.empty((k, 2), dtype=f32, device=scores.device)
    call("asr_crf_unaries_scores_f32", ptr(scores), ptr(ws), ptr(z), scores.numel() // k, k, float(np.float32(th_factor)), tau,
         stream_ptr())
    return z


def crf_unaries_from_labels(labels, ids, conf):
    """labels int32 [H, W], ids: the K class ids -> unaries z [K + 1, H, W]: log(conf) for the label the map holds (0: label 0),
    log((1 - conf) / K) for the others, all 0 where the map holds none of them (asr_crf_unaries_labels_f32)."""
    cids, k = class_set(ids)
    conf = check_crf_conf(conf, k + 1)
    z = torch.empty((k + 1,) + tuple(labels.shape), dtype=f32, device=labels.device)
    call("asr_crf_unaries_labels_f32", ptr(labels, torch.int32), ptr(z), labels.numel(), cids, k + 1, conf, stream_ptr())
    return z


def crf_refine(guide, z, ids, params=None, out=None, want_q=False):
    """The windowed CRF of include/asr_hip.h: guide [H, W, 3] float32, unaries z [L, H, W] float32, ids: the L - 1 class ids of
    labels 1 .. L-1, params: check_crf's argument -> the int32 label map [H, W] (into out when given), or with want_q
    (labels, Q [L, H, W]).  Device tensors only.  The workspace (the two Q buffers) comes from torch's caching allocator."""
    H, W = _check_guide(guide, "crf_refine")
    p = params if isinstance(params, CrfParams) else check_crf(params)
    cids, k = class_set(ids)
    if not isinstance(z, torch.Tensor) or tuple(z.shape) != (k + 1, H, W):
        shape = tuple(z.shape) if isinstance(z, torch.Tensor) else type(z)
        raise ValueError(f"crf_refine: z must be [{k + 1}, {H}, {W}] (label 0 and {k} ids), got {shape}")
    if out is None:
        out = torch.empty((H, W), dtype=torch.int32, device=z.device)
    elif tuple(out.shape) != (H, W):
        raise ValueError(f"crf_refine: out must be {(H, W)}, got {tuple(out.shape)}")
    q = torch.empty_like(z) if want_q else None
    lib = _lib.load()
    ws = torch.empty(lib.asr_crf_workspace_bytes(k + 1, H, W) // 4, dtype=f32, device=z.device)
    cfg = _lib.CrfConfig(*p)
    call("asr_crf_refine_f32", ptr(guide), ptr(z), cids, k + 1, H, W, C.byref(cfg), ptr(ws), ptr(out, torch.int32),
         ptr(q, allow_none=True), stream_ptr())
    return (out, q) if want_q else out


# ---------------------------------------------------------------------------------------------
def _region_int(v, name, what="min_region"):
    try:
        if isinstance(v, (bool, str, bytes)):
            raise TypeError
        n = int(v)
        same = float(v) == float(n)
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"{what}: {name} must be an integer, got {v!r}") from None
    if not same:
        raise ValueError(f"{what}: {name} must be an integer, got {v!r}")
    return n


def check_min_region(min_region):
    """min_region of a label-map clean-up as (min_area, connectivity): an int (connectivity 4) or a pair (min_area,
    connectivity); min_area >= 1, connectivity 4 or 8.  Host only; ValueError otherwise."""
    if isinstance(min_region, (tuple, list)):
        if len(min_region) != 2:
            raise ValueError(f"min_region must be an integer or (min_area, connectivity), got {min_region!r}")
        area, conn = _region_int(min_region[0], "min_area"), _region_int(min_region[1], "connectivity")
    else:
        area, conn = _region_int(min_region, "min_area"), 4
    if area < 1:
        raise ValueError(f"min_region: min_area {area} below 1")
    if area > 2 ** 31 - 1:
        raise ValueError(f"min_region: min_area {area} above 2^31 - 1")
    if conn not in (4, 8):
        raise ValueError(f"min_region: connectivity {conn} (4 or 8)")
    return area, conn


def _region_maps(labels, name):
    if not isinstance(labels, torch.Tensor):
        raise AsrError(f"{name}: expected a torch.Tensor, got {type(labels)}")
    if labels.dim() not in (2, 3) or min(labels.shape) < 1:
        raise AsrError(f"{name}: labels must be [H, W] or [M, H, W], got {tuple(labels.shape)}")
    maps = 1 if labels.dim() == 2 else int(labels.shape[0])
    return maps, int(labels.shape[-2]), int(labels.shape[-1])


def label_regions(labels, connectivity=4):
    """int32 label maps [H, W] or [M, H, W] -> (root, area), int32 of the same shape: the smallest linear index (within the
    pixel's own map) and the pixel count of each pixel's connected region of equal value (asr_label_regions_i32; connectivity
    4 or 8).  The workspace (4 bytes per pixel) comes from torch's caching allocator."""
    maps, h, w = _region_maps(labels, "label_regions")
    lib = _lib.load()
    root, area = torch.empty_like(labels), torch.empty_like(labels)
    nbytes = lib.asr_label_regions_workspace_bytes(maps, h, w)
    ws = torch.empty(max(nbytes // 4, 1), dtype=torch.int32, device=labels.device)
    call("asr_label_regions_i32", ptr(labels, torch.int32), ptr(root, torch.int32), ptr(area, torch.int32),
         ptr(ws, torch.int32), nbytes, maps, h, w, int(connectivity), stream_ptr())
    return root, area


def clean_labels(labels, min_area, connectivity=4, regions=None, out=None, want_stats=False):
    """int32 label maps [H, W] or [M, H, W] -> the maps with every region of fewer than min_area pixels replaced by the one
    value of its non-small surround, or by 0 when that surround is empty or mixed (asr_clean_labels_i32).  regions: the
    (root, area) of label_regions(labels, connectivity), to reuse them; out: may be labels itself (in place).
    want_stats: also the int64 [M, 4] (or [4]) tensor of regions, small regions, pixels in small regions, pixels changed."""
    maps, h, w = _region_maps(labels, "clean_labels")
    min_area, connectivity = check_min_region((min_area, connectivity))
    root, area = label_regions(labels, connectivity) if regions is None else regions
    for t, nm in ((root, "root"), (area, "area")):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(labels.shape):
            raise AsrError(f"clean_labels: {nm} must have the shape of labels, {tuple(labels.shape)}")
    if out is None:
        out = torch.empty_like(labels)
    elif tuple(out.shape) != tuple(labels.shape):
        raise AsrError(f"clean_labels: out must be {tuple(labels.shape)}, got {tuple(out.shape)}")
    lib = _lib.load()
    stats = torch.empty((maps, 4), dtype=torch.int64, device=labels.device) if want_stats else None
    nbytes = lib.asr_clean_labels_workspace_bytes(maps, h, w)
    ws = torch.empty(max(nbytes // 4, 1), dtype=torch.int32, device=labels.device)
    call("asr_clean_labels_i32", ptr(labels, torch.int32), ptr(root, torch.int32), ptr(area, torch.int32),
         ptr(out, torch.int32), ptr(stats, torch.int64, allow_none=True), ptr(ws, torch.int32), nbytes, maps, h, w,
         int(connectivity), int(min_area), stream_ptr())
    if want_stats:
        return out, (stats[0] if labels.dim() == 2 else stats)
    return out


def check_segments(segments):
    """segments of a region-by-region score as (num_labels, connectivity, include_zero): an int L, a pair (L, connectivity) or
    a triple (L, connectivity, include_zero); 1 <= L <= 64, connectivity 4 or 8 (default 8), include_zero a bool or 0 / 1
    (default False).  Host only; ValueError otherwise."""
    conn, zero = 8, False
    if isinstance(segments, (tuple, list)):
        if not 1 <= len(segments) <= 3:
            raise ValueError(f"segments must be L, (L, connectivity) or (L, connectivity, include_zero), got {segments!r}")
        labels = _region_int(segments[0], "num_labels", "segments")
        if len(segments) > 1:
            conn = _region_int(segments[1], "connectivity", "segments")
        if len(segments) > 2:
            zero = segments[2]
            if not isinstance(zero, (bool, np.bool_)) and not (isinstance(zero, (int, np.integer)) and zero in (0, 1)):
                raise ValueError(f"segments: include_zero must be a bool, got {zero!r}")
            zero = bool(zero)
    else:
        labels = _region_int(segments, "num_labels", "segments")
    if not 1 <= labels <= _lib.MAX_SEGMENT_LABELS:
        raise ValueError(f"segments: {labels} labels (1..{_lib.MAX_SEGMENT_LABELS})")
    if conn not in (4, 8):
        raise ValueError(f"segments: connectivity {conn} (4 or 8)")
    return labels, conn, zero


def segment_match(truth, preds, num_labels=21, connectivity=8, include_zero=False, truth_regions=None, pred_regions=None,
                  want_planes=False, out=None):
    """The segments of int32 prediction maps [H, W] or [M, H, W] matched against those of ONE truth [H, W] (include/asr_hip.h,
    "segments"; asr_segment_match_i32) -> device int64 counts [M, L, 4] (TP, FP, FN, Q per label; [L, 4] for an [H, W]
    prediction), written into out when given.  truth_regions / pred_regions: the (root, area) of label_regions(truth | preds,
    connectivity), to reuse them; what is not given is labelled here.  want_planes: also (pred_match, truth_match), int32 of
    preds' shape.  The workspace comes from torch's caching allocator."""
    num_labels, connectivity, include_zero = check_segments((num_labels, connectivity, include_zero))
    maps, h, w = _region_maps(preds, "segment_match")
    if not isinstance(truth, torch.Tensor) or tuple(truth.shape) != (h, w):
        shape = tuple(truth.shape) if isinstance(truth, torch.Tensor) else type(truth)
        raise AsrError(f"segment_match: truth must be [{h}, {w}], the shape of one prediction, got {shape}")
    t_root, t_area = label_regions(truth, connectivity) if truth_regions is None else truth_regions
    p_root = label_regions(preds, connectivity)[0] if pred_regions is None else pred_regions[0]
    for t, nm, like in ((t_root, "truth root", truth), (t_area, "truth area", truth), (p_root, "predicted root", preds)):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(like.shape):
            raise AsrError(f"segment_match: the {nm} must have the shape {tuple(like.shape)}")
    shape = (maps, num_labels, 4) if preds.dim() == 3 else (num_labels, 4)
    if out is None:
        out = torch.empty(shape, dtype=torch.int64, device=preds.device)
    elif tuple(out.shape) != shape:
        raise AsrError(f"segment_match: out must be {shape}, got {tuple(out.shape)}")
    lib = _lib.load()
    planes = (torch.empty_like(preds), torch.empty_like(preds)) if want_planes else (None, None)
    nbytes = lib.asr_segment_match_workspace_bytes(maps, h, w)
    ws = torch.empty(max(nbytes // 8, 1), dtype=torch.int64, device=preds.device)
    call("asr_segment_match_i32", ptr(truth, torch.int32), ptr(t_root, torch.int32), ptr(t_area, torch.int32),
         ptr(preds, torch.int32), ptr(p_root, torch.int32), ptr(out, torch.int64), ptr(planes[0], torch.int32, allow_none=True),
         ptr(planes[1], torch.int32, allow_none=True), ptr(ws, torch.int64), nbytes, maps, h, w, num_labels,
         int(include_zero), stream_ptr())
    return (out,) + planes if want_planes else out


MAX_SWEEP_FACTORS = 256


def threshold_sweep_iou_counts(images, truth, factors, class_id, include_bg=False):
    """images [S, ...] float32 -> int64 [S, K, 4]: counts[s, k] = iou_counts(truth_s, threshold(images[s], class_id,
    th_factor=factors[k])) for every factor, in one pass over the images (asr_threshold_sweep_iou_counts_f32).  truth: int32
    with the pixel count of ONE image (shared by all) or of all S images (one label map each)."""
    s = images.shape[0] if images.dim() > 1 else 1
    per = images.numel() // s if s else 0
    if s == 0 or per == 0 or per * s != images.numel():
        raise AsrError("threshold_sweep_iou_counts: images must be a non-empty [S, ...] stack")
    if truth.numel() == per:
        shared = 1
    elif truth.numel() == per * s:
        shared = 0
    else:
        raise AsrError(f"threshold_sweep_iou_counts: truth has {truth.numel()} pixels, expected {per} or {per * s}")
    f = to_device(np.asarray(factors, dtype=np.float32).reshape(-1), device=images.device)
    k = f.numel()
    if not 1 <= k <= MAX_SWEEP_FACTORS:
        raise AsrError(f"threshold_sweep_iou_counts: {k} threshold factors (1..{MAX_SWEEP_FACTORS})")
    lib = _lib.load()
    ws_bytes = lib.asr_threshold_sweep_workspace_bytes(s, k)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=images.device)
    counts = torch.empty((s, k, 4), dtype=torch.int64, device=images.device)
    call("asr_threshold_sweep_iou_counts_f32", ptr(images), ptr(truth, torch.int32), ptr(f), ptr(ws, torch.uint8), ws_bytes,
         ptr(counts, torch.int64), per, s, k, shared, int(class_id), int(bool(include_bg)), stream_ptr())
    return counts


# ---------------------------------------------------------------------------------------------
# model layers
# ---------------------------------------------------------------------------------------------
def pack_pw_weights(w_kn):
    k, n = w_kn.shape
    lib = _lib.load()
    out = torch.empty(lib.asr_pwconv_packed_floats(k, n), dtype=f32, device=w_kn.device)
    call("asr_pwconv_pack_weights_f32", ptr(w_kn), ptr(out), k, n, stream_ptr())
    return out


def pack_pw_weights_f16x3(w_kn):
    k, n = w_kn.shape
    lib = _lib.load()
    out = torch.empty(lib.asr_pwconv_packed_floats_f16x3(k, n), dtype=f32, device=w_kn.device)
    call("asr_pwconv_pack_weights_f16x3", ptr(w_kn), ptr(out), k, n, stream_ptr())
    return out


def pwconv(x, w_packed, bias, k, n, out=None, residual=None, relu=False, ldx=None, ldy=None, ldres=None, m=None,
           sub_stride=1, h_in=0, w_in=0, f16x3=False):
    """Rows of x ([..., ldx] with the first k columns used) times packed W [k,n].  f16x3: w_packed comes from
    pack_pw_weights_f16x3 and the split-f16 kernel is used."""
    ldx = ldx or x.shape[-1]
    m = m if m is not None else x.numel() // ldx
    if out is None:
        out = torch.empty((m, n), dtype=f32, device=x.device)
        ldy = n
    ldy = ldy or out.shape[-1]
    ldres = ldres or (residual.shape[-1] if residual is not None else 0)
    call("asr_pwconv_mfma_f16x3" if f16x3 else "asr_pwconv_mfma_f32", ptr(x), ptr(w_packed), ptr(bias, allow_none=True),
         ptr(residual, allow_none=True),
         ptr(out), m, k, n, ldx, ldy, ldres, int(relu), sub_stride, h_in, w_in, stream_ptr())
    return out


def conv3x3_mfma(x, w_packed, bias, cout, stride=1, pad=1, dil=1, relu=False, f16x3=False):
    """Dense 3x3 as an implicit GEMM; w_packed from pack_pw_weights (f32 MFMA) or pack_pw_weights_f16x3 (f16x3=True)
    on the [9 * cin, cout] matrix."""
    b, h, w, cin = x.shape
    ho = (h + 2 * pad - (2 * dil + 1)) // stride + 1
    wo = (w + 2 * pad - (2 * dil + 1)) // stride + 1
    y = torch.empty((b, ho, wo, cout), dtype=f32, device=x.device)
    call("asr_conv3x3_mfma_f16x3" if f16x3 else "asr_conv3x3_mfma_f32", ptr(x), ptr(w_packed), ptr(bias, allow_none=True), ptr(y), b, h, w, cin, cout, stride,
         pad, dil, ho, wo, cin, cout, int(relu), stream_ptr())
    return y


def conv3x3_direct(x, w_hwio, bias, stride, pad_top, pad_left, out_hw, relu=False, f16x3=False):
    """Dense 3x3 for tiny cin (the stem).  f16x3=True: the split-f16 MFMA form (cin = 3, cout = 32 only)."""
    b, h, w, cin = x.shape
    cout = w_hwio.shape[-1]
    y = torch.empty((b, out_hw[0], out_hw[1], cout), dtype=f32, device=x.device)
    call("asr_conv3x3_stem_f16x3" if f16x3 else "asr_conv3x3_direct_f32", ptr(x), ptr(w_hwio), ptr(bias), ptr(y), b, h, w, cin,
         cout, stride, pad_top, pad_left, out_hw[0], out_hw[1], cin, cout, int(relu), stream_ptr())
    return y


def entry_stem_fused(x, w1_hwio, b1, w2_packed16, b2):
    """relu(conv3x3(relu(conv3x3_s2(x, w1) + b1), w2) + b2), 3 -> 32 -> 64 channels, in one kernel (even input sizes);
    w2_packed16 = pack_pw_weights_f16x3 of the [288, 64] matrix."""
    b, h, w, c = x.shape
    if c != 3 or tuple(w1_hwio.shape) != (3, 3, 3, 32):
        raise AsrError("entry_stem_fused: x [B,H,W,3] and w1 [3,3,3,32] expected")
    y = torch.empty((b, h // 2, w // 2, 64), dtype=f32, device=x.device)
    call("asr_entry_stem_f16x3", ptr(x), ptr(w1_hwio), ptr(b1), ptr(w2_packed16), ptr(b2), ptr(y), b, h, w, 3, 64, stream_ptr())
    return y


def sepconv_fused(x, w_33c, bias_dw, w_packed16, bias_pw, cout, pre_relu=False, dw_relu=False, out_relu=False):
    """A whole separable conv (depthwise 3x3 stride 1 + pointwise) in one kernel: cin in {64, 128} -> 128."""
    b, h, w, c = x.shape
    y = torch.empty((b, h, w, cout), dtype=f32, device=x.device)
    call("asr_sepconv_fused_f16x3", ptr(x), ptr(w_33c), ptr(bias_dw), ptr(w_packed16), ptr(bias_pw), ptr(y), b, h, w, c, cout, c,
         cout, int(pre_relu), int(dw_relu), int(out_relu), stream_ptr())
    return y


def dwconv3x3_split(x, w_33c, bias, stride=1, rate=1, pre_relu=False, post_relu=0):
    """Depthwise 3x3 ('same', or the explicit symmetric pad of the stride-2 sepconvs) whose output is written as
    split-f16 chunks for pwconv_presplit.  Returns (buffer [B*Ho*Wo, chunks, 32] float32-typed storage, (B, Ho, Wo), chunks)."""
    b, h, w, c = x.shape
    pad = rate
    ho, wo = (h, w) if stride == 1 else ((h + 2 * pad - (2 * rate + 1)) // stride + 1, (w + 2 * pad - (2 * rate + 1)) // stride + 1)
    chunks = (c + 31) // 32
    y = torch.empty((b * ho * wo, chunks, 32), dtype=f32, device=x.device)
    call("asr_dwconv3x3_nhwc_split_f16", ptr(x), ptr(w_33c), ptr(bias), ptr(y), b, h, w, c, stride, rate, pad, pad, ho, wo, c,
         chunks, int(pre_relu), int(post_relu), stream_ptr())
    return y, (b, ho, wo), chunks


def pwconv_presplit(x_split, w_packed16, bias, k, n, chunks, out=None, residual=None, relu=0, ldx_chunks=None, ldy=None,
                    ldres=None, m=None):
    """Pointwise conv on a split-f16 operand (dwconv3x3_split); w_packed16 from pack_pw_weights_f16x3.  ldx_chunks: chunks
    per row of x_split (default `chunks`, of which the first ceil(k / 32) are used); ldy / ldres: floats per row of out /
    residual (default: their last dimension); m: rows (default: x_split's)."""
    ldx_chunks = ldx_chunks or chunks
    m = m if m is not None else x_split.shape[0]
    if out is None:
        out = torch.empty((m, n), dtype=f32, device=x_split.device)
        ldy = n
    ldy = ldy or out.shape[-1]
    ldres = ldres or (residual.shape[-1] if residual is not None else 0)
    call("asr_pwconv_mfma_f16x3_presplit", ptr(x_split), ptr(w_packed16), ptr(bias, allow_none=True),
         ptr(residual, allow_none=True), ptr(out), m, k, n, ldx_chunks, ldy, ldres, int(relu), stream_ptr())
    return out


def aspp_dwconv3(x, w3, bias3, rates=(6, 12, 18), pre_relu=False, post_relu=True):
    """Fused three-rate ASPP depthwise: x [B,H,W,C], w3 [3,3,3,C], bias3 [3,C] -> three [B,H,W,C]."""
    b, h, w, c = x.shape
    outs = [torch.empty((b, h, w, c), dtype=f32, device=x.device) for _ in range(3)]
    call("asr_aspp_dwconv3_nhwc_f32", ptr(x), ptr(w3), ptr(bias3), ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), b, h, w, c,
         int(rates[0]), int(rates[1]), int(rates[2]), c, c, int(pre_relu), int(post_relu), stream_ptr())
    return outs


def aspp_dwconv3_split(x, w3, bias3, rates=(6, 12, 18), pre_relu=False, post_relu=True):
    """aspp_dwconv3 with its three outputs as split-f16 GEMM operands (c % 32 == 0): three buffers
    [B*H*W, c / 32, 32] of float32-typed storage for pwconv_presplit."""
    b, h, w, c = x.shape
    if c % 32:
        raise AsrError("aspp_dwconv3_split: channels must be a multiple of 32")
    outs = [torch.empty((b * h * w, c // 32, 32), dtype=f32, device=x.device) for _ in range(3)]
    call("asr_aspp_dwconv3_nhwc_split_f16", ptr(x), ptr(w3), ptr(bias3), ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), b, h, w, c,
         int(rates[0]), int(rates[1]), int(rates[2]), c, c // 32, int(pre_relu), int(post_relu), stream_ptr())
    return outs


def dwconv3x3(x, w_33c, bias, stride=1, rate=1, pad_top=None, pad_left=None, out_hw=None, pre_relu=False,
              post_relu=False, force_direct=0, out=None, ldy=None):
    """force_direct is the kernel mode: 0 auto, 1 direct, 2 streaming register window."""
    b, h, w, c = x.shape
    if pad_top is None:
        pad_top = pad_left = rate            # stride-1 'same'
    if out_hw is None:
        out_hw = (h, w)
    if out is None:
        out = torch.empty((b, out_hw[0], out_hw[1], c), dtype=f32, device=x.device)
    ldy = ldy or out.shape[-1]
    call("asr_dwconv3x3_nhwc_f32", ptr(x), ptr(w_33c), ptr(bias), ptr(out), b, h, w, c, stride, rate, pad_top, pad_left,
         out_hw[0], out_hw[1], c, ldy, int(pre_relu), int(post_relu), int(force_direct), stream_ptr())
    return out


def gap(x):
    b, h, w, c = x.shape
    y = torch.empty((b, c), dtype=f32, device=x.device)
    call("asr_gap_f32", ptr(x), ptr(y), b, h * w, c, c, stream_ptr())
    return y


def resize_bilinear(x, out_hw, out=None, ldy=None):
    b, h, w, c = x.shape
    if out is None:
        out = torch.empty((b, out_hw[0], out_hw[1], c), dtype=f32, device=x.device)
    ldy = ldy or out.shape[-1]
    call("asr_resize_bilinear_f32", ptr(x), ptr(out), b, h, w, c, out_hw[0], out_hw[1], c, ldy, stream_ptr())
    return out
