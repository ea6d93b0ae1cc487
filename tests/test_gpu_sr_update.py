"""The last stage of every SR solver step (csrc/sr.hip: sr_prior_and_update) held to the bit: the five update rules in
their eight configurations against the float32 restatement of tests/sr_update_ref.py, the solver against explicit
forward + fused-backward steps for every rule and for bilateral TV, the bilateral-TV gradient against
oracle.sr.bilateral_tv_grad (written in the kernel's pair order), its value against oracle.sr.bilateral_tv, and the
refusals of make_step.

asr_sr_backward_cfg_f32 returns x_new and the raw gradient from the same launch, and sr.hip is built without contraction,
so the rule is checked as x_new == rule(x, grad_out, slots, alpha) with no tolerance, whatever the data term did.  The
only inequality in this file is the T * 2^-52 bound of the bilateral-TV value (derived at test_btv_value).

The input generator `rule_inputs` runs on the host alone: test_sr_update_host.py imports it and proves that every mutant of
sr_update_ref.MUTANTS is told from the right rule on these very inputs."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import sr as o_sr

import sr_update_ref as R
from test_gpu_sr_shapes import ATOL_GRAD, LAM, _Problem      # _Problem builds its transforms with _transform_set

pytestmark = pytest.mark.gpu

# (H, W) <- (h, w): the smallest shapes at which each instantiation and edge exists
SHAPES = [((2, 2), (1, 1)),        # f 2: the smallest legal target, wholly inside every bilateral-TV window
          ((4, 12), (1, 3)),       # f 4
          ((6, 6), (1, 1)),        # f 6: the generic LOG2F = 0 instantiation
          ((16, 8), (2, 1)),       # f 8
          ((22, 34), (11, 17)),    # f 2: odd sizes, W just over one 32-pixel backward tile
          ((40, 72), (10, 18))]    # f 4: second 64-column block partly live
SOLVER_SHAPES = [((22, 34), (11, 17)), ((36, 60), (6, 10))]     # the second: f 6
N, B = 5, 3
SENTINEL = np.float32(7.25)
LAM_GRID = (0.0, 0.0, 0.5, 0.0)    # g = 2 * 0.5 * x: the gradient IS x, so g takes the values of GRID
GRID = np.array([0.0, 1e-12, -1e-12, 1e-3, -1e-3, 1.0, -1.0, 1e3, -1e3], np.float32)
ALPHAS = np.array([0.0031622776, 0.0, 0.00070710678], np.float32)   # three different ones in one launch, one exactly 0
BTV_ALPHAS, BTV_SHIFTS = (0.6, 0.8, 0.5, 1.0), (1, 2, 3, 4)
INVALID = -1


def _sid(shape):
    (H, W), (h, w) = shape
    return f"{H}x{W}from{h}x{w}"


@functools.lru_cache(maxsize=None)
def _prob(shape):
    """n = 5 copies, batch 3, the T0 transform set of test_gpu_sr_shapes (built by its _transform_set); host arrays only."""
    return _Problem(shape, "T0", N, 70 + SHAPES.index(shape) if shape in SHAPES else 90, batch=B)


def rule_inputs(shape, rule, kind, g=None):
    """Host inputs of one fused step of `rule` (a key of sr_update_ref.RULES) on `shape`: x, m, v, vhat [B, H, W] float32,
    alphas [B], lambdas, stripe (bool [H, W]) and g (the gradient the kernel must return when it is known on the host: the
    rule grid's, else None).  The argument g is the gradient the step will see -- the GPU test reads it back from a
    gradient-only launch first, the host test lets a random one stand in; it decides vhat alone (default: the rule grid's
    own gradient, else zero).
      m: random, of both signs (Adadelta: positive -- its accum_update is a mean of squares and goes under a square root);
      v: random positive, log-uniform over 1e-12 .. 3, down to where epsilon decides the denominator;
      vhat: twice or half the new v that g gives, at random: above it on about half the pixels, below it on the rest;
      slots the rule does not use: filled with SENTINEL (plain SGD: m is None).
    kind "general": x = the resized target plus noise, every lambda on.
    kind "grid": x drawn from GRID with a run of equal values at the start of the first row; the last column is the stripe:
      x = 0 and every used slot 0 there, where each rule must return exactly 0 change."""
    (H, W), _ = shape
    opt, flag, c0, c1, c2, used = R.RULES[rule]
    rng = np.random.default_rng([SHAPES.index(shape), list(R.RULES).index(rule), int(kind == "grid")])
    stripe = np.zeros((H, W), bool)
    if kind == "grid":
        x = rng.choice(GRID, (B, H, W))
        x[:, 0, :min(4, W - 1)] = x[:, 0, :1]
        stripe[:, W - 1] = True
        x[:, stripe] = 0.0
        lam, g_known = LAM_GRID, x.copy()
    else:
        assert kind == "general"
        x, lam, g_known = _prob(shape).x.copy(), LAM, None
    m = (rng.uniform(0.05, 1.0, x.shape) * (1.0 if rule == "adadelta" else rng.choice([-1.0, 1.0], x.shape))).astype(np.float32)
    v = (10.0 ** rng.uniform(-12.0, 0.5, x.shape)).astype(np.float32)
    if g is None:
        g = g_known if g_known is not None else np.zeros_like(x)
    g = np.asarray(g, dtype=np.float32)
    v_new = v + (g * g - v) * np.float32(c1)               # Adam's new v, as sr_update_ref.step computes it
    vhat = v_new * rng.choice([0.5, 2.0], x.shape).astype(np.float32)
    slots = dict(m=m, v=v, vhat=vhat)
    for k in slots:
        if k in used:
            slots[k][:, stripe] = 0.0
        else:
            slots[k] = np.full(x.shape, SENTINEL, np.float32)
    if rule == "sgd":
        slots["m"] = None
    return SimpleNamespace(x=np.ascontiguousarray(x, dtype=np.float32), g=g_known, alphas=ALPHAS.copy(), lam=lam, stripe=stripe,
                           used=used, **slots)


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    assert a.dtype == np.float32
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(got, want, what):
    g, w = _bits(got), _bits(want)
    assert np.array_equal(g, w), f"{what}: {int((g != w).sum())} of {g.size} elements differ"


def _cfg(rule, **kw):
    from asr_amd import ops
    opt, flag, c0, c1, c2, _ = R.RULES[rule]
    return ops.sr_config(opt, flag, c0, c1, c2, **kw)


# ---- (a) each rule, one fused step ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["general", "grid"])
@pytest.mark.parametrize("rule", list(R.RULES))
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_each_rule_one_fused_step_bit_for_bit(dev, shape, rule, kind):
    """x_new and every slot the rule uses equal sr_update_ref.step(x, grad_out, slots, alphas) bit for bit; sentinel slots,
    x, the residual and the alphas are left as they were."""
    from asr_amd import ops
    p, cfg = _prob(shape), _cfg(rule)
    opt, flag, c0, c1, c2, used = R.RULES[rule]
    yd, rot, tr, irot, itr = p.device()
    first = rule_inputs(shape, rule, kind)                 # x and the lambdas do not depend on g
    xd = ops.to_device(first.x)
    resid = ops.sr_forward_residual(xd, yd, rot, tr)
    resid_before = resid.clone()
    _, grad_only = ops.sr_backward(xd, resid, irot, itr, first.lam, cfg, state=None)
    inp = rule_inputs(shape, rule, kind, g=grad_only.cpu().numpy())
    assert np.array_equal(inp.x, first.x)
    state = {k: (None if getattr(inp, k) is None else ops.to_device(getattr(inp, k))) for k in ("m", "v", "vhat")}
    state["alphas"] = ops.to_device(inp.alphas)
    x_new, grad = ops.sr_backward(xd, resid, irot, itr, inp.lam, cfg, state=state, want_grad=True)
    _same_bits(grad, grad_only, "grad_out with and without the update")
    g = grad.cpu().numpy()
    assert np.isfinite(g).all()
    if kind == "grid":      # the grid really arrived
        nz = inp.x != 0
        assert nz.any() and (g[nz] != 0).all() and np.array_equal(np.sign(g[nz]), np.sign(inp.x[nz]))
        assert np.array_equal(g, inp.g)                    # 2 * 0.5 * x, every other term a zero
    exp_x, exp_m, exp_v, exp_vhat = R.step(opt, flag, c0, c1, c2, inp.x, g, inp.m, inp.v, inp.vhat, inp.alphas)
    if rule == "amsgrad":   # vhat above the new v on about half the pixels, below it on the rest
        above = (inp.vhat > exp_v)[:, ~inp.stripe]
        assert above.any() and not above.all()
        if above.size >= 64:
            assert 0.3 <= above.mean() <= 0.7, above.mean()
    _same_bits(x_new, exp_x, "x_new")
    for k, want in (("m", exp_m), ("v", exp_v), ("vhat", exp_vhat)):
        if want is None:
            assert state[k] is None
        elif k in used:
            _same_bits(state[k], want, k)
        else:
            assert want is getattr(inp, k) and bool(torch.all(state[k] == float(SENTINEL))), k
    _same_bits(xd, inp.x, "x")
    assert torch.equal(resid, resid_before)
    _same_bits(state["alphas"], inp.alphas, "alphas")
    if kind == "grid":      # the stripe: x = 0, slots 0, g = 0 -> no change at all, for every alpha
        s = torch.from_numpy(inp.stripe)
        assert not _bits(x_new.cpu()[:, s]).any()
    moved = x_new.cpu().numpy() != inp.x
    assert moved[0].any() and moved[2].any()
    if rule not in ("momentum", "nesterov"):               # alphas[1] == 0: image 1 moves by its momentum alone
        assert not moved[1].any()


# ---- (b) solver == explicit steps ----------------------------------------------------------------------------------
# name -> (rule, base step size, slot_init, bilateral TV)
SOLVES = {
    "momentum": ("momentum", 2e-3, {}, False),
    "nesterov": ("nesterov", 2e-3, {}, False),
    "adagrad": ("adagrad", 1e-2, {"v": 0.1}, False),
    "adadelta": ("adadelta", 1.0, {}, False),
    "adamax": ("adamax", 1e-3, {}, False),
    "adam_btv": ("adam", 1e-3, {}, True),
}
ITERS = 3


def _solve_alphas(base):
    a = np.float32(base) * (1.0 + 0.25 * np.arange(ITERS)[:, None] + 0.0625 * np.arange(B)[None, :])
    a = a.astype(np.float32)
    assert len(set(a.ravel().tolist())) == a.size          # alphas[it, b] all different
    return a


@pytest.mark.parametrize("name", list(SOLVES))
@pytest.mark.parametrize("shape", SOLVER_SHAPES, ids=_sid)
def test_solver_equals_explicit_steps_for_every_rule(dev, shape, name):
    """asr_sr_solve_cfg_f32 (K_gt + gather, the update in the last chunk's launch) for plane_chunk 0, 2 (a last chunk of one
    copy) and 1, and cut into 1 + 2 iterations through one state dict, against 3 x (asr_sr_forward_residual_f32 + the fused
    asr_sr_backward_cfg_f32): x, m, v and vhat bit for bit."""
    from asr_amd import ops
    rule, base, slot_init, btv = SOLVES[name]
    (H, W), _ = shape
    p = _prob(shape)
    yd, rot, tr, irot, itr = p.device()
    alphas = ops.to_device(_solve_alphas(base))

    def solve(chunk, cuts):
        cfg, st, it0 = _cfg(rule, use_btv=btv, plane_chunk=chunk), {}, 0
        x = ops.sr_init_target(yd, (H, W))
        for c in cuts:
            ops.sr_solve(x, yd, rot, tr, irot, itr, alphas[it0:it0 + c].contiguous(), LAM, cfg=cfg, slot_init=slot_init,
                         state=st, want_loss=False)
            it0 += c
        return x, st["m"], st["v"], st["vhat"]

    cfg = _cfg(rule, use_btv=btv)
    x = ops.sr_init_target(yd, (H, W))
    x0 = x.clone()
    slots = [torch.full_like(x, float(slot_init.get(k, 0.0))) for k in ("m", "v", "vhat")]
    for it in range(ITERS):
        resid = ops.sr_forward_residual(x, yd, rot, tr)
        x, _ = ops.sr_backward(x, resid, irot, itr, LAM, cfg,
                               state=dict(m=slots[0], v=slots[1], vhat=slots[2], alphas=alphas[it].contiguous()))
    want = [x] + slots
    assert all(bool(torch.isfinite(t).all()) for t in want) and not torch.equal(x, x0)
    for chunk, cuts in ((0, (ITERS,)), (2, (ITERS,)), (1, (ITERS,)), (0, (1, ITERS - 1)), (2, (1, ITERS - 1))):
        got = solve(chunk, cuts)
        for what, a, r in zip(("x", "m", "v", "vhat"), got, want):
            assert torch.equal(a, r), (chunk, cuts, what, float((a - r).abs().max()))


# ---- (c) bilateral-TV gradient -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _btv_x(shape):
    """[B, H, W] from the nine-value grid k / 8 (dyadic, in [0, 1]): exact ties are common, and one is forced per image."""
    (H, W), _ = shape
    x = (np.random.default_rng(80 + SHAPES.index(shape)).integers(0, 9, (B, H, W)) / 8.0).astype(np.float32)
    x[:, 0, 1] = x[:, 0, 0]
    return x


def _img(x_b):
    return torch.from_numpy(np.ascontiguousarray(x_b)[None, :, :, None])


@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
@pytest.mark.parametrize("s", BTV_SHIFTS)
@pytest.mark.parametrize("a", BTV_ALPHAS)
def test_btv_gradient_bit_for_bit(dev, a, s, shape):
    """lambdas = (0, 0.3, 0, 0): grad_out is the prior's gradient alone, and oracle.sr.bilateral_tv_grad adds the same
    float32 terms in the same pair order."""
    from asr_amd import ops
    p, x = _prob(shape), _btv_x(shape)
    yd, rot, tr, irot, itr = p.device()
    xd = ops.to_device(x)
    resid = ops.sr_forward_residual(xd, yd, rot, tr)
    cfg = ops.sr_config(use_btv=True, btv_alpha=a, btv_shift=s)
    x_new, grad = ops.sr_backward(xd, resid, irot, itr, (0.0, 0.3, 0.0, 0.0), cfg, state=None)
    assert x_new is None
    g = grad.cpu().numpy()
    ties = int((x[:, :, 1:] == x[:, :, :-1]).sum()) + int((x[:, 1:] == x[:, :-1]).sum())
    assert ties > 0
    for b in range(B):
        ref = o_sr.bilateral_tv_grad(_img(x[b]), 0.3, a, s).numpy()[0, :, :, 0]
        assert np.array_equal(g[b], ref), (b, int((g[b] != ref).sum()), float(np.abs(g[b] - ref).max()))


def test_btv_gradient_with_every_lambda_on(dev):
    """Sanity only, no new tolerance: with all four lambdas, grad_out minus the gradient of the same call with
    lambda_tv = 0 is the bilateral-TV gradient to the ATOL_GRAD of test_gpu_sr_shapes."""
    from asr_amd import ops
    shape = SHAPES[4]
    p, x = _prob(shape), _btv_x(shape)
    yd, rot, tr, irot, itr = p.device()
    xd = ops.to_device(x)
    resid = ops.sr_forward_residual(xd, yd, rot, tr)
    cfg = ops.sr_config(use_btv=True, btv_alpha=0.6, btv_shift=2)
    _, full = ops.sr_backward(xd, resid, irot, itr, LAM, cfg, state=None)
    _, no_tv = ops.sr_backward(xd, resid, irot, itr, (LAM[0], 0.0, LAM[2], LAM[3]), cfg, state=None)
    d = (full - no_tv).cpu().numpy()
    for b in range(B):
        ref = o_sr.bilateral_tv_grad(_img(x[b]), LAM[1], 0.6, 2).numpy()[0, :, :, 0]
        np.testing.assert_allclose(d[b], ref, rtol=0, atol=ATOL_GRAD)


# ---- (d) bilateral-TV value ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
@pytest.mark.parametrize("s", BTV_SHIFTS)
@pytest.mark.parametrize("a", BTV_ALPHAS)
def test_btv_value(dev, a, s, shape):
    """terms[b][1] against oracle.sr.bilateral_tv.  x is dyadic (multiples of 1/8 in [0, 1]); with a = 0.5 every weight is a
    power of two, so every product and every partial sum is representable in float64 and every summation order gives the
    same number: exact equality.  Other a: each term w * |x - x'| (two float32 factors) is exact in float64 and
    non-negative, so a sum of the T = H * W * (2s+1)(s+1) of them in ANY order is within T * 2^-53 (relative) of the true
    sum; the kernel's and the oracle's sums are two such orders, hence |got - ref| <= T * 2^-52 * ref.  The bound is the
    worst case of the arithmetic: nothing was measured to set it."""
    from asr_amd import ops
    (H, W), _ = shape
    p, x = _prob(shape), _btv_x(shape)
    yd, rot, tr, irot, itr = p.device()
    xd = ops.to_device(x)
    resid = ops.sr_forward_residual(xd, yd, rot, tr)
    terms = ops.sr_loss_terms(xd, resid, ops.sr_config(use_btv=True, btv_alpha=a, btv_shift=s)).cpu().numpy()
    T = H * W * (2 * s + 1) * (s + 1)
    for b in range(B):
        ref = o_sr.bilateral_tv(_img(x[b]), a, s)
        got = float(terms[b][1])
        assert ref > 0.0
        if a == 0.5:
            assert got == ref, (b, got, ref)
        else:
            assert abs(got - ref) <= T * 2.0 ** -52 * ref, (b, got, ref, abs(got - ref) / ref)


# ---- (e) refusals --------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(dev, lib):
    """make_step (csrc/sr.hip): a rule whose slot buffers were not given, a bilateral-TV window outside 1..4 and an unknown
    optimizer return ASR_ERR_INVALID_ARG with their message, and x_new, grad_out and the slots keep their sentinel."""
    from asr_amd import _lib, ops
    shape = SHAPES[4]
    (H, W), (h, w) = shape
    p = _prob(shape)
    yd, rot, tr, irot, itr = p.device()
    xd = ops.to_device(p.x)
    resid = ops.sr_forward_residual(xd, yd, rot, tr)
    alphas = ops.to_device(ALPHAS)
    fill = float(SENTINEL)
    x_new, grad, m, v, vhat = (torch.full_like(xd, fill) for _ in range(5))
    ptr = lambda t: None if t is None else _lib.ptr(t)

    def call(cfg, m_, v_, vhat_):
        return lib.asr_sr_backward_cfg_f32(ptr(xd), ptr(x_new), ptr(resid), ptr(irot), ptr(itr), ptr(m_), ptr(v_), ptr(vhat_),
                                           ptr(alphas), ptr(grad), B, N, H, W, h, w, *LAM, C.byref(cfg), _lib.stream_ptr())

    slots_msg = lambda opt: f"optimizer {opt} needs slot buffers that were not given".encode()
    bad_opt = _cfg("adam")
    bad_opt.optimizer = 5
    cases = [(_cfg("momentum"), None, v, vhat, slots_msg(1)),
             (_cfg("nesterov"), None, v, vhat, slots_msg(1)),
             (_cfg("adagrad"), m, None, vhat, slots_msg(2)),
             (_cfg("adadelta"), None, v, vhat, slots_msg(3)),
             (_cfg("adadelta"), m, None, vhat, slots_msg(3)),
             (_cfg("adamax"), None, v, vhat, slots_msg(4)),
             (_cfg("adamax"), m, None, vhat, slots_msg(4)),
             (_cfg("amsgrad"), m, v, None, slots_msg(0)),
             (_cfg("adam", use_btv=True, btv_shift=0), m, v, vhat, b"btv_shift 0 outside [1, 4]"),
             (_cfg("adam", use_btv=True, btv_shift=5), m, v, vhat, b"btv_shift 5 outside [1, 4]"),
             (bad_opt, m, v, vhat, b"unknown optimizer 5")]
    for i, (cfg, m_, v_, vhat_, msg) in enumerate(cases):
        assert call(cfg, m_, v_, vhat_) == INVALID, i
        assert msg in lib.asr_last_error(), (i, lib.asr_last_error())
    torch.cuda.synchronize()
    for t in (x_new, grad, m, v, vhat):
        assert bool(torch.all(t == fill))
    # accepted: the rules that do not read the missing slot
    assert call(_cfg("sgd"), None, v, vhat) == 0
    torch.cuda.synchronize()
    assert bool(torch.all(v == fill)) and bool(torch.all(vhat == fill)) and not bool(torch.any(x_new == fill))
    x_new.fill_(fill)
    m.fill_(0.25)
    v.fill_(0.5)
    assert call(_cfg("adam"), m, v, None) == 0
    torch.cuda.synchronize()
    assert bool(torch.all(vhat == fill)) and not bool(torch.any(x_new == fill)) and not bool(torch.any(v == 0.5))
