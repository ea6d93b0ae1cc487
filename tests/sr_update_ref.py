"""The update rules of the SR solver's last stage (csrc/sr.hip: sr_prior_and_update) restated in numpy float32, one IEEE
operation per statement, in the order of the table in include/asr_hip.h ("the other optimisers and priors") -- which is the
order of the Keras* classes of oracle/sr.py (test_sr_update_host.py holds the two together bit for bit).
TEST INFRASTRUCTURE ONLY.

np.sqrt and / are correctly rounded; there is no np.power and no fused multiply-add.  Subnormals are excluded: TensorFlow's
CPU threads and the GPU may treat them differently and nothing here pins that, so `step` asserts that none of its inputs,
outputs or named intermediates is one (assert_normal) -- a condition on the test inputs, checked on the CPU."""
import numpy as np

F = np.float32
OPT_ADAM, OPT_SGD, OPT_ADAGRAD, OPT_ADADELTA, OPT_ADAMAX = 0, 1, 2, 3, 4      # ASR_OPT_*
MIN_NORMAL = 2.0 ** -126

_B1, _B2, _EPS, _MOM, _RHO = F(0.9), F(0.999), F(1e-7), F(0.9), F(0.95)
# name -> (optimizer, flag, c0, c1, c2, slots the rule reads and writes): the eight configurations of the sweeps
RULES = {
    "adam":     (OPT_ADAM, 0, F(1) - _B1, F(1) - _B2, _EPS, ("m", "v")),
    "amsgrad":  (OPT_ADAM, 1, F(1) - _B1, F(1) - _B2, _EPS, ("m", "v", "vhat")),
    "sgd":      (OPT_SGD, 0, F(0), F(0), F(0), ()),
    "momentum": (OPT_SGD, 0, _MOM, F(0), F(0), ("m",)),
    "nesterov": (OPT_SGD, 1, _MOM, F(0), F(0), ("m",)),
    "adagrad":  (OPT_ADAGRAD, 0, F(0), F(0), _EPS, ("v",)),
    "adadelta": (OPT_ADADELTA, 0, _RHO, F(1) - _RHO, _EPS, ("m", "v")),
    "adamax":   (OPT_ADAMAX, 0, F(1) - _B1, _B2, _EPS, ("m", "v")),
}


def assert_normal(*arrays):
    """Every non-zero finite value has magnitude >= 2^-126 (None is skipped)."""
    for a in arrays:
        if a is None:
            continue
        a = np.asarray(a)
        mag = np.abs(a[np.isfinite(a) & (a != 0)].astype(np.float64))
        assert mag.size == 0 or mag.min() >= MIN_NORMAL, f"subnormal value {mag.min():.3e}"


def _per_image(alpha, x):
    a = np.asarray(alpha, dtype=F)
    return a.reshape((-1,) + (1,) * (x.ndim - 1)) if a.ndim == 1 else a


def _f32(*arrays):
    for a in arrays:
        assert a is None or a.dtype == np.float32, a.dtype


def step(optimizer, flag, c0, c1, c2, x, g, m, v, vhat, alpha, _mutant=None):
    """One update of x [B, ...] with gradient g: (x_new, m, v, vhat), all float32.  alpha: one value per image ([B]) or a
    scalar.  Slots the rule does not use come back untouched (the same object, None included).  _mutant: MUTANTS only."""
    c0, c1, c2 = F(c0), F(c1), F(c2)
    _f32(x, g, m, v, vhat)
    a = _per_image(alpha, x)
    if _mutant == "alpha0" and a.ndim:
        a = np.broadcast_to(a.reshape(-1)[0], a.shape)
    named = []                                             # the intermediates g*g, acc, upd
    ins = dict(m=m, v=v, vhat=vhat)
    if optimizer == OPT_SGD:
        used = ()
        if c0 == 0:
            xn = x - g * a
        else:
            used = ("m",)
            acc = m * c0 - g * a
            named.append(acc)
            if not flag:
                xn = x + acc
            elif _mutant == "nesterov_acc":
                xn = x + acc
            else:
                xn = x + (acc * c0 - g * a)
            m = acc
    elif optimizer == OPT_ADAGRAD:
        used = ("v",)
        gg = g * g
        acc = v + gg
        named += [gg, acc]
        if _mutant == "eps_in_sqrt":
            xn = x - (g * a) / np.sqrt(acc + c2)
        else:
            xn = x - (g * a) / (np.sqrt(acc) + c2)
        v = acc
    elif optimizer == OPT_ADADELTA:                        # c0 = rho, c1 = 1 - rho; v = accum, m = accum_update
        used = ("m", "v")
        gg = g * g
        acc = v * c0 + gg * c1
        au = m
        upd = np.sqrt(au + c2) * (F(1) / np.sqrt(acc + c2)) * g
        au_new = au * c0 + (upd * upd) * c1
        named += [gg, acc, upd]
        if _mutant == "adadelta_late_read":               # the update re-derived from accum_update after it was written
            upd = np.sqrt(au_new + c2) * (F(1) / np.sqrt(acc + c2)) * g
        xn = x - upd * a
        m, v = au_new, acc
    elif optimizer == OPT_ADAMAX:                          # c0 = 1 - beta1, c1 = beta2
        used = ("m", "v")
        mm = m + (g - m) * c0
        vv = np.maximum(c1 * v, g if _mutant == "adamax_no_abs" else np.abs(g))
        xn = x - a * (mm / (vv + c2))
        m, v = mm, vv
    else:                                                  # Adam / AMSGrad: c0 = 1 - beta1, c1 = 1 - beta2
        assert optimizer == OPT_ADAM
        used = ("m", "v", "vhat") if flag else ("m", "v")
        gg = g * g
        mm = m + (g - m) * c0
        vv = v + (gg - v) * c1
        named += [gg, vv]
        if flag:
            root_of = vv if _mutant == "vhat_not_maxed" else np.maximum(vhat, vv)
            vhat = root_of
        else:
            root_of = vv
        if _mutant == "eps_in_sqrt":
            denom = np.sqrt(root_of + c2)
        else:
            denom = np.sqrt(root_of) + c2
        xn = x - (mm * a) / denom
        m, v = mm, vv
    if _mutant is None:
        outs = dict(m=m, v=v, vhat=vhat)
        assert_normal(x, g, a, xn, *named, *(ins[k] for k in used), *(outs[k] for k in used))
    _f32(xn, m, v, vhat)
    return xn, m, v, vhat


def _mutant(kind):
    def f(optimizer, flag, c0, c1, c2, x, g, m, v, vhat, alpha):
        return step(optimizer, flag, c0, c1, c2, x, g, m, v, vhat, alpha, _mutant=kind)
    f.__name__ = kind
    return f


# (name, the RULES it mutates, a wrong `step`): used ONLY to prove that the test inputs tell the right rule from these
MUTANTS = [
    ("epsilon inside the square root", ("adam", "amsgrad", "adagrad"), _mutant("eps_in_sqrt")),
    ("vhat not maxed", ("amsgrad",), _mutant("vhat_not_maxed")),
    ("Nesterov steps by acc instead of acc*c0 - g*alpha", ("nesterov",), _mutant("nesterov_acc")),
    ("Adadelta reads accum_update after writing it", ("adadelta",), _mutant("adadelta_late_read")),
    ("Adamax max(c1*v, g) without the absolute value", ("adamax",), _mutant("adamax_no_abs")),
    ("image 0's alpha used for every image", tuple(RULES), _mutant("alpha0")),
]
