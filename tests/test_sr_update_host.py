"""The yardsticks of tests/test_gpu_sr_update.py, checked without a device:
  - sr_update_ref.step is oracle.sr.Keras{Adam, SGD, Adagrad, Adadelta, Adamax}.apply bit for bit, from non-fresh slots;
  - every mutant of sr_update_ref.MUTANTS gives other bits than `step` on the GPU test's own inputs (its generator is
    imported, not copied), so that test cannot pass by having nothing to say;
  - oracle.sr.bilateral_tv is exact on dyadic inputs with alpha = 0.5 (rational arithmetic);
  - make_step's slot refusals through the C ABI (refused before any launch: the pointers are never dereferenced)."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch

from oracle import sr as o_sr

import sr_update_ref as R
from test_gpu_sr_update import ALPHAS, SHAPES, _cfg, _sid, rule_inputs

F = np.float32
FAKE = 1 << 20                      # non-null, never dereferenced on the host: every call below is refused before a launch
INVALID = -1


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def _oracle(rule):
    """(the oracle's optimiser with a non-zero step counter, alpha as the oracle computes it for the coming step)."""
    if rule in ("adam", "amsgrad"):
        o = o_sr.KerasAdam(1e-3, amsgrad=rule == "amsgrad")
        alpha = o.alpha
    elif rule in ("sgd", "momentum", "nesterov"):
        o = o_sr.KerasSGD(2e-3, 0.0 if rule == "sgd" else 0.9, rule == "nesterov")
        alpha = lambda: o.learning_rate
    elif rule == "adagrad":
        o = o_sr.KerasAdagrad(1e-2)
        alpha = lambda: o.learning_rate
    elif rule == "adadelta":
        o = o_sr.KerasAdadelta(1.0)
        alpha = lambda: o.learning_rate
    else:
        assert rule == "adamax"
        o = o_sr.KerasAdamax(1e-3)
        alpha = lambda: F(o.learning_rate / (F(1.0) - np.power(o.beta_1, F(o.iterations + 1), dtype=np.float32)))
    o.iterations = 4
    return o, alpha


@pytest.mark.parametrize("rule", list(R.RULES))
def test_step_is_the_oracles_apply_bit_for_bit(rule):
    """3 consecutive steps from non-fresh slots with random gradients (a flat patch of zeros among them)."""
    opt, flag, c0, c1, c2, used = R.RULES[rule]
    o, alpha = _oracle(rule)
    # the table of include/asr_hip.h: what c0, c1, c2 mean for this optimiser
    if opt == R.OPT_ADAM:
        assert (c0, c1, c2, bool(flag)) == (F(1) - o.beta_1, F(1) - o.beta_2, o.epsilon, o.amsgrad)
    elif opt == R.OPT_SGD:
        assert (c0, bool(flag)) == (o.momentum, o.nesterov)
    elif opt == R.OPT_ADAGRAD:
        assert c2 == o.epsilon
    elif opt == R.OPT_ADADELTA:
        assert (c0, c1, c2) == (o.rho, F(1) - o.rho, o.epsilon)
    else:
        assert (c0, c1, c2) == (F(1) - o.beta_1, o.beta_2, o.epsilon)
    rng = np.random.default_rng(list(R.RULES).index(rule))
    shape = (2, 9, 13)
    x = rng.standard_normal(shape).astype(np.float32)
    m = (rng.uniform(0.05, 1.0, shape) * (1.0 if rule == "adadelta" else rng.choice([-1.0, 1.0], shape))).astype(np.float32)
    v = rng.uniform(0.05, 2.0, shape).astype(np.float32)
    vhat = (v * rng.choice([0.5, 2.0], shape)).astype(np.float32)
    var = torch.from_numpy(x.copy())
    slots = {k: torch.from_numpy(a.copy()) for k, a in (("m", m), ("v", v), ("vhat", vhat))}
    for it in range(3):
        g = rng.standard_normal(shape).astype(np.float32)
        g[0, 2:4, 3:7] = 0.0
        a = alpha()
        x, m, v, vhat = R.step(opt, flag, c0, c1, c2, x, g, m, v, vhat, a)
        o.apply(var, torch.from_numpy(g.copy()), slots)
        assert np.array_equal(_bits(x), _bits(var.numpy())), (rule, it, "x")
        for k, mine in (("m", m), ("v", v), ("vhat", vhat)):
            assert np.array_equal(_bits(mine), _bits(slots[k].numpy())), (rule, it, k)
    assert o.iterations == 7


def test_unused_slots_come_back_untouched():
    x = np.ones((1, 2, 2), np.float32)
    s = [np.full_like(x, 7.25) for _ in range(3)]
    for rule, (opt, flag, c0, c1, c2, used) in R.RULES.items():
        out = R.step(opt, flag, c0, c1, c2, x, x, None if rule == "sgd" else s[0], s[1], s[2], F(0.5))
        for k, before, after in zip(("m", "v", "vhat"), s, out[1:]):
            if k not in used:
                assert after is (None if (rule, k) == ("sgd", "m") else before), (rule, k)
            else:
                assert after is not before
    assert all(np.all(t == 7.25) for t in s)


def test_assert_normal():
    R.assert_normal(np.array([0.0, -0.0, 2.0 ** -126, -1e30, np.inf, np.nan], np.float32), None)
    for bad in (np.float32(2.0 ** -127), np.array([1.0, -1e-40], np.float32)):
        with pytest.raises(AssertionError):
            R.assert_normal(bad)
    with pytest.raises(AssertionError):                    # an intermediate: g * g
        opt, flag, c0, c1, c2, _ = R.RULES["adagrad"]
        g = np.full((1, 1, 1), 1e-20, np.float32)
        R.step(opt, flag, c0, c1, c2, g, g, None, np.ones_like(g), None, F(1e-3))


@pytest.mark.parametrize("kind", ["general", "grid"])
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_every_mutant_is_told_from_the_rule_on_the_gpu_tests_inputs(shape, kind):
    """rule_inputs is the generator the GPU test uploads from.  On the rule grid the kernel's gradient is known here (it is
    x); for the general set, whose gradient only the device knows, a random one of the same scale stands in.  Every shape
    but the 2 x 2 one must tell every mutant from the rule, on both input sets."""
    for rule, (opt, flag, c0, c1, c2, used) in R.RULES.items():
        inp = rule_inputs(shape, rule, kind)
        assert inp.alphas[1] == 0.0 and len(set(inp.alphas.tolist())) == 3 and np.array_equal(inp.alphas, ALPHAS)
        g = inp.g
        if g is None:
            g = np.random.default_rng(5).standard_normal(inp.x.shape).astype(np.float32)
            inp = rule_inputs(shape, rule, kind, g=g)
        args = (opt, flag, c0, c1, c2, inp.x, g, inp.m, inp.v, inp.vhat, inp.alphas)
        want = R.step(*args)                               # asserts that nothing is subnormal
        if kind == "grid":
            st = inp.stripe
            assert st.any() and not inp.x[:, st].any() and not _bits(want[0][:, st]).any()
            for k, t in zip(("m", "v", "vhat"), want[1:]):
                assert k not in used or not _bits(t[:, st]).any(), (rule, k)
            assert np.array_equal(inp.g, inp.x)
        if rule == "amsgrad":       # vhat above the new v on about half the pixels, below it on the rest
            above = (inp.vhat > want[2])[:, ~inp.stripe]
            assert above.any() and not above.all()
            assert above.size < 64 or 0.3 <= above.mean() <= 0.7
        if inp.x[0].size < 16:          # 2 x 2: two free pixels per image on the grid; it is there for the window edge, not the rules
            continue
        for name, rules, mutant in R.MUTANTS:
            if rule not in rules:
                continue
            got = mutant(*args)
            differs = any(a is not None and not np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, want))
            assert differs, (name, rule)


def test_the_rule_grid_holds_the_listed_values():
    from test_gpu_sr_update import GRID
    assert sorted(GRID.tolist()) == sorted(np.array([0.0, 1e-12, -1e-12, 1e-3, -1e-3, 1, -1, 1e3, -1e3], np.float32).tolist())
    seen = set()
    for shape in SHAPES:
        inp = rule_inputs(shape, "adam", "grid")
        seen |= set(inp.x.ravel().tolist())
        assert np.all(inp.x[:, 0, :min(4, inp.x.shape[2] - 1)] == inp.x[:, 0, :1])      # the run of equal values
    assert seen == set(GRID.tolist())


@pytest.mark.parametrize("H,W", [(2, 2), (4, 6), (22, 34)])
def test_bilateral_tv_is_exact_on_dyadic_inputs(H, W):
    """x a multiple of 2^-8 in [0, 1], alpha = 0.5: every |difference| is a multiple of 2^-8, every weight a power of two,
    every partial sum below 2^53 * 2^-16 -- all representable in float64, so oracle.sr.bilateral_tv returns the rational
    value itself (and so does any other summation order)."""
    k = np.random.default_rng(H * 100 + W).integers(0, 257, (H, W))
    x = torch.from_numpy((k / 256.0).astype(np.float32)[None, :, :, None])
    assert np.array_equal(x.numpy()[0, :, :, 0] * 256.0, k)
    for s in (1, 2, 3, 4):
        pad = np.zeros((H + 2 * s, W + 2 * s), np.int64)
        pad[s:s + H, s:s + W] = k
        exact = Fraction(0)
        for h in range(-s, s + 1):
            for v in range(0, s + 1):
                shifted = pad[s - v:s - v + H, s - h:s - h + W]          # translate(x, (h, v))(q) = x(q - (h, v)), zero outside
                exact += Fraction(int(np.abs(k - shifted).sum()), 256) * Fraction(1, 2 ** (abs(h) + v))
        got = o_sr.bilateral_tv(x, 0.5, s)
        assert Fraction(got) == exact, (s, got, float(exact))


def test_make_step_refuses_missing_slots_before_any_launch(lib):
    def call(cfg, m, v, vhat, x_new=FAKE + 4096):
        return lib.asr_sr_backward_cfg_f32(FAKE, x_new, FAKE, FAKE, FAKE, m, v, vhat, FAKE, FAKE, 1, 2, 8, 8, 4, 4,
                                           1.0, 0.3, 0.0, 0.0, C.byref(cfg), None)

    msg = lambda opt: f"optimizer {opt} needs slot buffers that were not given".encode()
    for rule, slots, opt in (("momentum", (None, FAKE, FAKE), 1), ("nesterov", (None, None, None), 1),
                             ("adagrad", (FAKE, None, FAKE), 2), ("adadelta", (None, FAKE, FAKE), 3),
                             ("adadelta", (FAKE, None, FAKE), 3), ("adamax", (None, FAKE, FAKE), 4),
                             ("adamax", (FAKE, None, FAKE), 4), ("amsgrad", (FAKE, FAKE, None), 0),
                             ("adam", (None, FAKE, FAKE), 0), ("adam", (FAKE, None, FAKE), 0)):
        assert call(_cfg(rule), *slots) == INVALID, (rule, slots)
        assert msg(opt) in lib.asr_last_error(), (rule, lib.asr_last_error())
    for shift in (0, 5, -1):
        assert call(_cfg("adam", use_btv=True, btv_shift=shift), FAKE, FAKE, FAKE) == INVALID
        assert f"btv_shift {shift} outside [1, 4]".encode() in lib.asr_last_error()
    for bad in (5, -1):
        cfg = _cfg("adam")
        cfg.optimizer = bad
        assert call(cfg, FAKE, FAKE, FAKE) == INVALID and f"unknown optimizer {bad}".encode() in lib.asr_last_error()
