"""The case table of tests/test_gpu_sr_option_shapes.py: which option (data term, per-measurement weights, edge weights,
update rule, monitor, plane chunking) runs on which geometry of tests/test_gpu_sr_shapes.py, and `instantiations`, the dispatch
of csrc/sr.hip (sr_solve_impl, sr_backward_impl, sr_loss_terms_impl, asr_sr_forward_residual[_dt]_f32, asr_sr_data_bound_f32)
restated in plain Python: the kernel instantiations a case launches.  HOST ONLY -- nothing here touches a device;
tests/test_sr_option_cases_host.py holds the table against the source text of sr.hip.  TEST INFRASTRUCTURE ONLY.

A case is (shape key, transform kind, data term, weights mode, tv-weights mode, rule, monitor mode, plane_chunk):
  shape      a key of test_gpu_sr_shapes.SHAPES (A, E: f 4; B: f 2; C: f 8; D: f 6, the generic-factor instantiation)
  kind       T0 (pure translations, affine rotations) or T2 (affine-but-not-pure and projective translate stages, one
             projective rotation), test_gpu_sr_shapes._transform_set's
  loss       "l2", "l1" or "huber"
  weights    "none", "batch" ([B, N, h, w]) or "shared" ([N, h, w], stride 0)
  tvw        "none", "batch" ([B, H, W]) or "shared" ([H, W])
  rule       a solve under "adam" (AMSGrad), "sgd" or "pd" (primal-dual); "steps": the loop of single steps
             (asr_sr_forward_residual[_dt]_f32 + the fused backward + the loss terms); "bound": asr_sr_data_bound_f32
  monitor    "off", "trace" (patience 0: never stops) or "stop"
  chunk      plane_chunk (0: all copies at once; 2 with n = 5: a last chunk of one copy)
Every problem has n = 5 copies (copy 3 wholly out of frame, copy 4 turned by pi / 2) and batch 2 with one transform set per
image: test_gpu_sr_shapes._problem(shape, kind, N_COPIES, SEED), the very problems that suite holds against the oracle."""
import os
import re
from collections import namedtuple

import numpy as np

from test_gpu_sr_shapes import OUT_OF_FRAME, SHAPES, _Problem, _problem, _proj_range, _transform_set   # noqa: F401 (re-exported)

N_COPIES, BATCH, SEED = 5, 2, 50
Case = namedtuple("Case", "shape kind loss weights tvw rule monitor chunk")

LOSSES = ("l2", "l1", "huber")
MODES = ("none", "batch", "shared")
RULES = ("adam", "sgd", "pd", "steps", "bound")
MONITORS = ("off", "trace", "stop")


def problem(case_or_shape, kind=None):
    """The shared, never-modified problem of a case (or of a shape key and a kind)."""
    if isinstance(case_or_shape, Case):
        case_or_shape, kind = case_or_shape.shape, case_or_shape.kind
    return _problem(case_or_shape, kind, N_COPIES, SEED)


def factor(shape):
    (H, W), (h, w) = SHAPES[shape]
    assert H % h == 0 and W % w == 0 and H // h == W // w
    return H // h


def log2f(f):
    """The LOG2F template argument of a factor: 2 -> 1, 4 -> 2, 8 -> 3, any other even factor -> 0 (integer / and %)."""
    return {2: 1, 4: 2, 8: 3}.get(f, 0)


def _b(flag):
    return "true" if flag else "false"


def has_data_term(case):
    """Whether ops hands the library an asr_sr_data_term: anything but L2 without weights -- and always under the monitor,
    which has the *_dt form only."""
    return case.loss != "l2" or case.weights != "none" or (case.monitor != "off" and case.rule in ("adam", "sgd", "pd"))


def instantiations(case, want_loss=True):
    """The set of kernel names (template arguments as csrc/sr.hip writes them at the launch, without blanks) that the case
    launches.  want_loss: whether the solve is asked for the loss terms of its last iteration."""
    case = Case(*case)
    assert case.shape in SHAPES and case.kind in ("T0", "T2") and case.loss in LOSSES and case.weights in MODES
    assert case.tvw in MODES and case.rule in RULES and case.monitor in MONITORS and case.chunk >= 0
    L = log2f(factor(case.shape))
    dt, wtv, mon = has_data_term(case), case.tvw != "none", case.monitor != "off"
    out = set()
    if case.rule == "bound":                                   # asr_sr_data_bound_f32: L2 with the weights, no prior, no monitor
        assert case.loss == "l2" and not wtv and not mon
        return {"sr_affine_flags_kernel", "sr_bound_next_v_kernel", "sr_forward_residual_kernel<true,true>",
                f"sr_grad_translate_kernel<{L}>", "sr_backward_gather_kernel<false>", "sr_bound_maxima_kernel",
                "sr_bound_out_kernel"}
    if case.rule == "steps":                                   # the explicit one-step entry points + sr_loss_terms_impl
        assert not mon
        out.add("sr_forward_residual_kernel<false,true>" if dt else "sr_forward_residual_kernel<false>")
        out.add(f"sr_backward_adam_kernel<{L},{_b(wtv)}>")
        out.add("sr_loss_df_dt_kernel" if dt else "sr_loss_df_kernel")
        out.add(f"sr_loss_prior_kernel<{_b(wtv)}>")
        return out
    # sr_solve_impl
    pd = case.rule == "pd"
    assert not (pd and case.loss == "l1")                      # refused: the rule needs a smooth data term
    out.add("sr_affine_flags_kernel")
    if mon:
        out |= {"sr_mon_init_kernel", "sr_forward_residual_kernel<true,true,true>", "sr_mon_loss_df_kernel",
                f"sr_mon_loss_prior_kernel<{_b(wtv)}>", "sr_mon_decide_kernel", f"sr_grad_translate_kernel<{L},true>"}
        out.add(f"sr_backward_gather_pd_kernel<{_b(wtv)},true>" if pd else f"sr_backward_gather_kernel<{_b(wtv)},true>")
        return out
    out.add("sr_forward_residual_kernel<true,true>" if dt else "sr_forward_residual_kernel<true>")
    if want_loss:
        out.add("sr_loss_df_dt_kernel" if dt else "sr_loss_df_kernel")
        out.add(f"sr_loss_prior_kernel<{_b(wtv)}>")
    out.add(f"sr_grad_translate_kernel<{L}>")
    out.add(f"sr_backward_gather_pd_kernel<{_b(wtv)}>" if pd else f"sr_backward_gather_kernel<{_b(wtv)}>")
    return out


# ---- the option kernels of csrc/sr.hip, written out by hand ------------------------------------------------------------------------
OPTION_KERNELS = frozenset(
    ["sr_forward_residual_kernel<false>", "sr_forward_residual_kernel<false,true>", "sr_forward_residual_kernel<true>",
     "sr_forward_residual_kernel<true,true>", "sr_forward_residual_kernel<true,true,true>"]
    + [f"sr_grad_translate_kernel<{L}{m}>" for L in (1, 2, 3, 0) for m in ("", ",true")]
    + [f"sr_backward_adam_kernel<{L},{w}>" for L in (1, 2, 3, 0) for w in ("false", "true")]
    + ["sr_backward_gather_kernel<false>", "sr_backward_gather_kernel<true>", "sr_backward_gather_kernel<false,true>",
       "sr_backward_gather_kernel<true,true>"]
    + ["sr_backward_gather_pd_kernel<false>", "sr_backward_gather_pd_kernel<true>", "sr_backward_gather_pd_kernel<false,true>",
       "sr_backward_gather_pd_kernel<true,true>"]
    + ["sr_loss_prior_kernel<false>", "sr_loss_prior_kernel<true>", "sr_mon_loss_prior_kernel<false>",
       "sr_mon_loss_prior_kernel<true>", "sr_loss_df_dt_kernel", "sr_mon_loss_df_kernel", "sr_bound_maxima_kernel",
       "sr_bound_next_v_kernel", "sr_bound_out_kernel"])
# launched by the same entry points, with no option in their arguments
SOLVER_HELPERS = frozenset(["sr_affine_flags_kernel", "sr_loss_df_kernel", "sr_mon_init_kernel", "sr_mon_decide_kernel"])
# the other kernels of the file: no solver entry point launches them
OTHER_KERNELS = frozenset(["sr_init_kernel", "sr_tv_edge_weights_kernel", "sr_realign_kernel<0>", "sr_realign_kernel<1>",
                           "sr_realign_kernel<2>", "sr_realign_select_kernel", "sr_realign_covered_kernel",
                           "sr_realign_covered_median_kernel", "sr_realign_moments_kernel<false>",
                           "sr_realign_moments_kernel<true>"])

# the sections of sr.hip that live in files of their own (#include "sr_*_kernels.h"), hand-written like the lists above
RW_KERNELS = frozenset(["sr_rw_energy_kernel", "sr_rw_weights_kernel", "sr_rw_apply_kernel", "sr_rw_rearm_kernel"])
ADJ_GATHER_KERNELS = frozenset(f"sr_backward_gather{pd}_adj_kernel<{w},{m}>" for pd in ("", "_pd") for w in ("false", "true")
                               for m in ("false", "true"))
ADJ_KERNELS = frozenset(["sr_adjoint_flags_kernel"]) | ADJ_GATHER_KERNELS

_KERNEL = r"sr_[a-z0-9_]+_kernel(?![A-Za-z0-9_])(?:\s*<[^<>()]*>)?"


def spliced_source(path):
    """The text of csrc/sr.hip as the compiler sees its kernels: every `#include "sr_*_kernels.h"` line replaced by the text of
    that file (looked up beside `path`), so that the kernels and launch selectors of the included sections are read too."""
    here = os.path.dirname(os.path.abspath(path))

    def section(m):
        with open(os.path.join(here, m.group(1))) as f:
            return f.read()

    with open(path) as f:
        return re.sub(r'^[ \t]*#include[ \t]+"(sr_[a-z0-9_]+_kernels\.h)"[ \t]*$', section, f.read(), flags=re.M)


def source_instantiations(text):
    """Every kernel form that csrc/sr.hip hands to a launch: the first argument of hipLaunchKernelGGL, and every
    `sr_..._kernel<...>` in a statement that selects a kernel (a `return`, or a `?:` initialiser).  A template argument that is
    itself a bool template parameter of the selecting function (sr_backward_kernel_of<WTV>) is expanded to both values."""
    found = set()
    for m in re.finditer(r"hipLaunchKernelGGL\(\s*\(?\s*(" + _KERNEL + r")", text):
        found.add(m.group(1))
    for line in text.splitlines():
        s = line.strip()
        if "return " in s or ("?" in s and ":" in s and "=" in s and "hipLaunchKernelGGL" not in s):
            found.update(re.findall(_KERNEL + r"(?=\s*[;:])", s))
    out = set()
    for name in found:
        name = re.sub(r"\s+", "", name)
        params = re.findall(r"\b[A-Z][A-Z0-9_]*\b", name)
        if not params:
            out.add(name)
            continue
        assert len(params) == 1, name
        out.update(name.replace(params[0], v) for v in ("false", "true"))
    return out


# ---- the table ---------------------------------------------------------------------------------------------------------------------
def neutral_variants(shape, kind):
    """Section a on one geometry: each option on in the instantiation and neutral in value, alone (AMSGrad, all copies at
    once) and all together (AMSGrad; SGD; AMSGrad with a last chunk of one copy)."""
    alone = [("huber", "none", "none", "off"), ("huber", "batch", "none", "off"), ("huber", "shared", "none", "off"),
             ("l2", "none", "batch", "off"), ("l2", "none", "shared", "off"), ("l2", "none", "none", "trace")]
    out = [Case(shape, kind, l, w, t, "adam", m, 0) for l, w, t, m in alone]
    out.append(Case(shape, kind, "huber", "shared", "batch", "adam", "trace", 0))
    out.append(Case(shape, kind, "huber", "batch", "shared", "sgd", "trace", 0))
    out.append(Case(shape, kind, "huber", "batch", "shared", "adam", "trace", 2))
    return out


def plain(case):
    """The anchor of a neutral case: the same geometry and rule with every option off, all copies at once."""
    return Case(case.shape, case.kind, "l2", "none", "none", case.rule, "off", 0)


def steps_of(case):
    """The loop of single steps a split solve is held against."""
    return case._replace(rule="steps", monitor="off", chunk=0)


NEUTRAL_GEOMETRIES = [("B", "T0"), ("C", "T2"), ("D", "T2"), ("D", "T0"), ("E", "T2"), ("A", "T0")]
A_CASES = [c for g in NEUTRAL_GEOMETRIES for c in neutral_variants(*g)]

# b: options with effect, the split solve against the loop of single steps; each for plane_chunk 0, 2 and 1
B_OPTIONS = [("C", "T2", "huber", "batch", "batch"), ("D", "T0", "huber", "batch", "batch"),
             ("D", "T2", "l1", "shared", "shared"), ("B", "T0", "l1", "shared", "shared"),
             ("A", "T2", "l2", "batch", "shared"), ("C", "T0", "l2", "batch", "shared")]
B_CASES = [Case(*o, "adam", "off", chunk) for o in B_OPTIONS for chunk in (0, 2, 1)]
B_STEPS = [steps_of(Case(*o, "adam", "off", 0)) for o in B_OPTIONS]
# b, second bullet: q and r of the forward kernel under all three losses, per-image and shared weights
B_FORWARD_GEOMETRIES = [("C", "T2"), ("D", "T2"), ("B", "T0"), ("E", "T0")]
B_FORWARD = [Case(s, k, l, w, "none", "steps", "off", 0) for s, k in B_FORWARD_GEOMETRIES for l in LOSSES for w in ("batch", "shared")]

# c: primal-dual on f 8, f 6 and the narrow plane, general transforms (and once pure translations); WTV off / on
C_GEOMETRIES = [("C", "T2"), ("D", "T2"), ("A", "T2"), ("D", "T0")]
C_CASES = [Case(s, k, "l2" if tvw == "none" else "huber", "none" if tvw == "none" else "batch", tvw, "pd", "off", 0)
           for s, k in C_GEOMETRIES for tvw in ("none", "batch")]
# ... with a monitor that never stops: <WTV, true> against <WTV> (the same case with the monitor off)
C_MONITORED = [Case(s, k, "huber", "batch", "shared", "pd", "trace", chunk) for s, k in C_GEOMETRIES for chunk in (0, 2)]
C_MONITORED += [Case("C", "T0", "l2", "none", "none", "pd", "trace", 2), Case("D", "T2", "l2", "none", "none", "pd", "trace", 2)]
# ... and with a step that freezes image 0
C_FROZEN = [Case("D", "T2", "l2", "none", "batch", "pd", "stop", 2), Case("C", "T0", "l2", "none", "batch", "pd", "stop", 2)]

# d: a real stop at f 8 and f 6 under a last chunk of one copy; plain AMSGrad, and edge weights with Huber
D_OPTIONS = [("l2", "none", "none"), ("huber", "batch", "batch")]
D_CASES = [Case(s, k, l, w, t, "adam", "stop", 2) for s, k in (("C", "T2"), ("D", "T2"), ("D", "T0")) for l, w, t in D_OPTIONS]

# e: the step bound
E_CASES = [Case(s, k, "l2", w, "none", "bound", "off", chunk) for s in ("C", "D", "A") for k in ("T0", "T2")
           for w in ("none", "batch") for chunk in (0, 2)]

PLAIN = sorted({plain(c) for c in A_CASES})
PLAIN += [steps_of(c) for c in PLAIN if c.rule == "adam"]     # the residual of every iterate of the plain run, read back
TABLE = A_CASES + PLAIN + B_CASES + B_STEPS + B_FORWARD + C_CASES + C_MONITORED + C_FROZEN + D_CASES + E_CASES


# ---- option values (host arrays; the device tests upload them) --------------------------------------------------------------------
def data_weights(case, neutral=False, seed=7):
    """float32 [B, N, h, w] or [N, h, w] of the case's weights mode (None for "none").  neutral: all one.  Else values in [0, 1]
    with exact zeros and ones among them; the first two rows of copy 0 -- the identity copy, in frame everywhere -- are 0."""
    if case.weights == "none":
        return None
    p = problem(case)
    shape = (p.b, p.n, p.h, p.w) if case.weights == "batch" else (p.n, p.h, p.w)
    if neutral:
        return np.ones(shape, np.float32)
    rng = np.random.default_rng(seed)
    w = rng.random(shape, dtype=np.float32)
    w[rng.random(shape) < 0.05] = 0.0
    w[rng.random(shape) < 0.05] = 1.0
    w[..., 0, :2, :] = 0.0
    return w


def edge_weights(case, neutral=False, seed=9):
    """(wy, wx) float32 [B, H, W] or [H, W] of the case's tv-weights mode (None for "none"): all one, or values in [0, 1] with a
    tenth exact zeros and a tenth exact ones, as test_gpu_sr_pd._case builds them."""
    if case.tvw == "none":
        return None
    p = problem(case)
    shape = (p.b, p.H, p.W) if case.tvw == "batch" else (p.H, p.W)
    if neutral:
        return np.ones(shape, np.float32), np.ones(shape, np.float32)
    rng = np.random.default_rng(seed)
    planes = []
    for _ in range(2):
        plane = rng.random(shape, dtype=np.float32)
        plane[rng.random(shape) < 0.1] = 0.0
        plane[rng.random(shape) < 0.1] = 1.0
        planes.append(plane)
    return tuple(planes)


def stop_copies(case):
    """The copies of a "stop" case of section d: image 0 all zero (the start is then 0, the loss 0 from the first evaluation and
    the image stalls at once), image 1 the problem's own."""
    y = problem(case).y.copy()
    y[0] = 0.0
    return y


def option_combination(case):
    """Everything but the geometry and the chunking."""
    return case.loss, case.weights, case.tvw, case.rule, case.monitor
