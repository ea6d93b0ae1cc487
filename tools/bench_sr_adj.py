#!/usr/bin/env python3
"""What an iteration under the exact adjoint costs next to the registered one, for AMSGrad and for the primal-dual rule, and whether
the registered solve is still the parent's: the SR solve at the README's shape (1 image x 100 copies, 128^2 -> 512^2), in ONE
process, the variants interleaved round by round, timed with device events around a whole call.

    python tools/bench_sr_adj.py [--rounds 15] [--parent_lib /path/to/libasr_hip.so]

  amsgrad registered / exact       asr_sr_solve_adj_f32 with {Adam, amsgrad} under ASR_ADJ_REGISTERED / ASR_ADJ_EXACT: the same
  primal-dual registered / exact   entry point and launches, only the gather kernel differs (the exact one does nine maps per copy
                                   where the registered one does one)
  cfg                              asr_sr_solve_cfg_f32 with {Adam, amsgrad}: the call the hot path makes, supposed to be untouched
--parent_lib: a library built from the parent commit.  Its asr_sr_solve_cfg_f32 (AMSGrad) runs in the same rounds on the same
tensors, twice per round ("parent" and "parent again": the gap between those two is the spread a difference has to beat), and
its result must be this library's bit for bit.
Prints the median, the quartiles and the extremes of every variant in us per iteration, the ratios exact / registered, and
|cfg - parent| against the spread."""
import argparse, ctypes as C, hashlib, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from asr_amd import _lib, ops, transforms as T
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=15)
ap.add_argument("--parent_lib", default=None)
ap.add_argument("--n", type=int, default=100)
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--angle_max", type=float, default=0.15)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_sr_adj.py: no GPU visible -- nothing is measured without one")
dev = torch.device("cuda")
b1, b2, eps = np.float32(0.9), np.float32(0.999), np.float32(1e-7)
lam = (1.0, 0.3, 0.7, 0.0)
n, H, h, iters = args.n, 512, 128, args.iters

rng = np.random.RandomState(0)
y = rng.rand(1, n, h, h).astype(np.float32)
angles = rng.uniform(-args.angle_max, args.angle_max, (1, n)).astype(np.float32); angles[:, 0] = 0
shifts = rng.uniform(-30, 30, (1, n, 2)).astype(np.float32); shifts[:, 0] = 0
tf = lambda a: ops.to_device(a.reshape(1, n, 8))
rot, irot = tf(T.rotation_transforms(angles.reshape(-1), H, H)), tf(T.rotation_transforms(-angles.reshape(-1), H, H))
tr, itr = tf(T.translation_transforms(shifts.reshape(-1, 2))), tf(T.translation_transforms(-shifts.reshape(-1, 2)))
yd = ops.to_device(y)
adam_alphas = ops.to_device(np.array([T.adam_alpha(np.float32(1e-3), b1, b2, it + 1) for it in range(iters)], np.float32)[:, None].copy())
adam_cfg = ops.sr_config(_lib.OPT_ADAM, True, np.float32(1) - b1, np.float32(1) - b2, eps)
pd_cfg = ops.sr_config(_lib.OPT_PRIMAL_DUAL, c0=ops.PD_DUAL_RATIO)
pd_alphas = {a: ops.pd_steps(ops.sr_data_bound(rot, tr, irot, itr, (H, H), (h, h), lam[0], iters=6, adjoint=a), lam[2], iters)
             for a in ("registered", "exact")}
assert int(ops.sr_adjoint_flags(rot, tr, irot).cpu()[0]) == 1, "the exact form does not apply to the benchmark's transforms"

lib = _lib.load()
parent = None
if args.parent_lib:
    parent = C.CDLL(os.path.abspath(args.parent_lib))
    res, argtypes = _lib.SIGNATURES["asr_sr_solve_cfg_f32"]
    parent.asr_sr_solve_cfg_f32.restype, parent.asr_sr_solve_cfg_f32.argtypes = res, argtypes
ws_bytes = lib.asr_sr_solve_workspace_bytes_dt(1, n, H, H, h, h, C.byref(pd_cfg))        # the largest of those used here
ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.float32, device=dev)
l2 = _lib.SrDataTerm(_lib.DF_L2, 0.0, None, 0, None, None, 0)


def fresh():
    x = ops.sr_init_target(yd, (H, H))
    return x, torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x)


def solve_cfg(library):
    x, m, v, vh = fresh()
    rc = library.asr_sr_solve_cfg_f32(ops.ptr(x), ops.ptr(yd), ops.ptr(rot), ops.ptr(tr), ops.ptr(irot), ops.ptr(itr), ops.ptr(m),
                                      ops.ptr(v), ops.ptr(vh), ops.ptr(adam_alphas), iters, None, ops.ptr(ws), C.c_size_t(ws_bytes), 1,
                                      n, H, H, h, h, lam[0], lam[1], lam[2], lam[3], C.byref(adam_cfg), ops.stream_ptr())
    assert rc == 0, (rc, library.asr_last_error())
    return x


def solve_adj(cfg, alphas, adjoint):
    x, m, v, vh = fresh()
    rc = lib.asr_sr_solve_adj_f32(ops.ptr(x), ops.ptr(yd), ops.ptr(rot), ops.ptr(tr), ops.ptr(irot), ops.ptr(itr), ops.ptr(m), ops.ptr(v),
                                  ops.ptr(vh), ops.ptr(alphas), iters, None, ops.ptr(ws), C.c_size_t(ws_bytes), 1, n, H, H, h, h, lam[0],
                                  lam[1], lam[2], lam[3], C.byref(cfg), C.byref(l2), None, 0, None, _lib.ADJOINTS[adjoint],
                                  ops.stream_ptr())
    assert rc == 0, (rc, lib.asr_last_error())
    return x


variants = [("cfg", lambda: solve_cfg(lib))]
for a in ("registered", "exact"):
    variants.append((f"amsgrad {a}", lambda a=a: solve_adj(adam_cfg, adam_alphas, a)))
    variants.append((f"primal-dual {a}", lambda a=a: solve_adj(pd_cfg, pd_alphas[a], a)))
if parent is not None:
    variants = [("parent", lambda: solve_cfg(parent))] + variants + [("parent again", lambda: solve_cfg(parent))]
times = {v[0]: [] for v in variants}
sums = {}
for r in range(args.rounds + 2):                 # two warm-up rounds
    order = variants if r % 2 == 0 else variants[::-1]
    for label, fn in order:
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record(); torch.cuda.synchronize()
        if r >= 2:
            times[label].append(e0.elapsed_time(e1))
        sums[label] = hashlib.sha1(out.cpu().numpy().tobytes()).hexdigest()[:16]
print(f"N = {n}, {h}^2 -> {H}^2, |angle| <= {args.angle_max}, {iters} iterations, {args.rounds} interleaved rounds; us per iteration "
      f"(call time / iterations)")
med = {}
for label, _ in variants:
    t = 1000.0 * np.asarray(times[label]) / iters
    q = np.percentile(t, [0, 25, 50, 75, 100])
    med[label] = q[2]
    print(f"  {label:24s} median {q[2]:7.2f}  quartiles {q[1]:7.2f} .. {q[3]:7.2f}  range {q[0]:7.2f} .. {q[4]:7.2f}  sha1 {sums[label]}")
for rule in ("amsgrad", "primal-dual"):
    print(f"  {rule}: exact / registered per iteration: {med[rule + ' exact'] / med[rule + ' registered']:.3f} "
          f"(+{med[rule + ' exact'] - med[rule + ' registered']:.2f} us)")
assert sums["cfg"] == sums["amsgrad registered"], "ASR_ADJ_REGISTERED differs from asr_sr_solve_cfg_f32"
if parent is not None:
    assert sums["parent"] == sums["cfg"] == sums["parent again"], "the registered AMSGrad solve differs from the parent's"
    print(f"  cfg - parent: {med['cfg'] - med['parent']:+.2f} us; parent again - parent (spread): {med['parent again'] - med['parent']:+.2f} us")
