#!/usr/bin/env python3
"""What the multi-label coupling costs, and whether the uncoupled solve is still the parent's: the primal-dual SR solve of
K = 5 classes of one image (5 planes x 100 copies, 128^2 -> 512^2), in ONE process, the variants interleaved round by round,
timed with device events around a whole call.

    python tools/bench_sr_ml.py [--rounds 9] [--parent_lib /path/to/libasr_hip.so]

  uncoupled            asr_sr_solve_cfg_f32 with ASR_OPT_PRIMAL_DUAL, --iters iterations: what the label-map path runs without
                       couple=True; supposed to be the launches it always was
  ml, group 0          asr_sr_solve_ml_f32 with group = 0: the *_dt form of the same solve, no projection
  coupled              asr_sr_solve_ml_f32 with group = K: one projection launch more per iteration
  projection           asr_simplex_project_f32 alone on the [K, 512, 512] result of the uncoupled solve (a realistic mix of pixels
                       below and above a sum of 1), --proj_reps launches on as many buffers per timing
  copy                 a device copy of the same [K, 512, 512] floats, as often: K*H*W floats read and as many written, the
                       traffic of the stand-alone projection (inside the solve it writes the bordered copy too, K*H*W more)
--parent_lib: a library built from the parent commit.  Its asr_sr_solve_cfg_f32 runs in the same rounds on the same tensors,
twice per round ("parent" and "parent again": the gap between those two is the spread a difference has to beat), and its result
must be this library's bit for bit.
Prints the median, the quartiles and the extremes of every variant in us per iteration (projection and copy: per launch), the
ratios coupled / uncoupled and projection / copy, and the condition of DESIGN 7: |uncoupled - parent| inside the spread."""
import argparse, ctypes as C, hashlib, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from asr_amd import _lib, ops, transforms as T
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--parent_lib", default=None)
ap.add_argument("--classes", type=int, default=5)
ap.add_argument("--n", type=int, default=100)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--proj_reps", type=int, default=20)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_sr_ml.py: no GPU visible -- nothing is measured without one")
dev = torch.device("cuda")
lam = (1.0, 0.3, 0.7, 0.0)
K, n, H, h, iters = args.classes, args.n, 512, 128, args.iters

# K classes of one image: disjoint noisy low-resolution class maps under ONE set of transforms
rng = np.random.RandomState(0)
owner = rng.randint(0, K + 1, (n, h // 8, h // 8)).repeat(8, axis=1).repeat(8, axis=2)          # K = background
y = np.stack([(owner == k).astype(np.float32) for k in range(K)])
y = np.clip(y + rng.normal(0, 0.15, y.shape).astype(np.float32), 0, 1).astype(np.float32)
angles = rng.uniform(-0.15, 0.15, n).astype(np.float32); angles[0] = 0
shifts = rng.uniform(-30, 30, (n, 2)).astype(np.float32); shifts[0] = 0
tf = lambda a: ops.to_device(np.repeat(a.reshape(1, n, 8), K, axis=0))
rot, irot = tf(T.rotation_transforms(angles, H, H)), tf(T.rotation_transforms(-angles, H, H))
tr, itr = tf(T.translation_transforms(shifts)), tf(T.translation_transforms(-shifts))
yd = ops.to_device(y)
cfg = ops.sr_config(_lib.OPT_PRIMAL_DUAL, c0=ops.PD_DUAL_RATIO)
alphas = ops.pd_steps(ops.sr_data_bound(rot, tr, irot, itr, (H, H), (h, h), lam[0]), lam[2], iters)
dt = _lib.SrDataTerm(_lib.DF_L2, 0.1, None, 0, None, None, 0)

lib = _lib.load()
parent = None
if args.parent_lib:
    parent = C.CDLL(os.path.abspath(args.parent_lib))
    res, argtypes = _lib.SIGNATURES["asr_sr_solve_cfg_f32"]
    parent.asr_sr_solve_cfg_f32.restype, parent.asr_sr_solve_cfg_f32.argtypes = res, argtypes
ws_bytes = lib.asr_sr_solve_workspace_bytes_ml(K, n, H, H, h, h, C.byref(cfg), 0)              # the larger of the two forms
ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.float32, device=dev)


def solve(library, group=None):
    x = ops.sr_init_target(yd, (H, H))
    m, v, vh = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x)
    head = (ops.ptr(x), ops.ptr(yd), ops.ptr(rot), ops.ptr(tr), ops.ptr(irot), ops.ptr(itr), ops.ptr(m), ops.ptr(v), ops.ptr(vh),
            ops.ptr(alphas), iters, None, ops.ptr(ws), C.c_size_t(ws_bytes), K, n, H, H, h, h, lam[0], lam[1], lam[2], lam[3],
            C.byref(cfg))
    if group is None:
        rc = library.asr_sr_solve_cfg_f32(*head, ops.stream_ptr())
    else:
        rc = library.asr_sr_solve_ml_f32(*head, C.byref(dt), None, group, ops.stream_ptr())
    assert rc == 0, (rc, library.asr_last_error())
    return x


realistic = solve(lib).clone()
bufs = [torch.empty_like(realistic) for _ in range(args.proj_reps)]
dsts = [torch.empty_like(realistic) for _ in range(args.proj_reps)]


def project_all():
    for buf in bufs:
        ops.simplex_project(buf, K)
    return bufs[0]


def copy_all():
    for buf, dst in zip(bufs, dsts):
        dst.copy_(buf)
    return dsts[0]


variants = [("uncoupled", iters, lambda: solve(lib)), ("ml, group 0", iters, lambda: solve(lib, 0)),
            ("coupled", iters, lambda: solve(lib, K)), ("projection", args.proj_reps, project_all), ("copy", args.proj_reps, copy_all)]
if parent is not None:
    variants = [("parent", iters, lambda: solve(parent))] + variants + [("parent again", iters, lambda: solve(parent))]
times = {v[0]: [] for v in variants}
sums = {}
for r in range(args.rounds + 2):                 # two warm-up rounds
    order = variants if r % 2 == 0 else variants[::-1]
    for label, _, fn in order:
        if label in ("projection", "copy"):
            for buf in bufs:
                buf.copy_(realistic)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record(); torch.cuda.synchronize()
        if r >= 2:
            times[label].append(e0.elapsed_time(e1))
        sums[label] = hashlib.sha1(out.cpu().numpy().tobytes()).hexdigest()[:16]
over = float((realistic.clamp(min=0).sum(0) > 1).float().mean())
print(f"K = {K}, N = {n}, {h}^2 -> {H}^2, {iters} iterations, {args.rounds} interleaved rounds; us per iteration (call time / "
      f"iterations; projection and copy: / {args.proj_reps} launches); {100 * over:.1f} % of the projected pixels lie above a sum of 1")
med = {}
for label, per, _ in variants:
    t = 1000.0 * np.asarray(times[label]) / per
    q = np.percentile(t, [0, 25, 50, 75, 100])
    med[label] = q[2]
    print(f"  {label:16s} median {q[2]:9.2f}  quartiles {q[1]:9.2f} .. {q[3]:9.2f}  range {q[0]:9.2f} .. {q[4]:9.2f}  sha1 {sums[label]}")
assert sums["uncoupled"] == sums["ml, group 0"], "group 0 is not the uncoupled solve"
traffic = 2.0 * K * H * H * 4
print(f"  coupled / uncoupled per iteration: {med['coupled'] / med['uncoupled']:.4f}  (coupled - uncoupled: "
      f"{med['coupled'] - med['uncoupled']:+.2f} us; ml group 0 - uncoupled: {med['ml, group 0'] - med['uncoupled']:+.2f} us)")
print(f"  projection / copy per launch: {med['projection'] / med['copy']:.2f}  ({traffic / med['projection'] / 1e3:.0f} GB/s against "
      f"{traffic / med['copy'] / 1e3:.0f} GB/s over {traffic / 1e6:.1f} MB)")
if parent is not None:
    assert sums["parent"] == sums["uncoupled"] == sums["parent again"], "the uncoupled solve differs from the parent's"
    spread = abs(med["parent again"] - med["parent"])
    gap = med["uncoupled"] - med["parent"]
    print(f"  uncoupled - parent: {gap:+.2f} us; parent again - parent (spread): {med['parent again'] - med['parent']:+.2f} us")
    print(f"  condition (|uncoupled - parent| inside the spread): {'met' if abs(gap) <= spread else 'NOT met'}")
