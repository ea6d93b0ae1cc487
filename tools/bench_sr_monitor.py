#!/usr/bin/env python3
"""What the convergence monitor costs and what a freeze saves: the SR solve at the README's shape (1 image x 100 copies,
128^2 -> 512^2, 50 iterations, Adam / AMSGrad), in ONE process, the variants interleaved round by round, timed with device
events around a whole solve.

    python tools/bench_sr_monitor.py [--rounds 15] [--parent_lib /path/to/libasr_hip.so]

  unmonitored          asr_sr_solve_cfg_f32 of this library: supposed to be the launches it always was
  every = 1, 5, 10     asr_sr_solve_mon_f32 with patience = 0 (trace only, a history buffer): the cost of monitoring itself;
                       the result must be the unmonitored solve's bit for bit
  batch of 4           two images with all-zero copies and two ordinary ones, every = 1: "unfrozen" with patience = 0, "half
                       frozen" with patience = 10 and min_iter = 10 -- the zero images' loss is 0 from the start, so the rule
                       freezes exactly them at iteration 10 (iters_done is checked) and they sit out the other 40 iterations
--parent_lib: a library built from the parent commit.  Its asr_sr_solve_cfg_f32 runs in the same rounds on the same tensors,
twice per round ("parent" and "parent again": the gap between those two is the spread a difference has to beat), and its result
must be this library's bit for bit.
Prints the median, the quartiles and the extremes of every variant in us per iteration, and the two conditions of DESIGN 7:
unmonitored - parent inside the spread; the half-frozen batch faster than the unfrozen one by more than the spread."""
import argparse, ctypes as C, hashlib, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from asr_amd import _lib, ops, transforms as T
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=15)
ap.add_argument("--parent_lib", default=None)
ap.add_argument("--n", type=int, default=100)
ap.add_argument("--iters", type=int, default=50)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_sr_monitor.py: no GPU visible -- nothing is measured without one")
dev = torch.device("cuda")
b1, b2, eps = np.float32(0.9), np.float32(0.999), np.float32(1e-7)
lam = (1.0, 0.3, 0.7, 0.0)
n, H, h, iters, B4 = args.n, 512, 128, args.iters, 4

rng = np.random.RandomState(0)
y4 = rng.rand(B4, n, h, h).astype(np.float32)
y4[:2] = 0.0                                                   # images 0 and 1 of the batch of 4: loss 0 from the start
angles = rng.uniform(-0.15, 0.15, (B4, n)).astype(np.float32); angles[:, 0] = 0
shifts = rng.uniform(-30, 30, (B4, n, 2)).astype(np.float32); shifts[:, 0] = 0
tf = lambda a: ops.to_device(a.reshape(B4, n, 8))
rot4, irot4 = tf(T.rotation_transforms(angles.reshape(-1), H, H)), tf(T.rotation_transforms(-angles.reshape(-1), H, H))
tr4, itr4 = tf(T.translation_transforms(shifts.reshape(-1, 2))), tf(T.translation_transforms(-shifts.reshape(-1, 2)))
yd4 = ops.to_device(y4)
col = np.array([T.adam_alpha(np.float32(1e-3), b1, b2, it + 1) for it in range(iters)], np.float32)
alphas = {1: ops.to_device(col[:, None].copy()), B4: ops.to_device(np.repeat(col[:, None], B4, axis=1))}
# the single image is image 3 of the batch: an ordinary problem
one = lambda t: t[3:4].contiguous()
prob = {1: tuple(one(t) for t in (yd4, rot4, tr4, irot4, itr4)), B4: (yd4, rot4, tr4, irot4, itr4)}
cfg = ops.sr_config(_lib.OPT_ADAM, True, np.float32(1) - b1, np.float32(1) - b2, eps)

lib = _lib.load()
parent = None
if args.parent_lib:
    parent = C.CDLL(os.path.abspath(args.parent_lib))
    res, argtypes = _lib.SIGNATURES["asr_sr_solve_cfg_f32"]
    parent.asr_sr_solve_cfg_f32.restype, parent.asr_sr_solve_cfg_f32.argtypes = res, argtypes
ws_bytes = lib.asr_sr_solve_workspace_bytes_mon(B4, n, H, H, h, h, C.byref(cfg))        # the largest of all
ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.float32, device=dev)
history = torch.empty((iters, B4, 4), dtype=torch.float64, device=dev)
iters_done = torch.empty((B4,), dtype=torch.int32, device=dev)
l2_term = _lib.SrDataTerm(_lib.DF_L2, 0.0, None, 0, None, None, 0)


def solve(library, b=1, mon=None):
    yd, rot, tr, irot, itr = prob[b]
    x = ops.sr_init_target(yd, (H, H))
    m, v, vh = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x)
    head = (ops.ptr(x), ops.ptr(yd), ops.ptr(rot), ops.ptr(tr), ops.ptr(irot), ops.ptr(itr), ops.ptr(m), ops.ptr(v), ops.ptr(vh),
            ops.ptr(alphas[b]), iters, None, ops.ptr(ws), C.c_size_t(ws_bytes), b, n, H, H, h, h, lam[0], lam[1], lam[2], lam[3],
            C.byref(cfg))
    if mon is None:
        rc = library.asr_sr_solve_cfg_f32(*head, ops.stream_ptr())
    else:
        every, patience, min_iter = mon
        ms = _lib.SrMonitor(every, 0.0, patience, min_iter, history.data_ptr(), iters_done.data_ptr())
        rc = library.asr_sr_solve_mon_f32(*head, C.byref(l2_term), C.byref(ms), ops.stream_ptr())
    assert rc == 0, (rc, library.asr_last_error())
    return x


variants = [("unmonitored", lambda: solve(lib)), ("every = 1", lambda: solve(lib, mon=(1, 0, 0))),
            ("every = 5", lambda: solve(lib, mon=(5, 0, 0))), ("every = 10", lambda: solve(lib, mon=(10, 0, 0))),
            ("batch of 4, unfrozen", lambda: solve(lib, B4, mon=(1, 0, 0))),
            ("batch of 4, half frozen", lambda: solve(lib, B4, mon=(1, 10, 10)))]
if parent is not None:
    variants = [("parent", lambda: solve(parent))] + variants + [("parent again", lambda: solve(parent))]
times = {v[0]: [] for v in variants}
sums, done = {}, {}
for r in range(args.rounds + 2):                 # two warm-up rounds
    order = variants if r % 2 == 0 else variants[::-1]
    for label, fn in order:
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        x = fn()
        e1.record(); torch.cuda.synchronize()
        if r >= 2:
            times[label].append(e0.elapsed_time(e1))
        sums[label] = hashlib.sha1(x.cpu().numpy().tobytes()).hexdigest()[:16]
        if label.startswith("batch"):
            done[label] = iters_done.cpu().numpy().tolist()
print(f"N = {n}, {h}^2 -> {H}^2, {iters} iterations, {args.rounds} interleaved rounds; us per iteration (solve time / iterations)")
for label, _ in variants:
    t = 1000.0 * np.asarray(times[label]) / iters
    q = np.percentile(t, [0, 25, 50, 75, 100])
    print(f"  {label:24s} median {q[2]:7.2f}  quartiles {q[1]:7.2f} .. {q[3]:7.2f}  range {q[0]:7.2f} .. {q[4]:7.2f}  sha1(x) {sums[label]}")
for k in (1, 5, 10):
    assert sums[f"every = {k}"] == sums["unmonitored"], f"the traced solve (every = {k}) is not the unmonitored solve"
print(f"  iterations of the batch of 4: unfrozen {done['batch of 4, unfrozen']}, half frozen {done['batch of 4, half frozen']}")
assert done["batch of 4, unfrozen"] == [iters] * B4 and done["batch of 4, half frozen"] == [10, 10, iters, iters]
med = lambda k: float(np.median(times[k])) * 1000.0 / iters
print("  monitoring: " + "; ".join(f"every = {k} - unmonitored: {med(f'every = {k}') - med('unmonitored'):+.2f} us" for k in (1, 5, 10)))
saved = med("batch of 4, unfrozen") - med("batch of 4, half frozen")
print(f"  freeze: unfrozen - half frozen: {saved:+.2f} us per iteration of the batch")
if parent is not None:
    assert sums["parent"] == sums["unmonitored"] == sums["parent again"], "the unmonitored solve differs from the parent's"
    spread = abs(med("parent again") - med("parent"))
    gap = med("unmonitored") - med("parent")
    print(f"  unmonitored - parent: {gap:+.2f} us; parent again - parent (spread): {med('parent again') - med('parent'):+.2f} us")
    print(f"  condition 1 (|unmonitored - parent| inside the spread): {'met' if abs(gap) <= spread else 'NOT met'}")
    print(f"  condition 2 (half frozen faster than unfrozen by more than the spread): {'met' if saved > spread else 'NOT met'}")
