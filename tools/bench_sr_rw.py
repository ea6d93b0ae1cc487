#!/usr/bin/env python3
"""What copy reweighting costs: the SR solve at the README's shape (1 image x 100 copies, 128^2 -> 512^2, 50 iterations,
Adam / AMSGrad), in ONE process, the variants interleaved round by round, timed with device events around a whole solve.

    python tools/bench_sr_rw.py [--rounds 15] [--parent_lib /path/to/libasr_hip.so]

  plain                asr_sr_solve_cfg_f32 of this library: supposed to be the launches it always was
  rw never             asr_sr_solve_rw_f32 with start = the iteration count: the entry point without a reweighting; the result
                       must be the plain solve's bit for bit
  rw every 1 / 10      the same with start = 0 and every = 1 / 10: 50 / 5 reweightings (energy + weights + apply launches and the
                       raw-residual store of the forward launch)
--parent_lib: a library built from the parent commit.  Its asr_sr_solve_cfg_f32 runs in the same rounds on the same tensors,
twice per round ("parent" and "parent again": the gap between those two is the spread a difference has to beat), and its result
must be this library's bit for bit.
Prints the median, the quartiles and the extremes of every variant in us per iteration, the cost of one reweighting
((rw every 1 - rw never) / 50 reweightings) against one iteration, and whether plain - parent lies inside the parent's spread."""
import argparse, ctypes as C, os, sys
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
    sys.exit("bench_sr_rw.py: no GPU visible -- nothing is measured without one")
dev = torch.device("cuda")
b1, b2, eps = np.float32(0.9), np.float32(0.999), np.float32(1e-7)
lam = (1.0, 0.3, 0.7, 0.0)
n, H, h, iters = args.n, 512, 128, args.iters

rng = np.random.RandomState(0)
y = ops.to_device(rng.rand(1, n, h, h).astype(np.float32))
angles = rng.uniform(-0.15, 0.15, (1, n)).astype(np.float32); angles[:, 0] = 0
shifts = rng.uniform(-30, 30, (1, n, 2)).astype(np.float32); shifts[:, 0] = 0
tf = lambda a: ops.to_device(a.reshape(1, n, 8))
rot, irot = tf(T.rotation_transforms(angles.reshape(-1), H, H)), tf(T.rotation_transforms(-angles.reshape(-1), H, H))
tr, itr = tf(T.translation_transforms(shifts.reshape(-1, 2))), tf(T.translation_transforms(-shifts.reshape(-1, 2)))
alphas = ops.to_device(np.array([[T.adam_alpha(np.float32(1e-3), b1, b2, it + 1)] for it in range(iters)], np.float32))
cfg = ops.sr_config(_lib.OPT_ADAM, True, np.float32(1) - b1, np.float32(1) - b2, eps)
dt = _lib.SrDataTerm(_lib.DF_L2, 0.0, None, 0, None, None, 0)

lib = _lib.load()
parent = None
if args.parent_lib:
    parent = C.CDLL(os.path.abspath(args.parent_lib))
    res, argtypes = _lib.SIGNATURES["asr_sr_solve_cfg_f32"]
    parent.asr_sr_solve_cfg_f32.restype, parent.asr_sr_solve_cfg_f32.argtypes = res, argtypes
ws_bytes = lib.asr_sr_solve_workspace_bytes_rw(1, n, H, H, h, h, C.byref(cfg), 0)        # the largest of all
ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.float32, device=dev)
cw = torch.empty((1, n), dtype=torch.float32, device=dev)
x0 = ops.sr_init_target(y, (H, H))
x = torch.empty_like(x0)
m, v, vhat = (torch.empty_like(x0) for _ in range(3))
stream = _lib.stream_ptr()


def head():
    x.copy_(x0)
    for t in (m, v, vhat):
        t.zero_()
    return (x.data_ptr(), y.data_ptr(), rot.data_ptr(), tr.data_ptr(), irot.data_ptr(), itr.data_ptr(), m.data_ptr(), v.data_ptr(),
            vhat.data_ptr(), alphas.data_ptr(), iters, None, ws.data_ptr(), C.c_size_t(ws_bytes), 1, n, H, H, h, h, *lam, C.byref(cfg))


def run(variant):
    a = head()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    if variant in ("parent", "parent again"):
        rc = parent.asr_sr_solve_cfg_f32(*a, stream)
    elif variant == "plain":
        rc = lib.asr_sr_solve_cfg_f32(*a, stream)
    else:
        every, start = {"rw never": (1, iters), "rw every 1": (1, 0), "rw every 10": (10, 0)}[variant]
        rw = _lib.SrReweight(_lib.RW_CAUCHY, 2.0, every, start, cw.data_ptr(), None)
        rc = lib.asr_sr_solve_rw_f32(*a, C.byref(dt), None, 0, C.byref(rw), stream)
    e1.record()
    assert rc == 0, (variant, rc, lib.asr_last_error())
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters, x.clone()


variants = (["parent", "parent again"] if parent else []) + ["plain", "rw never", "rw every 10", "rw every 1"]
times = {k: [] for k in variants}
results = {}
for k in variants:                                  # warm-up, and the results to compare
    results[k] = run(k)[1]
for other in ("parent", "rw never"):
    if other in results:
        assert torch.equal(results[other], results["plain"]), f"{other} differs from the plain solve"
assert not torch.equal(results["rw every 1"], results["plain"])
for r in range(args.rounds):
    for k in (variants if r % 2 == 0 else variants[::-1]):
        times[k].append(run(k)[0])
med = {}
for k in variants:
    t = np.sort(times[k])
    med[k] = float(np.median(t))
    print(f"{k:14s} median {med[k]:8.2f} us/iter   quartiles {np.percentile(t, 25):8.2f} {np.percentile(t, 75):8.2f}   "
          f"min {t[0]:8.2f} max {t[-1]:8.2f}")
per_rw = med["rw every 1"] - med["rw never"]                             # start 0, every 1: one reweighting per iteration
per_rw10 = (med["rw every 10"] - med["rw never"]) * iters / len(range(0, iters, 10))      # start 0: reweightings at 0, 10, ...
print(f"one reweighting: {per_rw:.2f} us (every 1), {per_rw10:.2f} us (every 10) against one iteration of {med['rw never']:.2f} us")
if parent:
    spread = abs(med["parent"] - med["parent again"])
    pairs = np.abs(np.array(times["parent"]) - np.array(times["parent again"]))
    print(f"plain - parent = {med['plain'] - med['parent']:+.2f} us/iter; parent's own spread: medians {spread:.2f}, "
          f"paired runs median {np.median(pairs):.2f} max {pairs.max():.2f} us/iter")
