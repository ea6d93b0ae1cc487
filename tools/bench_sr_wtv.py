#!/usr/bin/env python3
"""What the edge-weighted TV prior costs: the SR solve at the README's shape (1 image x 100 copies, 128^2 -> 512^2, 50 iterations,
Adam / AMSGrad) with the TV prior and with the weighted one, in ONE process, the variants interleaved round by round, timed with
device events around a whole solve; and the weights kernel once at 512^2.

    python tools/bench_sr_wtv.py [--rounds 15] [--parent_lib /path/to/libasr_hip.so]

--parent_lib: a library built from the parent commit.  Its asr_sr_solve_cfg_f32 then runs in the same rounds, on the same
tensors and through the same direct call as this library's ("TV"), twice per round ("parent TV" and "parent TV again": the gap
between those two is the spread a difference has to beat), and its result must be this library's bit for bit.  The weighted
solves and "TV through ops" go through ops.sr_solve, which also allocates the workspace: compare those with each other.
Prints the median, the quartiles and the extremes of every variant in us per iteration; a checksum says that unit weights
are the TV solve."""
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
    sys.exit("bench_sr_wtv.py: no GPU visible -- nothing is measured without one")
dev = torch.device("cuda")
b1, b2, eps = np.float32(0.9), np.float32(0.999), np.float32(1e-7)
lam = (1.0, 0.3, 0.7, 0.0)
n, H, h, iters = args.n, 512, 128, args.iters

rng = np.random.RandomState(0)
yd = ops.to_device(rng.rand(1, n, h, h).astype(np.float32))
angles = rng.uniform(-0.15, 0.15, (1, n)).astype(np.float32); angles[0, 0] = 0
shifts = rng.uniform(-30, 30, (1, n, 2)).astype(np.float32); shifts[0, 0] = 0
tf = lambda a: ops.to_device(a.reshape(1, n, 8))
rot, irot = tf(T.rotation_transforms(angles.reshape(-1), H, H)), tf(T.rotation_transforms(-angles.reshape(-1), H, H))
tr, itr = tf(T.translation_transforms(shifts.reshape(-1, 2))), tf(T.translation_transforms(-shifts.reshape(-1, 2)))
alphas = ops.to_device(np.array([[T.adam_alpha(np.float32(1e-3), b1, b2, it + 1)] for it in range(iters)], np.float32))
cfg = ops.sr_config(_lib.OPT_ADAM, True, np.float32(1) - b1, np.float32(1) - b2, eps)
guide = ops.to_device(rng.rand(H, H, 3).astype(np.float32))
weights = ops.tv_edge_weights(guide, 100.0)
ones = (torch.ones((H, H), device=dev), torch.ones((H, H), device=dev))

parent = None
if args.parent_lib:
    parent = C.CDLL(os.path.abspath(args.parent_lib))
    res, argtypes = _lib.SIGNATURES["asr_sr_solve_cfg_f32"]
    parent.asr_sr_solve_cfg_f32.restype, parent.asr_sr_solve_cfg_f32.argtypes = res, argtypes
ws_bytes = _lib.load().asr_sr_solve_workspace_bytes_cfg(1, n, H, H, h, h, C.byref(cfg))
ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.float32, device=dev)


def solve_direct(lib):
    x = ops.sr_init_target(yd, (H, H))
    m, v, vh = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x)
    rc = lib.asr_sr_solve_cfg_f32(ops.ptr(x), ops.ptr(yd), ops.ptr(rot), ops.ptr(tr), ops.ptr(irot), ops.ptr(itr), ops.ptr(m),
                                  ops.ptr(v), ops.ptr(vh), ops.ptr(alphas), iters, None, ops.ptr(ws), C.c_size_t(ws_bytes), 1, n,
                                  H, H, h, h, lam[0], lam[1], lam[2], lam[3], C.byref(cfg), ops.stream_ptr())
    assert rc == 0, rc
    return x


def solve(tv_weights=None):
    return ops.sr_solve(ops.sr_init_target(yd, (H, H)), yd, rot, tr, irot, itr, alphas, lam, want_loss=False, cfg=cfg,
                        tv_weights=tv_weights)[0]


variants = [("TV", lambda: solve_direct(_lib.load())), ("TV through ops", solve), ("weighted (beta = 100)", lambda: solve(weights)),
            ("weighted (all ones)", lambda: solve(ones))]
if parent is not None:
    variants = [("parent TV", lambda: solve_direct(parent))] + variants + [("parent TV again", lambda: solve_direct(parent))]
times = {v[0]: [] for v in variants}
sums = {}
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
print(f"N = {n}, {h}^2 -> {H}^2, {iters} iterations, {args.rounds} interleaved rounds; us per iteration (solve time / iterations)")
for label, _ in variants:
    t = 1000.0 * np.asarray(times[label]) / iters
    q = np.percentile(t, [0, 25, 50, 75, 100])
    print(f"  {label:24s} median {q[2]:7.2f}  quartiles {q[1]:7.2f} .. {q[3]:7.2f}  range {q[0]:7.2f} .. {q[4]:7.2f}  sha1(x) {sums[label]}")
assert sums["weighted (all ones)"] == sums["TV"] == sums["TV through ops"], "unit weights are not the TV solve"
if parent is not None:
    assert sums["parent TV"] == sums["TV"] == sums["parent TV again"], "the TV solve differs from the parent's"
    med = lambda k: float(np.median(times[k])) * 1000.0 / iters
    print(f"  TV - parent: {med('TV') - med('parent TV'):+.2f} us; parent again - parent (spread): "
          f"{med('parent TV again') - med('parent TV'):+.2f} us; weighted - TV, both through ops: "
          f"{med('weighted (beta = 100)') - med('TV through ops'):+.2f} us")

# the weights kernel, 512^2, one image: 200 launches between two events
for _ in range(20):
    ops.tv_edge_weights(guide, 100.0)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(200):
    ops.tv_edge_weights(guide, 100.0)
e1.record(); torch.cuda.synchronize()
us = 1000.0 * e0.elapsed_time(e1) / 200
bytes_moved = H * H * (3 + 2) * 4
print(f"  tv_edge_weights at {H}^2: {us:.2f} us per call (launch and two allocations included), {bytes_moved / us / 1e3:.1f} GB/s of "
      f"its {bytes_moved / 1e6:.2f} MB")
