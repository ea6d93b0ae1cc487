#!/usr/bin/env python3
"""What the data term costs: the SR solve at the README's shape (1 image x 100 copies, 128^2 -> 512^2, 50 iterations, Adam /
AMSGrad) with the L2, Huber, L1 and weighted data terms, in ONE process, the variants interleaved round by round, timed with
device events around a whole solve; and the confidence kernel once on [100, 128, 128, 21] logits.

    python tools/bench_sr_dt.py [--rounds 15] [--parent_lib /path/to/libasr_hip.so]

Every variant is a direct call with the workspace allocated once, so the host work is the same for all of them.  "L2" is
asr_sr_solve_cfg_f32, "L2 through dt" the new entry point with {ASR_DF_L2, no weights}: the same arithmetic through the forward
kernel's data-term instantiation, and it must give the same bits.  The expectation for the weighted forms is one more 4-byte load
per residual element and nothing else.
--parent_lib: a library built from the parent commit.  Its asr_sr_solve_cfg_f32 then runs in the same rounds on the same tensors,
twice per round ("parent L2" and "parent L2 again": the gap between those two is the spread a difference has to beat), and its
result must be this library's bit for bit.
Prints the median, the quartiles and the extremes of every variant in us per iteration."""
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
    sys.exit("bench_sr_dt.py: no GPU visible -- nothing is measured without one")
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
wts = ops.to_device(rng.rand(n, h, h).astype(np.float32))
ones = torch.ones((n, h, h), device=dev)

lib = _lib.load()
parent = None
if args.parent_lib:
    parent = C.CDLL(os.path.abspath(args.parent_lib))
    res, argtypes = _lib.SIGNATURES["asr_sr_solve_cfg_f32"]
    parent.asr_sr_solve_cfg_f32.restype, parent.asr_sr_solve_cfg_f32.argtypes = res, argtypes
ws_bytes = lib.asr_sr_solve_workspace_bytes_dt(1, n, H, H, h, h, C.byref(cfg))        # the larger of the two
ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.float32, device=dev)


def solve(library, dt=None):
    x = ops.sr_init_target(yd, (H, H))
    m, v, vh = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x)
    head = (ops.ptr(x), ops.ptr(yd), ops.ptr(rot), ops.ptr(tr), ops.ptr(irot), ops.ptr(itr), ops.ptr(m), ops.ptr(v), ops.ptr(vh),
            ops.ptr(alphas), iters, None, ops.ptr(ws), C.c_size_t(ws_bytes), 1, n, H, H, h, h, lam[0], lam[1], lam[2], lam[3],
            C.byref(cfg))
    if dt is None:
        rc = library.asr_sr_solve_cfg_f32(*head, ops.stream_ptr())
    else:
        rc = library.asr_sr_solve_dt_f32(*head, C.byref(dt), ops.stream_ptr())
    assert rc == 0, rc
    return x


def term(loss, delta=0.0, weights=None):
    return _lib.SrDataTerm(loss, delta, ops.ptr(weights, allow_none=True), 1, None, None, 0)


variants = [("L2", lambda: solve(lib)), ("L2 through dt", lambda: solve(lib, term(_lib.DF_L2))),
            ("Huber (delta 0.1)", lambda: solve(lib, term(_lib.DF_HUBER, 0.1))), ("L1", lambda: solve(lib, term(_lib.DF_L1))),
            ("L2 weighted", lambda: solve(lib, term(_lib.DF_L2, 0.0, wts))),
            ("Huber weighted", lambda: solve(lib, term(_lib.DF_HUBER, 0.1, wts))),
            ("L2 weighted (all ones)", lambda: solve(lib, term(_lib.DF_L2, 0.0, ones)))]
if parent is not None:
    variants = [("parent L2", lambda: solve(parent))] + variants + [("parent L2 again", lambda: solve(parent))]
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
assert sums["L2 through dt"] == sums["L2"] == sums["L2 weighted (all ones)"], "L2 through the data-term entry point is not the L2 solve"
med = lambda k: float(np.median(times[k])) * 1000.0 / iters
print(f"  L2 through dt - L2: {med('L2 through dt') - med('L2'):+.2f} us; Huber - L2: {med('Huber (delta 0.1)') - med('L2'):+.2f} us; "
      f"L2 weighted - L2: {med('L2 weighted') - med('L2'):+.2f} us; Huber weighted - L2: {med('Huber weighted') - med('L2'):+.2f} us")
if parent is not None:
    assert sums["parent L2"] == sums["L2"] == sums["parent L2 again"], "the L2 solve differs from the parent's"
    print(f"  L2 - parent: {med('L2') - med('parent L2'):+.2f} us; parent again - parent (spread): "
          f"{med('parent L2 again') - med('parent L2'):+.2f} us")

# the confidence kernel on one image's logits, [100, 128, 128, 21]: 100 launches between two events
logits = torch.randn((n, h, h, 21), device=dev)
out = torch.empty((n, h, h), device=dev)
for kind in ("maxprob", "margin"):
    for _ in range(10):
        ops.opm_confidence(logits, kind, out=out)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(100):
        ops.opm_confidence(logits, kind, out=out)
    e1.record(); torch.cuda.synchronize()
    us = 1000.0 * e0.elapsed_time(e1) / 100
    moved = logits.numel() * 4 + out.numel() * 4
    print(f"  opm_confidence({kind}) on {tuple(logits.shape)}: {us:.2f} us per call, {moved / us / 1e3:.1f} GB/s of its {moved / 1e6:.1f} MB")
