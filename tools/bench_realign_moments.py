#!/usr/bin/env python3
"""The variance of the realigned copies: one asr_realign_moments_f32 call (variance + valid count under a shared ones plane,
what HotPath.run_image_labels' coverages launches) against what the library offered before it for the same map, on the MI355X
("Uncertainty over the copies and the risk-coverage curve").

    python tools/bench_realign_moments.py --impl fused|planes|mean_once      # one implementation, one process
    python tools/bench_realign_moments.py [--rounds 3]                        # the comparison

The shape is the label-map workload's: K' = 3 solved classes, N = 100 copies, 128 x 128 -> 512 x 512.  The inputs are copied
from the host (no set-up kernel runs on the device):
--impl fused:     one asr_realign_moments_f32 call over the [3, 100, 128, 128] stacks, out_var and out_nv;
--impl planes:    the stacks viewed as 300 single-copy stacks through asr_realign_max_f32 (one launch that writes the 300
                  realigned planes, 315 MB), then torch.var(unbiased=False) over the copies -- every copy counted, zero fill
                  included, so not the same rule where a copy left the frame: the nearest the parent commit offers;
--impl mean_once: a single asr_realign_mean_f32 call over the same stacks -- one walk over the copies; the fused call makes two.
An --impl run warms up, then times WINDOWS windows of CALLS calls each with a host clock around a device synchronise, and
prints one JSON line with the microseconds per call of every window.  The comparison starts each implementation in a process of
its own, ROUNDS times, alternating them, and prints one JSON line: the median per implementation, the run-to-run spread
(largest - smallest window median of one implementation over its rounds), fused / planes, and whether the difference exceeds
that spread.  It states what it measured; it gates nothing.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

CALLS, WINDOWS, WARMUP = 50, 5, 10
K, N, LR, HR = 3, 100, 128, 512
IMPLS = ("fused", "planes", "mean_once")


def run(impl):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch
    from asr_amd import ops, transforms as T

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    y = torch.as_tensor((rng.random((K, N, LR, LR), dtype=np.float32) > 0.5).astype(np.float32)).to(dev)      # two-valued, as argmax stacks
    ones = torch.ones((LR, LR), dtype=torch.float32, device=dev)
    angles = rng.uniform(-0.15, 0.15, N).astype(np.float32)
    shifts = rng.uniform(-80, 80, (N, 2)).astype(np.float32)             # the reference's draw: up to 80 px of 512
    rot1, tr1 = T.rotation_transforms(-angles, HR, HR).reshape(1, N, 8), T.translation_transforms(-shifts).reshape(1, N, 8)
    rot = torch.as_tensor(np.repeat(rot1, K, axis=0)).to(dev).contiguous()
    tr = torch.as_tensor(np.repeat(tr1, K, axis=0)).to(dev).contiguous()
    y1, rot_each, tr_each = y.view(K * N, 1, LR, LR), rot.view(K * N, 1, 8), tr.view(K * N, 1, 8)

    def call():
        if impl == "fused":
            return ops.realign_moments(y, tr, rot, (HR, HR), want=("var", "nv"), wgt=ones)["var"]
        if impl == "planes":
            planes = ops.realign(y1, tr_each, rot_each, (HR, HR), "max").view(K, N, HR, HR)
            return torch.var(planes, dim=1, unbiased=False)
        return ops.realign(y, tr, rot, (HR, HR), "mean")

    for _ in range(WARMUP):
        out = call()
    torch.cuda.synchronize()
    windows = []
    for _ in range(WINDOWS):
        t0 = time.perf_counter()
        for _ in range(CALLS):
            out = call()
        torch.cuda.synchronize()
        windows.append((time.perf_counter() - t0) * 1e6 / CALLS)
    print(json.dumps({"what": "run", "impl": impl, "classes": K, "n": N, "calls": CALLS, "us_per_call": windows,
                      "checksum": float(torch.nan_to_num(out).double().sum())}))
    return 0


def compare(rounds):
    med = {impl: [] for impl in IMPLS}
    sums = {}
    for _ in range(rounds):
        for impl in IMPLS:                        # alternating: every round runs each implementation once
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--impl", impl], capture_output=True, text=True,
                               timeout=300)
            if r.returncode != 0:
                print(r.stdout[-2000:] + r.stderr[-2000:], file=sys.stderr)
                return r.returncode
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            med[impl].append(statistics.median(rec["us_per_call"]))
            sums[impl] = rec["checksum"]
    out = {"what": "compare", "classes": K, "n": N, "lr": LR, "hr": HR, "rounds": rounds, "calls_per_window": CALLS,
           "windows": WINDOWS}
    for impl in IMPLS:
        out[impl + "_us"] = statistics.median(med[impl])
        out[impl + "_spread_us"] = max(med[impl]) - min(med[impl])
    spread = max(out[i + "_spread_us"] for i in ("fused", "planes"))
    out["fused_over_planes"] = out["fused_us"] / out["planes_us"]
    out["fused_over_mean_once"] = out["fused_us"] / out["mean_once_us"]
    out["fused_faster_beyond_spread"] = out["planes_us"] - out["fused_us"] > spread
    out["checksums"] = sums
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--impl", choices=IMPLS)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    sys.exit(run(args.impl) if args.impl else compare(args.rounds))
