#!/usr/bin/env python3
"""The coverage-normalised mean of the realigned copies: one asr_realign_covered_f32 call (mean + coverage) against what the
library offered before it for the same result, on the MI355X ("Coverage-normalised fusions").

    python tools/bench_realign_covered.py --config 1|4 --impl fused|two_launch|mean_once     # one implementation, one process
    python tools/bench_realign_covered.py [--config 1|4] [--rounds 3]                         # the comparison

--config 1: BASELINE configs[1]'s SR shape, B = 1, N = 100, 128 x 128 -> 512 x 512; --config 4: configs[4]'s, N = 200,
256 x 256 -> 512 x 512 (default: both).  The inputs are copied from the host (no set-up kernel runs on the device), the weights
are per-copy planes in [0, 1]:
--impl fused:      one asr_realign_covered_f32 call, out_mean and out_cov (cov_min = 0.5);
--impl two_launch: asr_realign_mean_f32 on y * w, asr_realign_mean_f32 on w, one torch division (the product y * w is made once,
                   outside the timed window: the fused call takes y already weighted too);
--impl mean_once:  a single asr_realign_mean_f32 call on y * w -- the price of the second plane is fused - mean_once.
An --impl run warms up, then times WINDOWS windows of CALLS calls each with a host clock around a device synchronise, and
prints one JSON line with the microseconds per call of every window.  The comparison starts each implementation in a process of
its own, ROUNDS times, alternating them, and prints one JSON line per shape: the median per implementation, the run-to-run
spread (largest - smallest window median of one implementation over its rounds), fused / two_launch, and whether the difference
exceeds that spread.  It states what it measured; it gates nothing.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

CALLS, WINDOWS, WARMUP = 50, 5, 10
CONFIGS = {1: dict(n=100, lr=128, hr=512), 4: dict(n=200, lr=256, hr=512)}
IMPLS = ("fused", "two_launch", "mean_once")


def run(config, impl):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch
    from asr_amd import ops, transforms as T

    c = CONFIGS[config]
    n, lr, hr = c["n"], c["lr"], c["hr"]
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    w = torch.as_tensor(rng.random((1, n, lr, lr), dtype=np.float32)).to(dev)
    yw = torch.as_tensor(rng.random((1, n, lr, lr), dtype=np.float32)).to(dev) * w
    angles = rng.uniform(-0.15, 0.15, n).astype(np.float32)
    shifts = rng.uniform(-80, 80, (n, 2)).astype(np.float32)             # the reference's draw: up to 80 px of 512
    rot = torch.as_tensor(T.rotation_transforms(-angles, hr, hr).reshape(1, n, 8)).to(dev)
    tr = torch.as_tensor(T.translation_transforms(-shifts).reshape(1, n, 8)).to(dev)

    def call():
        if impl == "fused":
            return ops.realign_covered(yw, w, tr, rot, (hr, hr), want=("mean", "cov"))["mean"]
        if impl == "two_launch":
            s, cov = ops.realign(yw, tr, rot, (hr, hr), "mean"), ops.realign(w, tr, rot, (hr, hr), "mean")
            return torch.where(cov * n >= 0.5, s / cov, torch.zeros_like(s))
        return ops.realign(yw, tr, rot, (hr, hr), "mean")

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
    print(json.dumps({"what": "run", "config": config, "impl": impl, "n": n, "calls": CALLS, "us_per_call": windows,
                      "checksum": float(torch.nan_to_num(out).double().sum())}))
    return 0


def compare(configs, rounds):
    status = 0
    for config in configs:
        med = {impl: [] for impl in IMPLS}
        sums = {}
        for _ in range(rounds):
            for impl in IMPLS:                        # alternating: every round runs each implementation once
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--config", str(config), "--impl", impl],
                                   capture_output=True, text=True, timeout=300)
                if r.returncode != 0:
                    print(r.stdout[-2000:] + r.stderr[-2000:], file=sys.stderr)
                    return r.returncode
                rec = json.loads(r.stdout.strip().splitlines()[-1])
                med[impl].append(statistics.median(rec["us_per_call"]))
                sums[impl] = rec["checksum"]
        out = {"what": "compare", "config": config, "rounds": rounds, "calls_per_window": CALLS, "windows": WINDOWS}
        for impl in IMPLS:
            out[impl + "_us"] = statistics.median(med[impl])
            out[impl + "_spread_us"] = max(med[impl]) - min(med[impl])
        spread = max(out[i + "_spread_us"] for i in ("fused", "two_launch"))
        out["fused_over_two_launch"] = out["fused_us"] / out["two_launch_us"]
        out["second_plane_us"] = out["fused_us"] - out["mean_once_us"]
        out["fused_faster_beyond_spread"] = out["two_launch_us"] - out["fused_us"] > spread
        out["checksums"] = sums
        print(json.dumps(out), flush=True)
    return status


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, choices=sorted(CONFIGS))
    ap.add_argument("--impl", choices=IMPLS)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if args.impl:
        sys.exit(run(args.config or 1, args.impl))
    sys.exit(compare([args.config] if args.config else sorted(CONFIGS), args.rounds))
