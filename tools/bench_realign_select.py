#!/usr/bin/env python3
"""The pixel-wise median of the realigned copies: one asr_realign_select_f32 call against what the library offered before it,
on the MI355X ("Order statistics over the realigned copies").

    python tools/bench_realign_select.py --config 1|4 --impl parent|head|max_mean
    python tools/bench_realign_select.py --gate --parent P.csv --head H.csv --max_mean M.csv

--config 1: BASELINE configs[1]'s SR shape, B = 1, N = 100, 128 x 128 -> 512 x 512; --config 4: configs[4]'s, N = 200,
256 x 256 -> 512 x 512.  Each run makes 20 calls on the same inputs (copied from the host: no set-up kernel runs on the device):
--impl parent: the median without the select kernel -- one asr_realign_max_f32 call on the stack viewed as [B * N, 1, h, w],
    which returns the N warped planes (N * H * W floats written), then torch.sort(dim=0) and an index of the sorted stack.
    Only s[lo] is indexed, not the lerp with s[hi] that the even-n median needs and the head computes: the parent does a
    little less than the head, which favours the parent;
--impl head: one asr_realign_select_f32 call with the median's ranks;
--impl max_mean: asr_realign_max_mean_f32 on the same inputs -- the same per-copy work folded instead of selected, so the price
    of the selection is on record.
Run each under `rocprofv3 --kernel-trace --stats --output-format csv` in a process of its own; --gate then reads the three
*kernel_stats.csv files, sums ALL kernels of each run, and prints one JSON line with the microseconds per call, head / parent
(the gate: <= 0.5) and head / max_mean.  Exit status 1 when the gate fails.
"""
import argparse
import csv
import json
import os
import sys

CALLS = 20
CONFIGS = {1: dict(n=100, lr=128, hr=512), 4: dict(n=200, lr=256, hr=512)}

ap = argparse.ArgumentParser()
ap.add_argument("--config", type=int, choices=sorted(CONFIGS), default=1)
ap.add_argument("--impl", choices=["parent", "head", "max_mean"])
ap.add_argument("--gate", action="store_true")
ap.add_argument("--parent")
ap.add_argument("--head")
ap.add_argument("--max_mean")
args = ap.parse_args()


def total_us_per_call(path):
    with open(path, newline="") as fh:
        rows = list(csv.DictReader(fh))
    return sum(float(r["TotalDurationNs"]) for r in rows) / 1e3 / CALLS, {r["Name"][:80]: int(r["Calls"]) for r in rows}


def gate():
    out = {"what": "gate", "config": args.config, "calls": CALLS}
    for key in ("parent", "head", "max_mean"):
        out[key + "_us"], out[key + "_kernels"] = total_us_per_call(getattr(args, key))
    out["head_over_parent"] = out["head_us"] / out["parent_us"]
    out["head_over_max_mean"] = out["head_us"] / out["max_mean_us"]
    out["gate_head_le_half_parent"] = out["head_over_parent"] <= 0.5
    print(json.dumps(out))
    return 0 if out["gate_head_le_half_parent"] else 1


def run():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch
    from asr_amd import ops, transforms as T

    c = CONFIGS[args.config]
    n, lr, hr = c["n"], c["lr"], c["hr"]
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    y = torch.as_tensor(rng.random((1, n, lr, lr), dtype=np.float32)).to(dev)
    angles = rng.uniform(-0.15, 0.15, n).astype(np.float32)
    shifts = rng.uniform(-80, 80, (n, 2)).astype(np.float32)             # the reference's draw: up to 80 px of 512
    rot = torch.as_tensor(T.rotation_transforms(-angles, hr, hr).reshape(1, n, 8)).to(dev)
    tr = torch.as_tensor(T.translation_transforms(-shifts).reshape(1, n, 8)).to(dev)
    ranks = [ops.quantile_ranks(n, 0.5)]
    lo = ranks[0][0]
    torch.cuda.synchronize()
    for _ in range(CALLS):
        if args.impl == "parent":
            planes = ops.realign(y.view(n, 1, lr, lr), tr.view(n, 1, 8), rot.view(n, 1, 8), (hr, hr), "max")     # [N, H, W]
            out = torch.sort(planes, dim=0).values[lo].clone()
        elif args.impl == "head":
            out = ops.realign_select(y, tr, rot, (hr, hr), ranks=ranks, trim_k=None)[0]
        else:
            out = ops.realign(y, tr, rot, (hr, hr), "both")[0]
    torch.cuda.synchronize()
    moved = {"parent": (n * lr * lr + 2 * n * hr * hr + hr * hr) * 4, "head": (n * lr * lr + hr * hr) * 4,
             "max_mean": (n * lr * lr + 2 * hr * hr) * 4}[args.impl]
    print(json.dumps({"what": "run", "config": args.config, "impl": args.impl, "calls": CALLS, "n": n,
                      "least_bytes_per_call": moved, "checksum": float(out.cpu().double().sum())}))
    return 0


if __name__ == "__main__":
    if args.gate:
        sys.exit(gate())
    if not args.impl:
        ap.error("--impl or --gate")
    sys.exit(run())
