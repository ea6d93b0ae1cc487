#!/usr/bin/env python3
"""ops.label_regions and ops.clean_labels on the MI355X ("Small regions"): 4 label maps of 512 x 512, the four maps
of one image in HotPath.run_image_labels, on two inputs:

  blobs      seeded blob-like maps (a coarse random grid of 6 values blown up 16 x, 8 % of the pixels then replaced by random
             values: specks and pin-holes over large regions, what a thresholded SR output looks like)
  one_region one all-equal map per plane: every union, every count and every walk meets the same root, the contention case

    python tools/bench_regions.py [--size 512] [--maps 4] [--min_area 16] [--connectivity 4] [--rounds 5]

Seeded inputs are copied from the host, both inputs and both calls are warmed up, and then ROUNDS rounds alternate the two
inputs; in each, a window of CALLS calls of label_regions and a window of CALLS calls of clean_labels (on the regions of the
same input) are timed with a host clock around a device synchronise.  One JSON line: per input and call the median and the
smallest and largest window in microseconds per call, the regions found, and the bytes a call must move (labels in; root and
area out, or the map out) with the GB/s that makes.  It states what it measured and gates nothing; without a GPU it fails."""
import argparse
import json
import os
import statistics
import sys
import time

CALLS, WARMUP = 50, 5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def blob_maps(maps, size, seed=0):
    import numpy as np
    rng = np.random.default_rng(seed)
    values = np.array([0, 3, 8, 12, 15, 255], dtype=np.int32)
    coarse = rng.choice(values, size=(maps, (size + 15) // 16, (size + 15) // 16), p=(0.5, 0.1, 0.1, 0.1, 0.1, 0.1))
    m = np.kron(coarse, np.ones((1, 16, 16), np.int32))[:, :size, :size]
    noise = rng.random(m.shape) < 0.08
    return np.where(noise, rng.choice(values, size=m.shape), m).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--maps", type=int, default=4)
    ap.add_argument("--min_area", type=int, default=16)
    ap.add_argument("--connectivity", type=int, choices=[4, 8], default=4)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from asr_amd import _lib, ops

    dev = _lib.require_gpu()
    inputs = {"blobs": torch.as_tensor(blob_maps(args.maps, args.size)).to(dev),
              "one_region": torch.full((args.maps, args.size, args.size), 7, dtype=torch.int32, device=dev)}
    regions = {k: ops.label_regions(v, args.connectivity) for k, v in inputs.items()}
    out = torch.empty_like(inputs["blobs"])
    calls = {"label_regions": lambda k: ops.label_regions(inputs[k], args.connectivity),
             "clean_labels": lambda k: ops.clean_labels(inputs[k], args.min_area, args.connectivity, regions=regions[k], out=out,
                                                        want_stats=True)}
    for k in inputs:
        for fn in calls.values():
            for _ in range(WARMUP):
                fn(k)
    torch.cuda.synchronize()
    us = {(k, c): [] for k in inputs for c in calls}
    for _ in range(args.rounds):
        for k in inputs:                                   # alternating: every round times each input once
            for c, fn in calls.items():
                t0 = time.perf_counter()
                for _ in range(CALLS):
                    fn(k)
                torch.cuda.synchronize()
                us[(k, c)].append((time.perf_counter() - t0) * 1e6 / CALLS)
    px = args.maps * args.size * args.size
    moved = {"label_regions": 4 * px * 3, "clean_labels": 4 * px * 4}          # labels -> root, area; labels, root, area -> out
    rec = {"what": "bench_regions", "size": args.size, "maps": args.maps, "min_area": args.min_area,
           "connectivity": args.connectivity, "rounds": args.rounds, "calls_per_window": CALLS}
    for k in inputs:
        _, stats = ops.clean_labels(inputs[k], args.min_area, args.connectivity, regions=regions[k], want_stats=True)
        rec[k + "_stats_per_map"] = stats.cpu().numpy().tolist()
        assert not bool((regions[k][0] < 0).any())
        for c in calls:
            w = us[(k, c)]
            rec[f"{k}_{c}_us"] = {"median": round(statistics.median(w), 2), "min": round(min(w), 2), "max": round(max(w), 2)}
            rec[f"{k}_{c}_GBps_of_minimum_bytes"] = round(moved[c] / statistics.median(w) * 1e-3, 1)
    print(json.dumps(rec), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
