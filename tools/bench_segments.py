#!/usr/bin/env python3
"""ops.segment_match on the MI355X ("Segments"): 4 label maps of 512 x 512 against one truth, the four maps of one
image in HotPath.run_image_labels, on three inputs:

  blobs         a seeded blob-like truth (a coarse random grid of 6 values, void among them, blown up 16 x) against four copies
                of it with 8 % of the pixels replaced by random values: large segments that match, and specks that do not
  checkerboard  an all-equal truth against 4-connected checkerboards: every pixel a segment of its own, h * w distinct pairs
                per map, 1024 in every tile -- both tables at their fullest
  one_region    an all-equal truth against all-equal maps: every tile adds to the same pair, the contention case

    python tools/bench_segments.py [--size 512] [--maps 4] [--labels 21] [--connectivity 8] [--rounds 5]

Seeded inputs are copied from the host, every call is warmed up, and then ROUNDS rounds alternate the inputs; in each, a window of
CALLS calls is timed with a host clock around a device synchronise, for three things: "label_and_match", the three calls
run_image_labels makes (label_regions of the truth, label_regions of the maps, segment_match); "match", segment_match alone on
given regions; and "torch_unique", a torch restatement of its pair counting alone on the same regions -- the 64-bit pair keys of
the counted pixels through torch.unique(return_counts=True) -- which stops short of the areas, the matches and the planes.  One
JSON line: per input and call the median and the smallest and largest window in microseconds per call, and the summed TP, FP, FN.
It states what it measured and gates nothing; without a GPU it fails."""
import argparse
import json
import os
import statistics
import sys
import time

CALLS, WARMUP = 50, 5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def blob_pair(maps, size, seed=0):
    import numpy as np
    rng = np.random.default_rng(seed)
    values = np.array([0, 3, 8, 12, 15, 255], dtype=np.int32)
    coarse = rng.choice(values, size=((size + 15) // 16, (size + 15) // 16), p=(0.5, 0.1, 0.1, 0.1, 0.1, 0.1))
    truth = np.kron(coarse, np.ones((16, 16), np.int32))[:size, :size].astype(np.int32)
    preds = np.repeat(truth[None], maps, axis=0)
    noise = rng.random(preds.shape) < 0.08
    return truth, np.where(noise, rng.choice(values[:5], size=preds.shape), preds).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--maps", type=int, default=4)
    ap.add_argument("--labels", type=int, default=21)
    ap.add_argument("--connectivity", type=int, choices=[4, 8], default=8)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from asr_amd import _lib, ops

    dev = _lib.require_gpu()
    n, L = args.size * args.size, args.labels
    truth, preds = blob_pair(args.maps, args.size)
    y, x = np.mgrid[:args.size, :args.size]
    checker = np.repeat(np.where((y + x) & 1, 7, 2).astype(np.int32)[None], args.maps, axis=0)
    flat = torch.full((args.size, args.size), 7, dtype=torch.int32, device=dev)
    # (truth, predictions, connectivity): the checkerboard is one only under 4-connectivity
    inputs = {"blobs": (torch.as_tensor(truth).to(dev), torch.as_tensor(preds).to(dev), args.connectivity),
              "checkerboard": (flat, torch.as_tensor(checker).to(dev), 4),
              "one_region": (flat, flat.expand(args.maps, -1, -1).contiguous(), args.connectivity)}
    regions = {k: (ops.label_regions(t, c), ops.label_regions(p, c)) for k, (t, p, c) in inputs.items()}
    out = torch.empty((args.maps, L, 4), dtype=torch.int64, device=dev)
    offsets = (torch.arange(args.maps, device=dev, dtype=torch.int64) * n).view(-1, 1, 1)

    def label_and_match(k):
        t, p, c = inputs[k]
        return ops.segment_match(t, p, L, c, truth_regions=ops.label_regions(t, c), pred_regions=ops.label_regions(p, c), out=out)

    def match(k):
        t, p, c = inputs[k]
        return ops.segment_match(t, p, L, c, truth_regions=regions[k][0], pred_regions=regions[k][1], out=out)

    def torch_unique(k):
        t, p, _ = inputs[k]
        (t_root, _), (p_root, _) = regions[k]
        counted = (t >= 0) & (t < L) & (p >= 1) & (p < L)
        keys = ((t_root.to(torch.int64) << 32) | (p_root.to(torch.int64) + offsets))[counted]
        return torch.unique(keys, return_counts=True)

    calls = {"label_and_match": label_and_match, "match": match, "torch_unique": torch_unique}
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
    rec = {"what": "bench_segments", "size": args.size, "maps": args.maps, "labels": L, "connectivity": args.connectivity,
           "rounds": args.rounds, "calls_per_window": CALLS,
           "workspace_MiB": round(_lib.load().asr_segment_match_workspace_bytes(args.maps, args.size, args.size) / 2 ** 20, 1)}
    for k in inputs:
        counts = match(k).cpu().numpy()
        pairs, pixels = torch_unique(k)
        rec[k + "_tp_fp_fn"] = counts[:, :, :3].sum(axis=(0, 1)).tolist()
        rec[k + "_distinct_pairs"] = int(pairs.numel())
        assert int(pixels.sum()) <= args.maps * n
        for c in calls:
            w = us[(k, c)]
            rec[f"{k}_{c}_us"] = {"median": round(statistics.median(w), 2), "min": round(min(w), 2), "max": round(max(w), 2)}
    print(json.dumps(rec), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
