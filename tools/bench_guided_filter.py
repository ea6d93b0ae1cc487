#!/usr/bin/env python3
"""The guided filter (asr_guided_prepare_f32 / asr_guided_apply_f32) against a torch restatement on the same device, on the
MI355X ("Guided filter").

    python tools/bench_guided_filter.py --impl hip|torch [--size 512] [--planes 20] [--radius 8]     # one side, one process
    python tools/bench_guided_filter.py [--rounds 3] [--size 512] [--planes 20] [--radius 8]         # the comparison
    python tools/bench_guided_filter.py --e2e [--images 6] [--radius 8]                              # run_image_labels' SR stage

--impl hip: ops.guided_prepare, ops.guided_apply on P planes, and ops.guided_filter (both) -- three timings.
--impl torch: what a user would write without the kernel: F.avg_pool2d(kernel 2r+1, stride 1, padding r,
count_include_pad=False) for every window mean (the clipped windows of the rule), torch.linalg.inv of the per-pixel 3x3
matrices in the guide-only part (shared by the planes, like the kernel's state) and a batched 3x3 product per plane.  The same
three timings.
An --impl run copies seeded inputs from the host, warms up, then times WINDOWS windows of CALLS calls each with a host clock
around a device synchronise and prints one JSON line with the microseconds per call of every window, for each of the three.
The comparison starts each side in a process of its own, ROUNDS times, alternating them, and prints one JSON line: the median
per side and stage, the run-to-run spread (largest - smallest window median of one side over its rounds), the bytes apply must
move (p in, q out, 2 x 4 workspace floats per pixel and plane, plus the guide and the state read once per pass) and the TB/s
that makes against the 8 TB/s of the HBM, hip / torch, whether the difference exceeds the spread, and the largest difference
between the two sides' outputs.  It states what it measured; it gates nothing.
--e2e: BASELINE configs[1]'s label-map workload (512 x 512, N = 100, argmax, 50 AMSGrad iterations, classes 3, 8 and 15 made to
win) through HotPath.run_image_labels with and without guide=(radius, 1e-3), alternated A B A B in one process; the
_sr_stage_ms per image of both, pruned (the winning classes) and with prune=False (20 planes per SR type).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

CALLS, WINDOWS, WARMUP = 20, 5, 5
EPS = 1e-3
STAGES = ("prepare", "apply", "whole")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def torch_prepare(I, r, eps):
    """I [3, H, W] -> (mu [3, H, W], inverse [H, W, 3, 3])."""
    import torch
    import torch.nn.functional as F
    box = lambda x: F.avg_pool2d(x[None], 2 * r + 1, stride=1, padding=r, count_include_pad=False)[0]
    mu = box(I)
    S = box((I[:, None] * I[None]).reshape(9, *I.shape[1:])).reshape(3, 3, *I.shape[1:]) - mu[:, None] * mu[None]
    M = S.permute(2, 3, 0, 1) + eps * torch.eye(3, device=I.device)
    return mu, torch.linalg.inv(M)


def torch_apply(state, I, p, r):
    """p [P, H, W] -> q [P, H, W]."""
    import torch
    import torch.nn.functional as F
    mu, Minv = state
    P = p.shape[0]
    box = lambda x: F.avg_pool2d(x[None], 2 * r + 1, stride=1, padding=r, count_include_pad=False)[0]
    m = box(p)
    c = box((p[:, None] * I[None]).reshape(3 * P, *p.shape[1:])).reshape(P, 3, *p.shape[1:]) - mu[None] * m[:, None]
    a = torch.einsum("hwij,pjhw->pihw", Minv, c)
    b = m - (a * mu[None]).sum(dim=1)
    return (box(a.reshape(3 * P, *p.shape[1:])).reshape(P, 3, *p.shape[1:]) * I[None]).sum(dim=1) + box(b)


def run(impl, size, planes, radius):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from asr_amd import ops

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    guide = torch.as_tensor(rng.random((size, size, 3), dtype=np.float32)).to(dev)
    p = torch.as_tensor(rng.standard_normal((planes, size, size), dtype=np.float32)).to(dev)
    out = torch.empty_like(p)
    if impl == "hip":
        prepare = lambda: ops.guided_prepare(guide, radius, EPS)
        state = prepare()
        apply = lambda: ops.guided_apply(state, guide, p, out=out)
        whole = lambda: ops.guided_filter(guide, p, radius, EPS, out=out)
    else:
        chw = guide.permute(2, 0, 1).contiguous()
        prepare = lambda: torch_prepare(chw, radius, EPS)
        state = prepare()
        apply = lambda: torch_apply(state, chw, p, radius)
        whole = lambda: torch_apply(torch_prepare(chw, radius, EPS), chw, p, radius)
    rec = {"what": "run", "impl": impl, "size": size, "planes": planes, "radius": radius, "calls": CALLS}
    for name, fn in zip(STAGES, (prepare, apply, whole)):
        for _ in range(WARMUP):
            res = fn()
        torch.cuda.synchronize()
        windows = []
        for _ in range(WINDOWS):
            t0 = time.perf_counter()
            for _ in range(CALLS):
                res = fn()
            torch.cuda.synchronize()
            windows.append((time.perf_counter() - t0) * 1e6 / CALLS)
        rec[name + "_us"] = windows
    q = res if isinstance(res, torch.Tensor) else out
    rec["checksum"] = float(q.double().sum())
    rec["probe"] = [float(v) for v in q.flatten()[:: max(1, q.numel() // 64)][:64].double().cpu()]
    print(json.dumps(rec))
    return 0


def apply_bytes(size, planes):
    """What asr_guided_apply_f32 must move: per pixel and plane p in, q out and the 4 workspace floats written and read back;
    per pixel and pass the guide (3 floats, both passes) and the state (9 floats, first pass)."""
    px = size * size
    return 4 * (px * planes * (1 + 1 + 2 * 4) + px * (3 + 9) + px * 3)


def compare(rounds, size, planes, radius):
    med = {impl: {s: [] for s in STAGES} for impl in ("hip", "torch")}
    probe, sums = {}, {}
    for _ in range(rounds):
        for impl in ("hip", "torch"):                     # alternating: every round runs each side once
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--impl", impl, "--size", str(size), "--planes",
                                str(planes), "--radius", str(radius)], capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                print(r.stdout[-2000:] + r.stderr[-2000:], file=sys.stderr)
                return r.returncode
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            for s in STAGES:
                med[impl][s].append(statistics.median(rec[s + "_us"]))
            probe[impl], sums[impl] = rec["probe"], rec["checksum"]
    out = {"what": "compare", "size": size, "planes": planes, "radius": radius, "eps": EPS, "rounds": rounds,
           "calls_per_window": CALLS, "windows": WINDOWS}
    for impl in ("hip", "torch"):
        for s in STAGES:
            out[f"{impl}_{s}_us"] = statistics.median(med[impl][s])
            out[f"{impl}_{s}_spread_us"] = max(med[impl][s]) - min(med[impl][s])
    out["hip_apply_us_per_plane"] = out["hip_apply_us"] / planes
    out["apply_bytes"] = apply_bytes(size, planes)
    out["hip_apply_TBps"] = out["apply_bytes"] / out["hip_apply_us"] * 1e-6
    out["hip_apply_share_of_8TBps"] = out["hip_apply_TBps"] / 8.0
    for s in STAGES:
        spread = max(out[f"hip_{s}_spread_us"], out[f"torch_{s}_spread_us"])
        out[f"{s}_hip_over_torch"] = out[f"hip_{s}_us"] / out[f"torch_{s}_us"]
        out[f"{s}_hip_faster_beyond_spread"] = out[f"torch_{s}_us"] - out[f"hip_{s}_us"] > spread
    out["max_abs_difference_of_probes"] = max(abs(a - b) for a, b in zip(probe["hip"], probe["torch"]))
    out["checksums"] = sums
    print(json.dumps(out), flush=True)
    return 0


def e2e(images, radius):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from bench import synth_image
    from asr_amd import distributed as D, ops, weights as W
    from asr_amd.model import DeeplabModel
    from asr_amd.pipeline import HotPath
    from asr_amd.superresolution_scripts.optimizer import Optimizer
    from asr_amd.superresolution_scripts.superresolution import Superresolution

    WIN, ALL, N, ITERS, BATCH, WARM = [3, 8, 15], list(range(1, 21)), 100, 50, 16, 1
    dev = torch.device("cuda", 0)
    model = DeeplabModel(W.make_synthetic_weights(1234, 21), (512, 512, 3), 21, False, None,
                         precision=os.environ.get("ASR_PRECISION", "f16x3"))
    imgs = [ops.to_device(synth_image(np.random.default_rng(1234 + j), 512), device=dev) for j in range(WARM + images)]

    def margin(im, c):                                   # tools/bench_labelmap.py's workload: background, then three winners
        logits = model.predict_device(im[None].contiguous(), batch_size=1)[0]
        other = logits.clone()
        other[..., c] = float("-inf")
        return (other.max(dim=-1).values - logits[..., c]).flatten()

    model.engine.shift_logit_bias(0, max(float(margin(im, 0).max()) for im in imgs) + 1.0)
    for c in WIN:
        model.engine.shift_logit_bias(c, float(torch.quantile(margin(imgs[0], c), 0.2)))
    params = D.replay_augmentation_stream(len(imgs), N, 0.15, 80)
    opt = Optimizer("adam", 1e-3, amsgrad=True, lr_scheduler=True, decay_steps=60, decay_rate=0.3)
    sr = Superresolution(1.0, 0.3, 0.7, 0.0, num_iter=ITERS, num_aug=N, optimizer=opt, feature_size=(128, 128),
                         output_size=(512, 512))
    path = HotPath(model, sr, mode="argmax", th_factor=0.2, batch_size=BATCH)

    def block(first, last, guided, prune):
        prof = {}
        for g in range(first, last):
            angles, shifts = params[g]
            path.run_image_labels(imgs[g], angles, shifts, ALL, adam_starts={c: g * ITERS for c in ALL}, prune=prune,
                                  profile=prof, **(dict(guide=(radius, EPS)) if guided else {}))
        return prof["_sr_stage_ms"] / (last - first)

    out = {"what": "e2e", "images": images, "radius": radius, "eps": EPS}
    for prune in (True, False):
        for guided in (False, True):
            block(0, WARM, guided, prune)
        ms = {False: [], True: []}
        for _ in range(2):                               # A B A B
            for guided in (False, True):
                ms[guided].append(block(WARM, len(imgs), guided, prune))
        key = "pruned" if prune else "all20"
        out[key + "_plain_sr_stage_ms"] = [round(v, 3) for v in ms[False]]
        out[key + "_guided_sr_stage_ms"] = [round(v, 3) for v in ms[True]]
        out[key + "_added_ms_per_image"] = round(float(np.mean(ms[True]) - np.mean(ms[False])), 3)
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--impl", choices=["hip", "torch"])
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--planes", type=int, default=20)
    ap.add_argument("--radius", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--images", type=int, default=6)
    args = ap.parse_args()
    if args.e2e:
        sys.exit(e2e(args.images, args.radius))
    if args.impl:
        sys.exit(run(args.impl, args.size, args.planes, args.radius))
    sys.exit(compare(args.rounds, args.size, args.planes, args.radius))
