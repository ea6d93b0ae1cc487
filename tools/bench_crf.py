#!/usr/bin/env python3
"""The windowed CRF (asr_crf_refine_f32) against a torch restatement on the same device, on the MI355X (DESIGN.md 7,
"Windowed CRF").

    python tools/bench_crf.py --impl hip|torch [--size 512] [--labels 21] [--radius 3] [--iters 5]     # one side, one process
    python tools/bench_crf.py [--rounds 3] [--size 512] [--radius 3] [--iters 5]                       # the comparison, L = 4 and 21
    python tools/bench_crf.py --e2e [--images 6] [--iters 5]                                           # run_image_labels' SR stage

--impl hip: ops.crf_refine of seeded unaries [L, size, size] against a seeded guide, labels only (the hot path's call).
--impl torch: what a user would write without the kernel: F.unfold windows (kernel 2r+1, zero padding, so a neighbour outside
the image carries weight 0 through an unfolded plane of ones) of the guide once per call for the two weight stacks, and of Q in
every iteration; softmax over the label axis; argmax of the final logits.
An --impl run copies seeded inputs from the host, warms up, then times WINDOWS windows of CALLS calls each with a host clock
around a device synchronise and prints one JSON line with the microseconds per call of every window.  The comparison starts each
side in a process of its own, ROUNDS times per label count, alternating them, and prints one JSON line per label count: the
median per side, the run-to-run spread (largest - smallest window median of one side over its rounds), the microseconds per
iteration, hip / torch, whether the difference exceeds the spread, and the share of pixels whose labels differ between the
sides.  It states what it measured; it gates nothing.
--e2e: BASELINE configs[1]'s label-map workload (512 x 512, N = 100, argmax, 50 AMSGrad iterations, classes 3, 8 and 15 made to
win) through HotPath.run_image_labels with and without crf={"iterations": T}, alternated A B A B in one process; the
_sr_stage_ms per image of both, pruned (the winning classes) and with prune=False (21 labels per SR type).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

CALLS, WINDOWS, WARMUP = 10, 5, 3
W_APP, W_SMOOTH, T_POS, T_RGB, T_SMOOTH = 4.0, 1.0, 2.0, 0.1, 1.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def torch_crf(guide_chw, z, r, iters):
    """guide [3, H, W], z [L, H, W] -> label indices [H, W] (argmax of the final logits)."""
    import torch
    import torch.nn.functional as F
    L, H, W = z.shape
    n = 2 * r + 1
    unfold = lambda x: F.unfold(x[None], n, padding=r).view(x.shape[0], n * n, H * W)
    inside = unfold(torch.ones((1, H, W), device=z.device))[0]                       # [n^2, HW]
    inside[n * n // 2] = 0.0                                                          # the pixel itself is no neighbour
    dy, dx = torch.meshgrid(torch.arange(-r, r + 1, device=z.device), torch.arange(-r, r + 1, device=z.device), indexing="ij")
    delta2 = (dy * dy + dx * dx).reshape(-1, 1).float()
    diff2 = ((unfold(guide_chw) - guide_chw.view(3, 1, H * W)) ** 2).sum(dim=0)
    a = torch.exp(torch.clamp(-delta2 / (2 * T_POS ** 2) - diff2 / (2 * T_RGB ** 2), min=-80.0)) * inside
    g = torch.exp(torch.clamp(-delta2 / (2 * T_SMOOTH ** 2), min=-80.0)) * inside
    a, g = a / a.sum(dim=0), g / g.sum(dim=0)
    zf = z.view(L, H * W)
    s, q = zf, torch.softmax(zf, dim=0)
    for _ in range(iters):
        u = unfold(q.view(L, H, W))                                                   # [L, n^2, HW]
        s = zf + W_APP * (u * a[None]).sum(dim=1) + W_SMOOTH * (u * g[None]).sum(dim=1)
        q = torch.softmax(s, dim=0)
    return s.argmax(dim=0).view(H, W)


def run(impl, size, labels, radius, iters):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from asr_amd import ops

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    guide = torch.as_tensor(rng.random((size, size, 3), dtype=np.float32)).to(dev)
    z = torch.as_tensor(rng.uniform(-1.5, 8.5, (labels, size, size)).astype(np.float32)).to(dev)
    z[0] = 0.0
    ids = list(range(1, labels))
    if impl == "hip":
        prm = ops.check_crf(dict(radius=radius, iterations=iters, w_app=W_APP, w_smooth=W_SMOOTH, theta_pos=T_POS,
                                 theta_rgb=T_RGB, theta_smooth=T_SMOOTH))
        out = torch.empty((size, size), dtype=torch.int32, device=dev)
        fn = lambda: ops.crf_refine(guide, z, ids, prm, out=out)
    else:
        chw = guide.permute(2, 0, 1).contiguous()
        fn = lambda: torch_crf(chw, z, radius, iters)
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
    rec = {"what": "run", "impl": impl, "size": size, "labels": labels, "radius": radius, "iters": iters, "calls": CALLS,
           "call_us": windows}
    path = os.environ.get("ASR_BENCH_CRF_LABELS")            # the comparison's hand-over of the label map
    if path:
        np.save(path, res.cpu().numpy().astype(np.int32))
    print(json.dumps(rec))
    return 0


def compare(rounds, size, radius, iters):
    import tempfile
    import numpy as np
    for labels in (4, 21):
        med, maps = {"hip": [], "torch": []}, {}
        with tempfile.TemporaryDirectory() as tmp:
            for _ in range(rounds):
                for impl in ("hip", "torch"):                 # alternating: every round runs each side once
                    env = dict(os.environ, ASR_BENCH_CRF_LABELS=os.path.join(tmp, impl + ".npy"))
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--impl", impl, "--size", str(size), "--labels",
                                        str(labels), "--radius", str(radius), "--iters", str(iters)], capture_output=True,
                                       text=True, timeout=600, env=env)
                    if r.returncode != 0:
                        print(r.stdout[-2000:] + r.stderr[-2000:], file=sys.stderr)
                        return r.returncode
                    rec = json.loads(r.stdout.strip().splitlines()[-1])
                    med[impl].append(statistics.median(rec["call_us"]))
                    maps[impl] = np.load(env["ASR_BENCH_CRF_LABELS"])
        out = {"what": "compare", "size": size, "labels": labels, "radius": radius, "iters": iters, "rounds": rounds,
               "calls_per_window": CALLS, "windows": WINDOWS}
        for impl in ("hip", "torch"):
            out[f"{impl}_call_us"] = statistics.median(med[impl])
            out[f"{impl}_call_spread_us"] = max(med[impl]) - min(med[impl])
        out["hip_us_per_iteration"] = out["hip_call_us"] / max(iters, 1)
        spread = max(out["hip_call_spread_us"], out["torch_call_spread_us"])
        out["hip_over_torch"] = out["hip_call_us"] / out["torch_call_us"]
        out["hip_faster_beyond_spread"] = out["torch_call_us"] - out["hip_call_us"] > spread
        out["share_of_pixels_labelled_differently"] = float((maps["hip"] != maps["torch"]).mean())
        print(json.dumps(out), flush=True)
    return 0


def e2e(images, iters):
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

    def block(first, last, crf, prune):
        prof = {}
        for g in range(first, last):
            angles, shifts = params[g]
            path.run_image_labels(imgs[g], angles, shifts, ALL, adam_starts={c: g * ITERS for c in ALL}, prune=prune,
                                  profile=prof, **(dict(crf={"iterations": iters}) if crf else {}))
        return prof["_sr_stage_ms"] / (last - first)

    out = {"what": "e2e", "images": images, "iters": iters}
    for prune in (True, False):
        for crf in (False, True):
            block(0, WARM, crf, prune)
        ms = {False: [], True: []}
        for _ in range(2):                               # A B A B
            for crf in (False, True):
                ms[crf].append(block(WARM, len(imgs), crf, prune))
        key = "pruned" if prune else "all20"
        out[key + "_plain_sr_stage_ms"] = [round(v, 3) for v in ms[False]]
        out[key + "_crf_sr_stage_ms"] = [round(v, 3) for v in ms[True]]
        out[key + "_added_ms_per_image"] = round(float(np.mean(ms[True]) - np.mean(ms[False])), 3)
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--impl", choices=["hip", "torch"])
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--labels", type=int, default=21)
    ap.add_argument("--radius", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--images", type=int, default=6)
    args = ap.parse_args()
    if args.e2e:
        sys.exit(e2e(args.images, args.iters))
    if args.impl:
        sys.exit(run(args.impl, args.size, args.labels, args.radius, args.iters))
    sys.exit(compare(args.rounds, args.size, args.radius, args.iters))
