#!/usr/bin/env python3
"""What HotPath's public methods launch and return on one small fixed-seed image, case by case.

    python tests/golden/make_hotpath_traces.py [--out FILE]     # on the MI355X; writes tests/golden/hotpath_traces.json

Each case records "calls", the ordered names of the C entry points issued through the package's ``call`` while the method
(and the .result() of a submitted handle) runs, and "out", the sha256 of every int32 mask or label map it returns and of its
``ious`` / ``counts`` / ``band_counts`` (and Mean_IOU) arrays, plus "adam_after", where the global Adam step counter stands
afterwards.  The forward pass is not part of the trace: its launches do not go through ``call``, and
tests/golden/engine_plan_digests.json pins them.  tests/test_gpu_hotpath_traces.py replays the cases and compares.

The model, image, ground truth and draws (small_inputs, which tests/test_gpu_labelmap_path.py's ``small`` fixture returns too):
a 64 x 64 Xception model on seeded synthetic weights with classes 3, 8 and 15 shifted until they win a share of the pixels, six
copies in forward batches of four and two.  Every case gets a fresh solver whose Adam counter stands at 40.
"""
import argparse
import contextlib
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(HERE, "hotpath_traces.json")
WIN = [3, 8, 15]                         # classes made to win
REQ = [5, 3, 12, 8, 17, 15]              # label-map class set: the winners between classes that win nothing
LOSERS = (5, 12, 17)
MODES = ("argmax", "slice", "slice_max")
ALL_TYPES = ("aug", "max", "mean")
BANDS = [3, 1, 2, 1]
TH, N_AUG, ITERS, BATCH, ADAM0, LANE = 0.2, 6, 5, 4, 40, 1


@contextlib.contextmanager
def recorded_calls():
    """Every module of the package that holds ``_lib.call`` under the name ``call`` gets a wrapper that notes the entry
    point's name first; yields the list the names go to."""
    from asr_amd import _lib
    orig, names = _lib.call, []

    def call(name, *args):
        names.append(name)
        return orig(name, *args)

    pkg = _lib.__name__.rsplit(".", 1)[0]
    holders = [m for n, m in list(sys.modules.items())
               if m is not None and (n == pkg or n.startswith(pkg + ".")) and getattr(m, "call", None) is orig]
    for m in holders:
        m.call = call
    try:
        yield names
    finally:
        for m in holders:
            m.call = orig


def _sha(a):
    a = np.ascontiguousarray(a)
    return f"{a.dtype}{list(a.shape)}:{hashlib.sha256(a.tobytes()).hexdigest()}"


def digest(v):
    """Tensors and arrays -> dtype, shape and sha256 of the bytes; dicts and lists keep their structure; ints stay."""
    if isinstance(v, torch.Tensor):
        assert v.dtype == torch.int32, v.dtype
        return _sha(v.cpu().numpy())
    if isinstance(v, dict):
        return {str(k): digest(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [digest(x) for x in v]
    if isinstance(v, (int, np.integer)):
        return int(v)
    return _sha(np.asarray(v))                  # numpy arrays, and floats as float64


def make_sr():
    from asr_amd.superresolution_scripts.optimizer import Optimizer
    from asr_amd.superresolution_scripts.superresolution import Superresolution
    opt = Optimizer("adam", 1e-3, amsgrad=True, lr_scheduler=True, decay_steps=60, decay_rate=0.3)
    sr = Superresolution(1.0, 0.3, 0.7, 0.0, num_iter=ITERS, num_aug=N_AUG, optimizer=opt, feature_size=(16, 16),
                         output_size=(64, 64))
    sr.optimizer.optimizer.iterations = ADAM0
    return sr


def shift_classes(model, image_dev, ids, fraction=0.25):
    """engine.shift_logit_bias for each class in turn (tools/bench_class_sets.py): class c then wins on about `fraction` of the
    un-augmented image's pixels; seeded synthetic weights never make it win by themselves.  Returns {class: shift}."""
    out = {}
    for c in ids:
        logits = model.predict_device(image_dev[None].contiguous(), batch_size=1)[0]
        other = logits.clone()
        other[..., c] = float("-inf")
        out[c] = float(torch.quantile((other.max(dim=-1).values - logits[..., c]).flatten(), fraction))
        model.engine.shift_logit_bias(c, out[c])
    return out


def small_inputs(dev):
    """(model, image, ground truth, angles, shifts) of the small label-map tests and of the cases here."""
    from bench import synth_image
    from asr_amd import ops, weights as W
    from asr_amd.model import DeeplabModel
    from asr_amd.superresolution_scripts.augmentation_utils import draw_augmentation_parameters
    model = DeeplabModel(W.make_synthetic_weights(1234, 21), (64, 64, 3), 21, False, None)      # Xception, OS 16
    img = ops.to_device(synth_image(np.random.default_rng(21), 64), device=dev)
    shift_classes(model, img, WIN)
    logits0 = model.predict_device(img[None].contiguous(), batch_size=1)[0].contiguous()
    gt = ops.standard_mask_classes(logits0, (64, 64), WIN).sum(dim=0).to(torch.int32)
    gt[32:34] = 255                                                                             # a void band
    gt[:8, :8] = 12                                                                             # a class the model never predicts
    np.random.seed(17)
    angles, shifts = draw_augmentation_parameters(N_AUG, 0.15, 8)
    return model, img, gt.contiguous(), angles, shifts


def fixture(dev):
    """small_inputs and the classes of LOSERS that are the argmax of no pixel of any copy."""
    from asr_amd import ops
    from asr_amd.superresolution_scripts import augmentation_utils as au
    model, img, gt, angles, shifts = small_inputs(dev)
    logits = model.predict_device(au.augment_on_device(img, angles, shifts).contiguous(), batch_size=N_AUG)
    won = set(int(v) for v in torch.unique(ops.argmax(logits.contiguous())).cpu())
    return model, img, gt, angles, shifts, [c for c in LOSERS if c not in won]


def cases(fix):
    """name -> function of a fresh solver that runs the case and returns its result."""
    from asr_amd.pipeline import HotPath
    model, img, gt, angles, shifts, losers = fix
    out = {}

    def single(method, mode, types, start):
        def run(sr):
            path = HotPath(model, sr, class_id=8, mode=mode, th_factor=TH, batch_size=BATCH)
            kw = dict(gt_dev=gt, adam_start=start, sr_types=types)
            if method == "run_image":
                return path.run_image(img, angles, shifts, **kw)
            if method == "submit_image":
                return path.submit_image(img, angles, shifts, **kw).result()
            return path.submit_lane(LANE, img, angles, shifts, **kw).result()
        return run

    for method in ("run_image", "submit_image", "submit_lane"):
        for mode in MODES:
            out[f"{method} {mode} all"] = single(method, mode, ALL_TYPES, 7)
            out[f"{method} {mode} max"] = single(method, mode, ("max",), None)

    def classes(mode, starts):
        return lambda sr: HotPath(model, sr, mode=mode, th_factor=TH, batch_size=BATCH).run_image_classes(
            img, angles, shifts, WIN, gt_dev=gt, adam_starts=starts)

    for mode in MODES:
        out[f"run_image_classes {mode} starts"] = classes(mode, {3: 0, 8: 3 * ITERS, 15: 7 * ITERS + 2})
        out[f"run_image_classes {mode} consecutive"] = classes(mode, None)

    def labels(ids, prune, bands):
        extra = dict(band_widths=BANDS, band_ignore_label=255) if bands else {}
        return lambda sr: HotPath(model, sr, mode="argmax", th_factor=TH, batch_size=BATCH).run_image_labels(
            img, angles, shifts, ids, gt_dev=gt, prune=prune, **extra)

    for prune in (True, False):
        for bands in (False, True):
            out[f"run_image_labels prune={int(prune)} bands={int(bands)}"] = labels(REQ, prune, bands)
    assert len(losers) >= 2, losers
    out["run_image_labels pruned to empty"] = labels(losers, True, True)
    return out


def run_cases(dev):
    """{case: {"calls": [...], "out": digests, "adam_after": int}} -- the content of hotpath_traces.json."""
    from asr_amd.pipeline import HotPath
    fix = fixture(dev)
    model, img, gt, angles, shifts, _losers = fix
    # the first forward of a (batch, lane) builds its plan: done here, so that no case depends on which ran before it
    warm = HotPath(model, make_sr(), class_id=8, mode="argmax", th_factor=TH, batch_size=BATCH)
    warm.run_image(img, angles, shifts, gt_dev=gt)
    warm.submit_lane(LANE, img, angles, shifts, gt_dev=gt).result()
    torch.cuda.synchronize()
    out = {}
    for name, run in cases(fix).items():
        sr = make_sr()
        with recorded_calls() as names:
            res = run(sr)
            torch.cuda.synchronize()
        out[name] = {"calls": list(names), "out": digest(res), "adam_after": int(sr.optimizer.optimizer.iterations)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    out = run_cases(torch.device("cuda", 0))
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {args.out}: {len(out)} cases, {sum(len(c['calls']) for c in out.values())} calls")


if __name__ == "__main__":
    main()
