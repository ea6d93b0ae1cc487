"""scripts/validate_classes.py end to end: four seeded synthetic 512 x 512 images (boxes over noise) whose ground truths hold
{8}, {8, 12}, {3, 8, 15} and background only.  Every CSV value must equal the mean this test computes itself from per-class
HotPath.run_image calls fed the same draws and Adam starts; a 2-rank gloo rehearsal on the one GPU writes the same bytes."""
import csv
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from bench import shifted_weights, synth_image
from conftest import ROOT

pytestmark = pytest.mark.gpu

SCRIPT = os.path.join(ROOT, "scripts", "validate_classes.py")
BOXES = [
    {8: (100, 400, 100, 400)},
    {8: (50, 250, 50, 450), 12: (300, 480, 100, 400)},
    {3: (20, 200, 20, 200), 8: (220, 480, 30, 250), 15: (250, 480, 280, 490)},
    {},
]
SHIFTED = [3, 8, 12, 15]
N_AUG, ITERS, TH, ANGLE, SHIFT = 8, 10, 0.2, 0.15, 20
COLOR = {3: (0.9, 0.1, 0.1), 8: (0.1, 0.8, 0.2), 12: (0.2, 0.2, 0.9), 15: (0.9, 0.9, 0.1)}


def _dataset(root):
    from PIL import Image
    img_dir, gt_dir = os.path.join(root, "images"), os.path.join(root, "gt")
    os.makedirs(img_dir)
    os.makedirs(gt_dir)
    for g, boxes in enumerate(BOXES):
        rgb = synth_image(np.random.default_rng(500 + g), 512)
        lab = np.zeros((512, 512), np.uint8)
        for c, (y0, y1, x0, x1) in boxes.items():
            rgb[y0:y1, x0:x1] = 0.5 * rgb[y0:y1, x0:x1] + 0.5 * np.array(COLOR[c], np.float32)
            lab[y0:y1, x0:x1] = c
            lab[y0:y0 + 3, x0:x1] = 255                                  # a void edge, as in VOC label maps
        Image.fromarray((rgb * 255).astype(np.uint8)).save(os.path.join(img_dir, f"{g}.jpg"), quality=95)
        Image.fromarray(lab, mode="L").save(os.path.join(gt_dir, f"{g}.png"))
    return img_dir, gt_dir


def _weights(root, dev):
    """Seeded synthetic weights with the logits bias of classes 3, 8, 12, 15 shifted so that each wins a share of the pixels of
    image 2 (bench.calibrate_class_bias, one class after the other), written as an .npz."""
    from asr_amd import ops, weights as W
    from asr_amd.model import DeeplabModel
    from asr_amd.utils import load_image
    w = W.make_synthetic_weights(1234, 21)
    model = DeeplabModel(w, (512, 512, 3), 21, False, None)
    img = ops.to_device(load_image(os.path.join(root, "images", "2.jpg"), image_size=(512, 512), normalize=True), device=dev)
    for c in SHIFTED:
        logits = model.predict_device(img[None].contiguous(), batch_size=1)[0]
        other = logits.clone()
        other[..., c] = float("-inf")
        delta = float(torch.quantile((other.max(dim=-1).values - logits[..., c]).flatten(), 0.2))
        model.engine.shift_logit_bias(c, delta)
        w = shifted_weights(w, c, delta)
    path = os.path.join(root, "weights.npz")
    np.savez(path, **{k: np.asarray(v) for k, v in w.items()})
    del model
    return path


def _args(img_dir, gt_dir, weights, out):
    return ["--images", img_dir, "--gt", gt_dir, "--num_aug", str(N_AUG), "--num_iter", str(ITERS), "--mode", "argmax",
            "--angle_max", str(ANGLE), "--shift_max", str(SHIFT), "--th_factor", str(TH), "--weights", weights, "--out", out]


def _run(cmd, env=None):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def _expected(img_dir, gt_dir, weights):
    """Per-class HotPath.run_image calls, image by image in the script's order, with the script's draws and Adam starts."""
    from asr_amd import distributed as D, ops
    from asr_amd.model import DeeplabV3Plus
    from asr_amd.pipeline import HotPath
    from asr_amd.superresolution_scripts.optimizer import Optimizer
    from asr_amd.superresolution_scripts.superresolution import Superresolution
    from asr_amd.utils import load_image
    model = DeeplabV3Plus(input_shape=(512, 512, 3), classes=21, OS=16, last_activation=None, load_weights=True,
                          weights_path=weights).build_model(final_upsample=False)
    opt = Optimizer("adam", 1e-3, amsgrad=True, lr_scheduler=True, decay_steps=60, decay_rate=0.3)
    sr = Superresolution(1, 0.3, 0.7, 0.0, num_iter=ITERS, num_aug=N_AUG, optimizer=opt, feature_size=(128, 128),
                         output_size=(512, 512))
    params = D.replay_augmentation_stream(len(BOXES), N_AUG, ANGLE, SHIFT, seed=1234)
    per_class = {}
    for g, boxes in enumerate(BOXES):
        img = ops.to_device(load_image(os.path.join(img_dir, f"{g}.jpg"), image_size=(512, 512), normalize=True))
        lab = load_image(os.path.join(gt_dir, f"{g}.png"), image_size=(512, 512), normalize=False, is_png=True,
                         resize_method="nearest")[..., 0].astype(np.int32)
        gt = ops.to_device(lab, torch.int32)
        for c in sorted(boxes):
            start = ITERS * sum(1 for b in BOXES[:g] if c in b)       # earlier images that hold c, one solve each
            res = HotPath(model, sr, class_id=c, mode="argmax", th_factor=TH, batch_size=16).run_image(
                img, *params[g], gt_dev=gt, adam_start=start)
            per_class.setdefault(c, []).append(res["ious"])
    fields = {"aug_iou_multiple": "aug_bg", "standard_iou_multiple": "standard_bg", "aug_iou_single": "aug_single",
              "standard_iou_single": "standard_single", "max_iou": "max", "mean_iou": "mean"}
    out = {}
    for c, recs in sorted(per_class.items()):
        t = np.asarray(recs)
        out[f"Class {c}"] = ({col: float(np.mean(t[:, D.IOU_FIELDS.index(f)])) for col, f in fields.items()}, len(recs))
    return out


def _read(path):
    with open(path, newline="") as fh:
        rows = list(csv.reader(fh))
    return rows[0], rows[1:]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_validate_classes_script_matches_per_class_runs(dev, tmp_path):
    root = str(tmp_path)
    img_dir, gt_dir = _dataset(root)
    weights = _weights(root, dev)
    out1 = os.path.join(root, "one.csv")
    _run([sys.executable, SCRIPT] + _args(img_dir, gt_dir, weights, out1))
    header, rows = _read(out1)
    assert header == ["Name", "aug_iou_multiple", "standard_iou_multiple", "aug_iou_single", "standard_iou_single", "max_iou",
                      "mean_iou", "n_images"]
    exp = _expected(img_dir, gt_dir, weights)
    assert [r[0] for r in rows] == list(exp) == ["Class 3", "Class 8", "Class 12", "Class 15"]
    for r in rows:
        means, count = exp[r[0]]
        assert int(r[7]) == count
        for col, v in zip(header[1:7], r[1:7]):
            got, ref = float(v), means[col]
            assert (math.isnan(got) and math.isnan(ref)) or got == ref, (r[0], col, got, ref)
    live = [r[0] for r in rows if math.isfinite(float(r[3])) and float(r[3]) > 0]
    assert len(live) >= 2, rows                                          # not NaN against NaN
    assert [int(r[7]) for r in rows] == [1, 3, 1, 1]
    # 2 ranks (gloo collectives) on the one GPU: the same bytes
    out2 = os.path.join(root, "two.csv")
    env = dict(os.environ, ASR_DIST_BACKEND="gloo")
    _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
          "--master-port", str(_free_port()), SCRIPT] + _args(img_dir, gt_dir, weights, out2), env=env)
    with open(out1, "rb") as a, open(out2, "rb") as b:
        assert a.read() == b.read()
