"""HotPath.run_image_labels on a small model input: the scores it fuses are those of run_image_classes (their thresholds are its
masks, bit for bit), each label map is the numpy fusion of those scores, the standard label map is the sum of the standard
masks; pruning classes that win no pixel changes no bit and no step counter, for Adam, Adagrad and the bilateral-TV prior; and
scripts/validate_labelmap.py end to end on the golden cat image, one rank and two."""
import csv
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from bench import shifted_weights, synth_image
from conftest import GOLDEN, ROOT
from test_labelmap_host import counts_numpy, fuse_numpy

sys.path.insert(0, GOLDEN)
from make_hotpath_traces import shift_classes as _shift_classes, small_inputs  # noqa: E402

pytestmark = pytest.mark.gpu

WIN = [3, 8, 15]                         # classes whose logit bias is shifted until they win a share of the pixels
REQ = [5, 3, 12, 8, 17, 15]              # requested set, unordered: the shifted classes between classes left alone
KEYS = ("standard", "aug", "max", "mean")
TH = 0.2


def _winners(model, img, angles, shifts):
    """The classes that are the argmax of some pixel of some copy, found without the code under test."""
    from asr_amd import ops
    from asr_amd.superresolution_scripts import augmentation_utils as au
    copies = au.augment_on_device(img, angles, shifts).contiguous()
    logits = model.predict_device(copies, batch_size=len(angles))
    return set(int(v) for v in torch.unique(ops.argmax(logits.contiguous())).cpu())


def _sr(kind, n, iters, feat, out, use_btv):
    from asr_amd.superresolution_scripts.optimizer import Optimizer
    from asr_amd.superresolution_scripts.superresolution import Superresolution
    if kind == "adam":
        opt = Optimizer("adam", 1e-3, amsgrad=True, lr_scheduler=True, decay_steps=60, decay_rate=0.3)
    else:
        opt = Optimizer(kind, 1e-2)
    return Superresolution(1.0, 0.3, 0.7, 0.0, num_iter=iters, num_aug=n, optimizer=opt, feature_size=feat, output_size=out,
                           use_BTV=use_btv)


@pytest.fixture(scope="module")
def small(dev):
    return small_inputs(dev)


@pytest.mark.parametrize("mode", ["argmax", "slice", "slice_max"])
def test_label_maps_are_the_fusion_of_the_class_set_scores(small, mode):
    from asr_amd import ops
    from asr_amd.pipeline import HotPath
    from asr_amd.utils import mean_iou_from_counts
    model, img, gt, angles, shifts = small
    sr = _sr("adam", 6, 5, (16, 16), (64, 64), False)
    starts = {c: 7 * j + 2 for j, c in enumerate(REQ)}
    sr.optimizer.optimizer.iterations = 123
    path = HotPath(model, sr, mode=mode, th_factor=TH, batch_size=4)
    res = path.run_image_labels(img, angles, shifts, REQ, gt_dev=gt, adam_starts=starts, prune=False, keep_scores=True)
    assert sr.optimizer.optimizer.iterations == 123                             # explicit starts leave the counter alone
    assert res["solved_ids"] == REQ
    ref = path.run_image_classes(img, angles, shifts, REQ, gt_dev=gt, adam_starts=starts)
    truth = gt.cpu().numpy()
    for t in ("aug", "max", "mean"):
        s, smax = res["scores"][t]
        assert (smax is not None) == (mode == "slice_max")
        # (a) the scores are the class-set path's: their thresholds are its masks
        masks = ops.threshold_classes(s, REQ, th_mask=smax) if smax is not None else ops.threshold_classes(s, REQ, th_factor=TH)
        assert torch.equal(masks, torch.stack([ref[c][t] for c in REQ])), t
        # (b) the label map is the rule applied to them
        want = fuse_numpy(s.cpu().numpy(), REQ, TH, smax.cpu().numpy() if smax is not None else None)
        assert torch.equal(res[t].cpu(), torch.from_numpy(want)), t
        assert np.array_equal(res["counts"][t], counts_numpy(truth, want)), t
    # (c) the standard label map is the sum of the standard masks
    assert torch.equal(res["standard"], torch.stack([ref[c]["standard"] for c in REQ]).sum(dim=0).to(torch.int32))
    assert np.array_equal(res["counts"]["standard"], counts_numpy(truth, res["standard"].cpu().numpy()))
    for key in KEYS:
        m = mean_iou_from_counts(res["counts"][key])
        assert res["Mean_IOU"][key] == m or (np.isnan(m) and np.isnan(res["Mean_IOU"][key]))
    if mode == "argmax":                      # not one class against nothing
        assert len(set(int(v) for v in torch.unique(res["aug"]).cpu()) - {0}) >= 2
        assert 0.0 < res["Mean_IOU"]["aug"] < 1.0


# Pruning rests on "a zero stack stays zero": zero data, zero gradient, zero step.  It holds for every update rule of
# asr_sr_config that was tried here (Adam / AMSGrad, Adagrad with its non-zero initial accumulator) and for both priors.
@pytest.mark.parametrize("kind,use_btv", [("adam", False), ("adagrad", False), ("adam", True)])
def test_pruning_changes_no_bit_and_no_counter(small, kind, use_btv):
    from asr_amd.pipeline import HotPath
    model, img, gt, angles, shifts = small
    won = _winners(model, img, angles, shifts)
    winning, losing = [c for c in REQ if c in won], [c for c in REQ if c not in won]
    assert len(winning) >= 2 and len(losing) >= 2, (winning, losing)           # the bias shifts did their work
    out = {}
    for prune in (True, False):
        sr = _sr(kind, 6, 5, (16, 16), (64, 64), use_btv)
        sr.optimizer.optimizer.iterations = 40
        res = HotPath(model, sr, mode="argmax", th_factor=TH, batch_size=4).run_image_labels(
            img, angles, shifts, REQ, gt_dev=gt, prune=prune)
        out[prune] = (res, sr.optimizer.optimizer.iterations)
    (a, it_a), (b, it_b) = out[True], out[False]
    assert a["solved_ids"] == winning and b["solved_ids"] == REQ               # pruned exactly the classes that never win
    assert it_a == it_b == 40 + len(REQ) * 5                                    # the counter passes every requested class
    for key in KEYS:
        assert torch.equal(a[key], b[key]), key
        assert np.array_equal(a["counts"][key], b["counts"][key]), key
    assert len(set(int(v) for v in torch.unique(a["aug"]).cpu()) - {0}) >= 2


def test_pruning_does_nothing_in_the_slice_modes_and_no_class_left_is_legal(small):
    from asr_amd.pipeline import HotPath
    model, img, gt, angles, shifts = small
    sr = _sr("adam", 6, 5, (16, 16), (64, 64), False)
    res = HotPath(model, sr, mode="slice", th_factor=TH, batch_size=6).run_image_labels(img, angles, shifts, REQ, prune=True,
                                                                                       adam_starts={c: 0 for c in REQ})
    assert res["solved_ids"] == REQ and "counts" not in res
    won = _winners(model, img, angles, shifts)
    none = [c for c in (5, 12, 17) if c not in won]
    assert len(none) >= 2
    sr.optimizer.optimizer.iterations = 9
    res = HotPath(model, sr, mode="argmax", th_factor=TH, batch_size=6).run_image_labels(img, angles, shifts, none, gt_dev=gt)
    assert res["solved_ids"] == [] and sr.optimizer.optimizer.iterations == 9 + len(none) * 5
    for t in ("aug", "max", "mean"):
        assert int(res[t].abs().sum()) == 0
        assert np.array_equal(res["counts"][t], counts_numpy(gt.cpu().numpy(), np.zeros((64, 64), np.int32)))


# ---- scripts/validate_labelmap.py ------------------------------------------------------------------------------------------
SCRIPT = os.path.join(ROOT, "scripts", "validate_labelmap.py")
N_AUG, ITERS, ANGLE, SHIFT = 8, 10, 0.15, 20
BOXES = {8: (60, 300, 80, 420), 12: (320, 480, 100, 400)}


def _dataset(root):
    """The golden cat image and its mirror image, with box ground truths (a void edge each) of classes 8 and 12."""
    from PIL import Image
    img_dir, gt_dir = os.path.join(root, "images"), os.path.join(root, "gt")
    os.makedirs(img_dir)
    os.makedirs(gt_dir)
    cat = Image.open(os.path.join(GOLDEN, "test_cat.jpg")).convert("RGB").resize((512, 512))
    lab = np.zeros((512, 512), np.uint8)
    for c, (y0, y1, x0, x1) in BOXES.items():
        lab[y0:y1, x0:x1] = c
        lab[y0:y0 + 3, x0:x1] = 255
    for g, flip in enumerate((False, True)):
        im = cat.transpose(Image.FLIP_LEFT_RIGHT) if flip else cat
        im.save(os.path.join(img_dir, f"{g}.jpg"), quality=95)
        Image.fromarray(lab[:, ::-1].copy() if flip else lab, mode="L").save(os.path.join(gt_dir, f"{g}.png"))
    return img_dir, gt_dir


def _weights(root, dev):
    from asr_amd import ops, weights as W
    from asr_amd.model import DeeplabModel
    from asr_amd.utils import load_image
    w = W.make_synthetic_weights(1234, 21)
    model = DeeplabModel(w, (512, 512, 3), 21, False, None)
    img = ops.to_device(load_image(os.path.join(root, "images", "0.jpg"), image_size=(512, 512), normalize=True), device=dev)
    for c, delta in _shift_classes(model, img, [3, 8, 12], fraction=0.2).items():
        w = shifted_weights(w, c, delta)
    path = os.path.join(root, "weights.npz")
    np.savez(path, **{k: np.asarray(v) for k, v in w.items()})
    del model
    return path


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(cmd, env=None):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def test_validate_labelmap_script_on_the_cat(dev, tmp_path):
    from PIL import Image
    root = str(tmp_path)
    img_dir, gt_dir = _dataset(root)
    weights = _weights(root, dev)
    args = lambda out, save: ["--images", img_dir, "--gt", gt_dir, "--num_aug", str(N_AUG), "--num_iter", str(ITERS), "--mode",
                              "argmax", "--angle_max", str(ANGLE), "--shift_max", str(SHIFT), "--th_factor", str(TH),
                              "--weights", weights, "--out", out, "--save_dir", save]
    out1, save1 = os.path.join(root, "one.csv"), os.path.join(root, "maps1")
    _run([sys.executable, SCRIPT] + args(out1, save1))
    with open(out1, newline="") as fh:
        rows = list(csv.reader(fh))
    assert rows[0] == ["Name", "standard_iou", "aug_iou", "max_iou", "mean_iou", "n"]
    assert [r[0] for r in rows[1:]] == ["Label 0", "Label 8", "Label 12", "dataset_mIoU", "mean_image_mIoU"]
    # the dataset mean again, from the saved PNGs and the ground-truth PNGs with numpy alone
    gts = [np.asarray(Image.open(os.path.join(gt_dir, f"{g}.png"))).astype(np.int32) for g in range(2)]
    for j, key in enumerate(KEYS):
        total = sum(counts_numpy(gts[g], np.asarray(Image.open(os.path.join(save1, f"{g}_{key}.png"))).astype(np.int32))
                    for g in range(2))
        ious = [total[2, l] / (total[0, l] + total[1, l] - total[2, l]) for l in (0, 8, 12)]
        assert float(rows[4][1 + j]) == float(np.mean(ious)), key
        for r, v in zip(rows[1:4], ious):
            assert float(r[1 + j]) == float(v), (key, r[0])
    aug = [np.asarray(Image.open(os.path.join(save1, f"{g}_aug.png"))) for g in range(2)]
    assert all(len(set(np.unique(a)) - {0}) >= 2 for a in aug)                   # label maps with several classes in them
    assert 0.0 < float(rows[4][2]) < 1.0
    # 2 ranks (gloo collectives) on the one GPU: the same bytes
    out2, save2 = os.path.join(root, "two.csv"), os.path.join(root, "maps2")
    env = dict(os.environ, ASR_DIST_BACKEND="gloo")
    _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
          "--master-port", str(_free_port()), SCRIPT] + args(out2, save2), env=env)
    with open(out1, "rb") as a, open(out2, "rb") as b:
        assert a.read() == b.read()
