"""The offline sweep over precomputed SR data (asr_amd.sweep.sweep_precomputed) against one evaluate_precomputed run per
configuration, each in a fresh seeded process -- what a wandb agent run of the reference's sweep_script.py amounts to --
and the two sweep scripts run end to end."""
import csv
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

NUM_AUG = 10
CLASS_ID = 8

CONFIGS = [
    dict(lambda_tv=0.3, lambda_L2=0.7, lambda_L1=0.0, num_iter=20, learning_rate=1e-3, amsgrad=True, decay_steps=60,
         decay_rate=0.3),
    dict(lambda_tv=4.75, lambda_L2=0.11, lambda_L1=0.01, num_iter=25, learning_rate=1e-2, decay_steps=7, decay_rate=0.5),
    dict(lambda_tv=0.84, lambda_L2=0.047, lambda_L1=0.0065, num_iter=15, learning_rate=1e-1, copy_dropout=0.2,
         decay_steps=10, decay_rate=0.65),
]

# one evaluate_precomputed run of one configuration in a fresh process, seeded like the reference's scripts
EVAL_ONE = r'''
import json, sys
import numpy as np
np.random.seed(1234)
sys.path.insert(0, sys.argv[1])
import torch
torch.cuda.set_device(0)
from asr_amd.evaluation import evaluate_precomputed, interchange_files
from asr_amd.superresolution_scripts.optimizer import Optimizer
from asr_amd.superresolution_scripts.superresolution import Superresolution
from asr_amd.sweep import HYPER_DEFAULTS
a = json.loads(sys.argv[2])
c = dict(HYPER_DEFAULTS, **a["config"])
opt = Optimizer(optimizer=c["optimizer"], learning_rate=c["learning_rate"], epsilon=c["epsilon"], beta_1=c["beta_1"],
                beta_2=c["beta_2"], amsgrad=c["amsgrad"], initial_accumulator_value=c["initial_accumulator_value"],
                momentum=c["momentum"], nesterov=c["nesterov"], lr_scheduler=c["lr_scheduler"], decay_steps=c["decay_steps"],
                decay_rate=c["decay_rate"])
sr = Superresolution(lambda_df=c["lambda_df"], lambda_tv=c["lambda_tv"], lambda_L2=c["lambda_L2"], lambda_L1=c["lambda_L1"],
                     num_iter=c["num_iter"], num_aug=a["num_aug"], optimizer=opt, use_BTV=c["use_BTV"],
                     copy_dropout=c["copy_dropout"], feature_size=tuple(a["feature_size"]), output_size=tuple(a["img_size"]))
table, valid = evaluate_precomputed(sr, interchange_files(a["data"]), a["gt"], a["standard"], num_aug=a["num_aug"],
                                    class_id=a["class_id"], th_factor=a["th_factor"], img_size=tuple(a["img_size"]),
                                    out_dir=a["out_dir"])
np.save(a["dest"], table)
'''


def _run(args, cwd, timeout=900):
    r = subprocess.run([sys.executable] + args, cwd=cwd, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def _save_png(path, arr):
    from PIL import Image
    Image.fromarray(np.asarray(arr, dtype=np.uint8)).save(path)


def _make_data(root, gt_dir, std_dir, files, feat, out):
    """Interchange files (argmax / slice_max) of a blob that moves a little between copies, plus ground-truth and
    standard-output PNGs at the output size (with some void pixels)."""
    from asr_amd.superresolution_scripts.superres_utils import save_SR_data
    for d in (root, gt_dir, std_dir):
        os.makedirs(d, exist_ok=True)
    yy, xx = np.mgrid[0:feat, 0:feat].astype(np.float32)
    paths = {}
    for name, mode in files:
        rng = np.random.default_rng(42 + int(name))                # per file: the same file whatever else is written
        angles = rng.uniform(-0.1, 0.1, NUM_AUG).astype(np.float32)
        shifts = rng.uniform(-3, 3, (NUM_AUG, 2)).astype(np.float32)
        r = feat * rng.uniform(0.2, 0.3)
        blobs = np.stack([((yy - feat / 2 - rng.uniform(-2, 2)) ** 2 + (xx - feat / 2 - rng.uniform(-2, 2)) ** 2 < r * r)
                          for _ in range(NUM_AUG)]).astype(np.float32)
        noise = rng.standard_normal(blobs.shape).astype(np.float32)
        if mode == "argmax":
            cm, mm = CLASS_ID * blobs, None
        else:
            cm, mm = 3.0 * blobs + 0.5 * noise, 2.0 * (1.0 - blobs) + 0.5 * noise[:, ::-1]
        paths[name] = save_SR_data(os.path.join(root, name), cm[..., None], None if mm is None else mm[..., None], angles,
                                   shifts, name, mode, 0.15, 80)
        oy, ox = np.mgrid[0:out, 0:out]
        rr = out * 0.26
        gt = np.where((oy - out / 2) ** 2 + (ox - out / 2) ** 2 < rr * rr, CLASS_ID, 0)
        gt[:2] = 255
        _save_png(os.path.join(gt_dir, f"{name}.png"), gt)
        std = np.where((oy - out / 2 - 3) ** 2 + (ox - out / 2) ** 2 < rr * rr, CLASS_ID, 0)
        _save_png(os.path.join(std_dir, f"{name}.png"), std)
    return paths


def _truncate(path, nbytes):
    size = os.path.getsize(path)
    with open(path, "r+b") as fh:
        fh.truncate(size - nbytes)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    base = tmp_path_factory.mktemp("sweep")
    gt, std = str(base / "gt"), str(base / "standard")
    full, clean = str(base / "full"), str(base / "clean")
    _make_data(full, gt, std, [("0", "argmax"), ("1", "argmax"), ("2", "slice_max")], 32, 128)
    _make_data(clean, str(base / "gt_unused"), str(base / "std_unused"), [("1", "argmax"), ("2", "slice_max")], 32, 128)
    # the copies of 1 and 2 are byte for byte those in `full`
    import filecmp
    for n in ("1", "2"):
        assert filecmp.cmp(os.path.join(full, f"{n}.hdf5"), os.path.join(clean, f"{n}.hdf5"), shallow=False)
    _truncate(os.path.join(full, "0.hdf5"), 24)                   # intact headers, short data: sorts first
    return dict(base=base, gt=gt, std=std, full=full, clean=clean)


def test_sweep_rows_equal_fresh_process_runs(dev, data):
    from asr_amd import sweep as SW
    from asr_amd.evaluation import interchange_files
    from asr_amd.superresolution_scripts.superres_utils import probe_SR_data
    paths = interchange_files(data["full"])
    assert [os.path.basename(p) for p in paths] == ["0.hdf5", "1.hdf5", "2.hdf5"]
    assert probe_SR_data(paths[0], num_aug=NUM_AUG)[0]            # the header probe alone would accept the truncated file
    factors = SW.TH_FACTORS
    table, thr, valid = SW.sweep_precomputed(CONFIGS, paths, data["gt"], data["std"], num_aug=NUM_AUG, class_id=CLASS_ID,
                                             th_factor=0.65, th_factors=factors, img_size=(128, 128), feature_size=(32, 32))
    assert table.shape == (3, 3, 6) and thr.shape == (3, 3, 17)
    assert list(valid) == [False, True, True]
    assert np.isnan(table[:, 0]).all() and np.isnan(thr[:, 0]).all()
    assert not np.isnan(table[:, 1:]).any() and (table[:, 1:, 2] > 0.1).all()         # non-trivial masks
    assert len({table[c, 2, 2] for c in range(3)}) > 1                              # the configurations differ
    k65 = factors.index(0.65)
    for c, cfg in enumerate(CONFIGS):
        dest = str(data["base"] / f"eval_{c}.npy")
        args = dict(config=cfg, num_aug=NUM_AUG, feature_size=[32, 32], img_size=[128, 128], data=data["clean"],
                    gt=data["gt"], standard=data["std"], class_id=CLASS_ID, th_factor=0.65, dest=dest,
                    out_dir=str(data["base"] / f"out_{c}"))
        _run(["-c", EVAL_ONE, ROOT, json.dumps(args)], ROOT)
        ref = np.load(dest)
        assert ref.shape == (2, 6)
        assert np.array_equal(table[c, 1:], ref, equal_nan=True), (c, table[c, 1:], ref)
        # the threshold table at 0.65 is the argmax file's aug_single (no th_mask there either)
        assert thr[c, 1, k65] == ref[0, 2]
    # the factors really change the score
    assert len(set(thr[0, 1])) > 2


def test_sweep_script_end_to_end(dev, data, tmp_path):
    spec = {"method": "grid", "metric": {"name": "aug_iou_single", "goal": "maximize"},
            "parameters": {"lambda_tv": {"values": [0.3, 4.75]}, "num_iter": {"value": 20},
                           "learning_rate": {"values": [1e-3, 1e-2]}}}
    (tmp_path / "sweep.json").write_text(json.dumps(spec))
    out_csv = tmp_path / "sweep.csv"
    out = _run([os.path.join(ROOT, "scripts", "sweep_script.py"), "--sweep", str(tmp_path / "sweep.json"), "--data",
                data["full"], "--gt", data["gt"], "--standard", data["std"], "--num_aug", str(NUM_AUG), "--feature_size", "32",
                "--out", str(out_csv)], str(tmp_path))
    assert "is invalid, skipping" in out and "Best configuration: index" in out
    rows = list(csv.reader(open(out_csv)))
    from asr_amd import sweep as SW
    assert rows[0] == ["index"] + list(SW.HYPER_DEFAULTS) + list(SW.METRICS) + ["n_valid"]
    assert len(rows) == 5 and [r[0] for r in rows[1:]] == ["0", "1", "2", "3"]
    assert all(r[-1] == "2" for r in rows[1:])
    col = rows[0].index("aug_iou_single")
    vals = [float(r[col]) for r in rows[1:]]
    best = int(np.argmax(vals))
    assert f"Best configuration: index {best}," in out


def test_threshold_tests_script_end_to_end(dev, data, tmp_path):
    out = _run([os.path.join(ROOT, "scripts", "threshold_tests.py"), "--data", data["full"], "--gt", data["gt"],
                "--standard", data["std"], "--num_aug", str(NUM_AUG), "--num_samples", "3", "--feature_size", "32",
                "--mode", "argmax", "--out", str(tmp_path / "th")], str(tmp_path))
    assert "Best record: Th_Value" in out and "Standard IoU: " in out and "Standard IoU: nan" not in out
    lines = (tmp_path / "th" / "th_argmax_3.csv").read_text().splitlines()
    assert lines[0] == ",Th_Value,IoU" and len(lines) == 18
    rows = [l.split(",") for l in lines[1:]]
    assert [int(r[0]) for r in rows] == list(range(17))
    assert [float(r[1]) for r in rows] == [round(v, 2) for v in np.arange(0.1, 0.95, 0.05)]
    ious = [float(r[2]) for r in rows]
    assert all(0.0 <= v <= 1.0 for v in ious) and len(set(ious)) > 1
