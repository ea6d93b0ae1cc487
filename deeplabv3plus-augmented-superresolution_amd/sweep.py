"""Offline hyper-parameter and threshold sweeps over precomputed SR data: the reference's sweep_script.py (run by a
wandb agent over configs/sweep_configs/*.yaml) and threshold_tests.py, without the wandb service.

A sweep file is read in the wandb format (JSON always, YAML through PyYAML when it is importable) and expanded into
configurations here (``grid`` / ``random``; ``bayes`` needs the service and runs as ``random``).  ``sweep_precomputed``
then evaluates every configuration over the interchange files of a class, loading and uploading each file ONCE for all
configurations: the standard, max-SR and mean-SR IoUs depend on no swept parameter and are computed once per image;
only the aug-SR solve and its threshold run per configuration.  Every row equals what ``evaluation.evaluate_precomputed``
gives for that configuration alone in a fresh process seeded like the reference's (np.random.seed(1234)).
"""
from __future__ import annotations

import csv
import itertools
import json
import math
import os
import sys

import numpy as np

from . import distributed as D

SEED = 1234

# sweep_script.py:51-73 (num_aug / num_samples are command-line settings here, not hyper-parameters)
HYPER_DEFAULTS = {
    "lambda_df": 1, "lambda_tv": 4.75, "lambda_L2": 0.11, "lambda_L1": 0.0, "num_iter": 300, "use_BTV": False,
    "copy_dropout": 0.0, "optimizer": "adam", "learning_rate": 1e-3, "beta_1": 0.9, "beta_2": 0.999, "epsilon": 1e-7,
    "amsgrad": False, "initial_accumulator_value": 0.1, "momentum": 0.6, "nesterov": False, "lr_scheduler": True,
    "decay_steps": 50, "decay_rate": 0.5,
}

# threshold_tests.py:48-70; its lambdas go through normalize_coefficients before use (:81-87)
THRESHOLD_DEFAULTS = {
    "lambda_df": 1.0, "lambda_tv": 0.84, "lambda_L2": 0.047, "lambda_L1": 0.0065, "num_iter": 300, "copy_dropout": 0.2,
    "use_BTV": False, "optimizer": "adam", "learning_rate": 1e-1, "beta_1": 0.9, "beta_2": 0.999, "epsilon": 1e-7,
    "amsgrad": False, "initial_accumulator_value": 0.1, "nesterov": True, "momentum": 0.2, "lr_scheduler": True,
    "decay_steps": 100, "decay_rate": 0.65,
}

# threshold_tests.py:105
TH_FACTORS = [round(v, 2) for v in np.arange(0.1, 0.95, step=0.05)]

# the keys of sweep_script.py's wandb.log -> distributed.IOU_FIELDS
METRICS = {
    "standard_iou_single": "standard_single", "standard_iou_multiple": "standard_bg", "aug_iou_single": "aug_single",
    "aug_iou_multiple": "aug_bg", "max_iou": "max", "mean_iou": "mean",
}

DISTRIBUTIONS = ("uniform", "q_uniform", "int_uniform", "log_uniform_values")


class SweepSpecError(ValueError):
    """A sweep file this driver cannot run."""


# ---- sweep file -------------------------------------------------------------------------------------------------
def load_spec(path):
    """A wandb sweep file -> dict.  ``.yaml`` / ``.yml`` need PyYAML; anything else is read as JSON."""
    with open(path) as fh:
        text = fh.read()
    if str(path).endswith((".yaml", ".yml")):
        try:
            import yaml
        except ImportError:
            raise SweepSpecError(f"{path}: reading YAML needs PyYAML, which is not installed; write the same sweep as "
                                 "JSON (the same keys and nesting) and pass the .json file") from None
        spec = yaml.safe_load(text)
    else:
        spec = json.loads(text)
    if not isinstance(spec, dict):
        raise SweepSpecError(f"{path}: a sweep file is a mapping with 'method' and 'parameters'")
    return spec


def _number(v):
    """YAML 1.1 reads ``1e-3`` (no dot) as a string; wandb reads it as a number, and so does this driver."""
    if isinstance(v, str):
        for cast in (int, float):
            try:
                return cast(v)
            except ValueError:
                pass
    return v


def _check_names(params):
    unknown = sorted(set(params) - set(HYPER_DEFAULTS))
    if unknown:
        raise SweepSpecError(f"unknown sweep parameter(s) {unknown}; allowed: {', '.join(HYPER_DEFAULTS)}")


def _is_range(p):
    return "min" in p or "max" in p or "distribution" in p


def _choices(name, p):
    if "value" in p:
        return [_number(p["value"])]
    if "values" in p:
        vals = [_number(v) for v in p["values"]]
        if not vals:
            raise SweepSpecError(f"parameter {name!r}: empty 'values'")
        return vals
    raise SweepSpecError(f"parameter {name!r}: needs 'value', 'values' or 'min'/'max'")


def _draw(name, p, rng):
    if not _is_range(p):
        vals = _choices(name, p)
        return vals[int(rng.integers(len(vals)))] if len(vals) > 1 else vals[0]
    if "min" not in p or "max" not in p:
        raise SweepSpecError(f"parameter {name!r}: a range needs both 'min' and 'max'")
    lo, hi = _number(p["min"]), _number(p["max"])
    dist = p.get("distribution")
    if dist is None:
        dist = "int_uniform" if isinstance(lo, int) and isinstance(hi, int) else "uniform"
    if dist not in DISTRIBUTIONS:
        raise SweepSpecError(f"parameter {name!r}: distribution {dist!r} is not one of {DISTRIBUTIONS}")
    if lo > hi:
        raise SweepSpecError(f"parameter {name!r}: min {lo} > max {hi}")
    if dist == "uniform":
        return float(rng.uniform(lo, hi))
    if dist == "int_uniform":
        return int(rng.integers(int(lo), int(hi) + 1))
    if dist == "log_uniform_values":
        if lo <= 0:
            raise SweepSpecError(f"parameter {name!r}: log_uniform_values needs min > 0")
        return float(math.exp(rng.uniform(math.log(lo), math.log(hi))))
    q = _number(p.get("q", 1.0))
    if not q > 0:
        raise SweepSpecError(f"parameter {name!r}: q must be > 0")
    # a multiple of q inside [min, max], each multiple equally likely
    k_lo, k_hi = math.ceil(lo / q - 1e-9), math.floor(hi / q + 1e-9)
    if k_lo > k_hi:
        raise SweepSpecError(f"parameter {name!r}: no multiple of q={q} lies in [{lo}, {hi}]")
    k = int(rng.integers(k_lo, k_hi + 1))
    if all(isinstance(v, int) for v in (lo, hi, q)):
        return k * q
    return float(min(max(round(k * q, 12), lo), hi))


def expand(spec, count=None, seed=None):
    """The configurations of a sweep, each a full hyper-parameter dict (unswept keys take HYPER_DEFAULTS).

    grid: the cartesian product of the ``value`` / ``values`` parameters, the first parameter varying slowest.
    random: ``count`` draws from a numpy Generator seeded with ``seed`` (the argument, else the spec's ``seed``, else 1234).
    bayes: run as random, with a note on stderr (Bayesian search needs the wandb service)."""
    params = spec.get("parameters") or {}
    if not isinstance(params, dict):
        raise SweepSpecError("'parameters' must be a mapping of name -> {value | values | min/max ...}")
    _check_names(params)
    method = spec.get("method", "grid")
    if method == "grid":
        ranged = [n for n, p in params.items() if _is_range(p)]
        if ranged:
            raise SweepSpecError(f"method 'grid' takes 'value'/'values' only; continuous range(s): {ranged}")
        names = list(params)
        grids = [_choices(n, params[n]) for n in names]
        out = [dict(zip(names, combo)) for combo in itertools.product(*grids)]
        if count is not None:
            out = out[:int(count)]
    elif method in ("random", "bayes"):
        if method == "bayes":
            print("sweep: method 'bayes' needs the wandb service; running it as 'random'", file=sys.stderr)
        count = spec.get("count") if count is None else count
        if count is None:
            raise SweepSpecError(f"method {method!r} needs a 'count' (in the file or on the command line)")
        seed = spec.get("seed", SEED) if seed is None else seed
        rng = np.random.default_rng(int(seed))
        out = [{n: _draw(n, p, rng) for n, p in params.items()} for _ in range(int(count))]
    else:
        raise SweepSpecError(f"unknown method {method!r} (grid, random, bayes)")
    return [dict(HYPER_DEFAULTS, **c) for c in out]


def metric_of(spec):
    """(IOU_FIELDS column index, goal) of the spec's ``metric``; without one, aug_iou_single / maximize."""
    m = spec.get("metric") or {}
    name = m.get("name", "aug_iou_single")
    if name not in METRICS:
        raise SweepSpecError(f"metric {name!r} is not one of {', '.join(METRICS)}")
    goal = m.get("goal", "maximize")
    if goal not in ("maximize", "minimize"):
        raise SweepSpecError(f"metric goal {goal!r} is not 'maximize' or 'minimize'")
    return D.IOU_FIELDS.index(METRICS[name]), goal


def best_index(values, goal):
    """Index of the best finite value (ties: the lowest index); None when none is finite."""
    v = np.asarray(values, dtype=np.float64)
    ok = np.flatnonzero(np.isfinite(v))
    if not len(ok):
        return None
    sub = v[ok] if goal == "maximize" else -v[ok]
    return int(ok[int(np.argmax(sub))])


# ---- CSV output -------------------------------------------------------------------------------------------------
def _cell(v):
    if isinstance(v, float) and math.isnan(v):
        return ""                                    # DataFrame.to_csv writes NaN as an empty field
    return v


def write_threshold_csv(path, th_values, ious):
    """threshold_tests.py's ``pd.DataFrame(data_list).to_csv(path)`` layout: header ``,Th_Value,IoU``, integer index."""
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(["", "Th_Value", "IoU"])
        for i, (t, v) in enumerate(zip(th_values, ious)):
            w.writerow([i, _cell(float(t)), _cell(float(v))])


def write_sweep_csv(path, configs, means, n_valid):
    """One row per configuration: index, every hyper-parameter, the six means (sweep_script.py's wandb.log names),
    n_valid."""
    names = list(HYPER_DEFAULTS)
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(["index"] + names + list(METRICS) + ["n_valid"])
        for i, (c, m) in enumerate(zip(configs, means)):
            w.writerow([i] + [c[n] for n in names] + [_cell(float(m[METRICS[k]])) for k in METRICS] + [int(n_valid)])


# ---- evaluation -------------------------------------------------------------------------------------------------
def build_solver(config, num_aug, feature_size=(128, 128), img_size=(512, 512)):
    """The Optimizer / Superresolution pair sweep_script.py:86-92 builds from a configuration."""
    from .superresolution_scripts.optimizer import Optimizer
    from .superresolution_scripts.superresolution import Superresolution
    c = dict(HYPER_DEFAULTS, **config)
    opt = Optimizer(optimizer=c["optimizer"], learning_rate=c["learning_rate"], epsilon=c["epsilon"], beta_1=c["beta_1"],
                    beta_2=c["beta_2"], amsgrad=c["amsgrad"], initial_accumulator_value=c["initial_accumulator_value"],
                    momentum=c["momentum"], nesterov=c["nesterov"], lr_scheduler=c["lr_scheduler"],
                    decay_steps=c["decay_steps"], decay_rate=c["decay_rate"])
    return Superresolution(lambda_df=c["lambda_df"], lambda_tv=c["lambda_tv"], lambda_L2=c["lambda_L2"],
                           lambda_L1=c["lambda_L1"], num_iter=int(c["num_iter"]), num_aug=num_aug, optimizer=opt,
                           use_BTV=bool(c["use_BTV"]), copy_dropout=c["copy_dropout"], feature_size=tuple(feature_size),
                           output_size=tuple(img_size))


def _seed_drop_mask(sr, seed):
    """The copy_dropout mask a fresh process seeded with ``seed`` draws on its first solve (np.random.shuffle on the
    global stream, superresolution.py:47-50), drawn here from its own RandomState so that it does not depend on how many
    configurations ran before."""
    n_drop = int(sr.num_aug * sr.copy_dropout)
    if n_drop:
        mask = np.full(sr.num_aug, fill_value=True)
        mask[:n_drop] = False
        np.random.RandomState(seed).shuffle(mask)
        sr._drop_masks[n_drop] = mask


def _probe_by_loading(path, num_aug):
    """(valid, solves) as the reference's loop decides it: the full load_SR_data either succeeds or the file is skipped
    (a file whose headers are intact but whose data is short is invalid, which a header probe cannot see).  The data is
    dropped; the solve loop loads each valid file again when its turn comes."""
    from .superresolution_scripts.superres_utils import load_SR_data
    try:
        _cm, max_masks, _a, _s, _f = load_SR_data(path, num_aug=num_aug)
    except Exception:
        return False, 0
    return True, 2 if max_masks is not None else 1


def sweep_precomputed(configs, paths, gt_dir, standard_dir=None, num_aug=100, class_id=8, th_factor=0.65, th_factors=None,
                      img_size=(512, 512), feature_size=(128, 128), rank=0, world=1, seed=SEED):
    """Evaluate C hyper-parameter configurations over the interchange files ``paths``.

    Returns ``(table [C, files, 6], thr [C, files, K] or None, valid [files])`` on every rank.  Row ``table[c]`` is bitwise
    what ``evaluation.evaluate_precomputed`` returns for configuration c alone, run in a fresh process that seeded
    np.random with ``seed``: each configuration keeps its own optimizer step counter (set per image to num_iter_c x the
    solves of the valid files before it, two for slice_max files) and its own copy_dropout mask.  ``thr[c, f, k]`` is
    threshold_tests.py's number: the aug-SR target of configuration c thresholded at ``th_factors[k]`` with no th_mask
    (also for slice_max files), scored single-class; all K factors of all C targets of an image come from one launch.

    Files are sharded with ``distributed.shard_indices``; validity and solve counts are all-gathered before any solve and
    the per-configuration rows are all-gathered once at the end.  An invalid file gets NaN rows, runs no solve and
    advances no counter."""
    import torch
    from . import _lib, ops
    from .superresolution_scripts.superres_utils import load_SR_data
    from .superresolution_scripts.superresolution import Superresolution, _stack_copies
    from .utils import _as_label_tensor, compute_IoU, iou_from_counts, load_image

    configs = [dict(HYPER_DEFAULTS, **c) for c in configs]
    n_cfg, n_files, n_io = len(configs), len(paths), len(D.IOU_FIELDS)
    k_th = 0 if th_factors is None else len(th_factors)
    if th_factors is not None and not 1 <= k_th <= ops.MAX_SWEEP_FACTORS:
        raise ValueError(f"th_factors: {k_th} factors (1..{ops.MAX_SWEEP_FACTORS})")
    solvers = [build_solver(c, num_aug, feature_size, img_size) for c in configs]
    for sr in solvers:
        _seed_drop_mask(sr, seed)

    mine = D.shard_indices(n_files, rank, world)
    flags = []
    for g in mine:
        ok, n_solves = _probe_by_loading(paths[g], num_aug)
        if not ok:
            print(f"File: {paths[g]} is invalid, skipping...")
        flags.append([1.0 if ok else 0.0, float(n_solves)])
    status = D.all_gather_rows(mine, flags, n_files, 2)
    valid = np.nan_to_num(status[:, 0]) > 0.5
    solves = np.where(valid, np.nan_to_num(status[:, 1]), 0.0).astype(np.int64)
    before = np.concatenate([[0], np.cumsum(solves)[:-1]]) if n_files else np.zeros(0, np.int64)

    width = n_cfg * (n_io + k_th)
    records = []
    dev = _lib.require_gpu() if any(valid[g] for g in mine) else None
    for g in mine:
        if not valid[g]:
            records.append([np.nan] * width)
            continue
        class_masks, max_masks, angles, shifts, filename = load_SR_data(paths[g], num_aug=num_aug)
        true_mask = load_image(os.path.join(gt_dir, f"{filename}.png"), image_size=img_size, normalize=False, is_png=True,
                               resize_method="nearest")
        truth = _as_label_tensor(true_mask, dev)
        y = _stack_copies(class_masks, dev)[None]                    # uploaded once for every configuration
        ym = _stack_copies(max_masks, dev)[None] if max_masks is not None and len(max_masks) == len(class_masks) else None
        a, s = Superresolution._batchify(angles, shifts)

        def iou_pair(pred):
            return [compute_IoU(truth, pred, img_size=img_size, class_id=class_id),
                    compute_IoU(truth, pred, img_size=img_size, class_id=class_id, include_bg=True)]

        def to_mask(sr, run):
            """compute_SR's threshold: against the max map's result in slice_max files, else th_factor * max."""
            target = run(sr, y)
            if ym is not None:
                return target, ops.threshold(target, class_id, th_mask=run(sr, ym))
            return target, ops.threshold(target, class_id, th_factor=th_factor)

        # standard / max-SR / mean-SR: no swept parameter enters them (compute_SR "max" / "mean", SR_single_class.py:103-120)
        std = [np.nan, np.nan]
        if standard_dir:
            sm = load_image(os.path.join(standard_dir, f"{filename}.png"), image_size=img_size, normalize=False, is_png=True,
                            resize_method="nearest")
            std = iou_pair(sm)
        shared = {}
        for mode in ("max", "mean"):
            _t, mask = to_mask(solvers[0], lambda sr, stack, m=mode: sr.realign_batch(stack, a, s, m)[0].contiguous())
            shared[mode] = compute_IoU(truth, mask, img_size=img_size, class_id=class_id)

        rows, targets = [], []
        for sr in solvers:
            # the global step counter the configuration's own sequential run would have reached (evaluation.py)
            sr.optimizer.optimizer.iterations = int(before[g]) * sr.num_iter
            target, mask = to_mask(sr, lambda sr_, stack: sr_.augmented_superresolution_batch(stack, a, s)[0][0].contiguous())
            rows.append(std + iou_pair(mask) + [shared["max"], shared["mean"]])
            targets.append(target)
        if k_th:
            counts = ops.threshold_sweep_iou_counts(torch.stack(targets), truth, th_factors, class_id).cpu().numpy()
            thr = [[iou_from_counts(ck, False) for ck in cc] for cc in counts]
        else:
            thr = [[] for _ in solvers]
        records.append([v for row in rows for v in row] + [v for t in thr for v in t])

    full = D.all_gather_rows(mine, records, n_files, width)             # [files, C*6 + C*K]
    table = full[:, :n_cfg * n_io].reshape(n_files, n_cfg, n_io).transpose(1, 0, 2).copy()
    thr = full[:, n_cfg * n_io:].reshape(n_files, n_cfg, k_th).transpose(1, 0, 2).copy() if k_th else None
    return table, thr, valid


def means_per_config(table, valid):
    """The six means over the valid images of every configuration row (evaluation.mean_over_valid)."""
    from .evaluation import mean_over_valid
    return [mean_over_valid(t, valid) for t in table]
