"""The per-image evaluation loop of the reference's SR_single_class.py:72-134: interchange file -> augmented / max /
mean SR -> six IoUs per image -> means over the VALID images.  Images are sharded over the ranks of the node
(asr_amd.distributed), the per-image records are all-gathered once at the end."""
from __future__ import annotations

import os

import numpy as np
import torch

from . import distributed as D, ops
from .label_record import counts_name, label_fields, label_layout
from .superresolution_scripts.augmentation_utils import _image_to_device
from .superresolution_scripts.superres_utils import DATA_EXTS, EXTRA_SR_TYPES, compute_SR, load_SR_data, probe_SR_data
from .utils import compute_IoU, load_image



def interchange_files(root_dir):
    """Every interchange file under ``root_dir`` in ONE order shared by all ranks: by the integer value of the file stem
    (VOC-style ids, the order SR_single_class.py:72 asks for with sort=True), names that are not integers after them in
    lexical order.  os.walk order is file-system dependent, so it is never used as the order."""
    found = []
    for folder, _dirs, files in os.walk(root_dir):
        found += [os.path.join(folder, f) for f in files if f.endswith(DATA_EXTS)]

    def key(path):
        stem = os.path.basename(path).split(".")[0]
        return (0, int(stem), path) if stem.isdigit() else (1, 0, path)

    # one file per image: a folder that holds both 7.hdf5 and 7.npz (two runs of stage 1 with different ASR_DATA_EXT)
    # must not evaluate image 7 twice -- the first extension of DATA_EXTS wins (.hdf5, the reference's format)
    best = {}
    for path in sorted(found, key=lambda q: (key(q)[:2], DATA_EXTS.index(next(e for e in DATA_EXTS if q.endswith(e))), q)):
        best.setdefault((os.path.dirname(path), os.path.basename(path).split(".")[0]), path)
    return sorted(best.values(), key=key)


def evaluate_precomputed(sr, paths, gt_dir, standard_dir=None, num_aug=100, class_id=8, th_factor=0.65,
                         img_size=(512, 512), out_dir=None, rank=0, world=1, save_final_output=False, extra_sr_types=(),
                         save_extra_output=False):
    """Returns (table, valid) on every rank: the [len(paths), 6] IoU table (distributed.IOU_FIELDS order) and the bool
    mask of the files that were evaluated.  The row of an invalid file is all-NaN and never enters a mean, like the
    reference's ``continue`` (SR_single_class.py:85-90); a VALID image whose IoUs are NaN (class absent from both masks)
    keeps its row, so the mean over the valid rows is NaN exactly when the reference's np.mean is.

    Validity is what ``load_SR_data`` would decide, read from each file's HEADERS (``probe_SR_data``: no mask is loaded, no
    rank opens another rank's files), so host memory stays at ONE image's maps whatever the shard size, like the
    reference's loop -- and it is all-gathered BEFORE any solve, together with the number of Adam solves each file will run
    (two for slice_max files: class map and max map).  Each valid file is then loaded once, when its turn comes.  ``sr.optimizer``'s global step
    counter is then set per image to what the reference's sequential loop would have reached: num_iter * (solves of the
    valid files before it); a skipped file runs no solve there, so it does not advance the counter here either, and
    sharding changes no update.

    extra_sr_types: any of "median", "trimmed_mean", "covered_mean" and "covered_median" (compute_SR's one-pass fusions
    beyond the reference's; sr.trim is the trimmed fraction, sr.cover / sr.cov_min / sr.valid_min rule the covered ones).  When it is not empty a THIRD value is returned: the [len(paths), len(extra_sr_types)] table of their
    single-class IoUs (compute_IoU without background, like the max and mean columns), gathered like the main table, an
    invalid file's row NaN.  They run after the three reference types and use no optimizer state, so the first two return
    values are what they are without extras.  save_extra_output writes their masks as PNGs under out_dir.  Like the three
    reference types, each extra type goes through compute_SR, which creates its ``{type}_SR`` folder under out_dir whether
    or not anything is saved there: with extras, out_dir must be a folder path (None is refused before any work)."""
    extra = tuple(extra_sr_types)
    for t in extra:
        if t not in EXTRA_SR_TYPES:
            raise ValueError(f"extra_sr_types: {t!r} is not one of {EXTRA_SR_TYPES}")
    if extra and paths and out_dir is None:
        raise ValueError("extra_sr_types needs out_dir: compute_SR creates each type's folder under it")
    extra_records = []
    mine = D.shard_indices(len(paths), rank, world)
    flags = []
    for g in mine:
        ok, n_solves = probe_SR_data(paths[g], num_aug=num_aug)
        if not ok:
            print(f"File: {paths[g]} is invalid, skipping...")
        flags.append([1.0 if ok else 0.0, float(n_solves)])
    status = D.all_gather_rows(mine, flags, len(paths), 2)                    # [files, (valid, solves)] on every rank
    valid = np.nan_to_num(status[:, 0]) > 0.5
    solves = np.where(valid, np.nan_to_num(status[:, 1]), 0.0).astype(np.int64)
    before = np.concatenate([[0], np.cumsum(solves)[:-1]]) if len(paths) else np.zeros(0, np.int64)
    records = []
    for g in mine:
        if not valid[g]:
            records.append([np.nan] * len(D.IOU_FIELDS))
            extra_records.append([np.nan] * len(extra))
            continue
        class_masks, max_masks, angles, shifts, filename = load_SR_data(paths[g], num_aug=num_aug)
        sr.optimizer.optimizer.iterations = int(before[g]) * sr.num_iter
        true_mask = load_image(os.path.join(gt_dir, f"{filename}.png"), image_size=img_size, normalize=False, is_png=True,
                               resize_method="nearest")
        mm = max_masks if max_masks is not None else []
        out = {t: compute_SR(sr, class_masks, angles, shifts, filename, max_masks=mm, SR_type=t, class_id=class_id,
                             dest_folder=out_dir, th_factor=th_factor, save_final_output=save_final_output)
               for t in ("aug", "max", "mean")}
        std = [np.nan, np.nan]
        if standard_dir:
            sm = load_image(os.path.join(standard_dir, f"{filename}.png"), image_size=img_size, normalize=False, is_png=True,
                            resize_method="nearest")
            std = [compute_IoU(true_mask, sm, img_size=img_size, class_id=class_id),
                   compute_IoU(true_mask, sm, img_size=img_size, class_id=class_id, include_bg=True)]
        records.append(std + [compute_IoU(true_mask, out["aug"], img_size=img_size, class_id=class_id),
                              compute_IoU(true_mask, out["aug"], img_size=img_size, class_id=class_id, include_bg=True),
                              compute_IoU(true_mask, out["max"], img_size=img_size, class_id=class_id),
                              compute_IoU(true_mask, out["mean"], img_size=img_size, class_id=class_id)])
        extra_records.append([compute_IoU(true_mask, compute_SR(sr, class_masks, angles, shifts, filename, max_masks=mm,
                                                                SR_type=t, class_id=class_id, dest_folder=out_dir,
                                                                th_factor=th_factor, save_final_output=save_extra_output),
                                          img_size=img_size, class_id=class_id) for t in extra])
    table = D.all_gather_iou(mine, records, len(paths))
    if not extra:
        return table, valid
    return table, valid, D.all_gather_rows(mine, extra_records, len(paths), len(extra))


CLASS_CSV_COLUMNS = ("aug_iou_multiple", "standard_iou_multiple", "aug_iou_single", "standard_iou_single", "max_iou",
                     "mean_iou")
# CSV column -> distributed.IOU_FIELDS entry ("multiple" = include_bg=True)
_CSV_FIELD = {"aug_iou_multiple": "aug_bg", "standard_iou_multiple": "standard_bg", "aug_iou_single": "aug_single",
              "standard_iou_single": "standard_single", "max_iou": "max", "mean_iou": "mean"}


def load_label_map(path, img_size):
    """A ground-truth PNG nearest-resized to img_size, as everywhere -> int32 [H, W] label map (host only)."""
    return load_image(path, image_size=img_size, normalize=False, is_png=True, resize_method="nearest")[..., 0].astype(np.int32)


def classes_of(label_map, class_ids):
    """The classes of an image: the labels of its ground truth that lie in class_ids, in class_ids' order; 0 (background)
    and 255 (void) never count."""
    present = set(int(v) for v in np.unique(np.asarray(label_map)))
    return [int(c) for c in class_ids if int(c) not in (0, 255) and int(c) in present]


def class_presence(gt_paths, class_ids, img_size):
    """bool [images, K]: image g's ground truth holds class_ids[k] (classes_of)."""
    out = np.zeros((len(gt_paths), len(class_ids)), dtype=bool)
    for g, p in enumerate(gt_paths):
        held = set(classes_of(load_label_map(p, img_size), class_ids))
        out[g] = [int(c) in held for c in class_ids]
    return out


def _class_set_run(class_ids, image_paths, gt_paths, rank, world, **draw):
    """What evaluate_classes and evaluate_labelmaps share before their loops: (the validated class ids, image g's replayed draw
    params[g] for every image of the whole list, this rank's image indices).  draw: replay_augmentation_stream's arguments."""
    class_ids = [int(c) for c in class_ids]
    if any(c in (0, 255) for c in class_ids) or len(set(class_ids)) != len(class_ids):
        raise ValueError(f"class_ids must be distinct and exclude 0 (background) and 255 (void), got {class_ids}")
    n_img = len(image_paths)
    if len(gt_paths) != n_img:
        raise ValueError(f"{n_img} images but {len(gt_paths)} ground truths")
    return class_ids, D.replay_augmentation_stream(n_img, **draw), D.shard_indices(n_img, rank, world)


def _image_and_labels_on_device(image_path, gt_path, img_size):
    """(normalised image float32 [H, W, 3], its label map int32 [H, W]), both on the device."""
    image = _image_to_device(load_image(image_path, image_size=img_size, normalize=True))
    return image, ops.to_device(load_label_map(gt_path, img_size), torch.int32, device=image.device)


def evaluate_classes(path, image_paths, gt_paths, class_ids=tuple(range(1, 21)), num_aug=100, angle_max=0.3, shift_max=30,
                     img_size=(512, 512), rank=0, world=1, seed=1234, sr_types=("aug", "max", "mean")):
    """Per-class evaluation of a set of images with one forward pass per image (HotPath.run_image_classes).  Returns
    (table, presence): table [images, K, 6] float64 in distributed.IOU_FIELDS order, NaN where image g's ground truth does
    not hold class_ids[k]; presence [images, K] bool.  An image whose ground truth holds none of the classes is skipped.

    Draws: image g gets draw g of distributed.replay_augmentation_stream over the WHOLE list, and that one draw serves every
    class of the image.  A reference per-class run draws along its own filtered list, so each class's numbers equal a
    per-class run fed these draws, not the reference scripts' draws.
    Adam: class c of image g starts at num_iter * solves_per_image(mode) * #{images before g whose ground truth holds c}
    -- the counter a per-class SR_single_class run over the filtered list reaches.  Every rank reads all label maps to know
    it, so the one all-gather of the results is the only collective."""
    class_ids, params, mine = _class_set_run(class_ids, image_paths, gt_paths, rank, world, num_aug=num_aug,
                                             angle_max=angle_max, shift_max=shift_max, seed=seed)
    n_img, k_set = len(image_paths), len(class_ids)
    presence = class_presence(gt_paths, class_ids, img_size)
    starts = D.adam_class_starts(presence, path.sr.num_iter, path.mode)
    rows = []
    for g in mine:
        rec = np.full((k_set, len(D.IOU_FIELDS)), np.nan)
        held = [c for c, p in zip(class_ids, presence[g]) if p]
        if held:
            image, gt = _image_and_labels_on_device(image_paths[g], gt_paths[g], img_size)
            angles, shifts = params[g]
            res = path.run_image_classes(image, angles, shifts, held, gt_dev=gt, sr_types=sr_types,
                                         adam_starts={c: int(starts[g, class_ids.index(c)]) for c in held})
            for c in held:
                rec[class_ids.index(c)] = res[c]["ious"]
        else:
            print(f"Image: {image_paths[g]} holds none of the classes, skipping...")
        rows.append(rec.reshape(-1))
    width = k_set * len(D.IOU_FIELDS)
    table = D.all_gather_rows(mine, np.asarray(rows).reshape(len(mine), width), n_img, width)
    return table.reshape(n_img, k_set, len(D.IOU_FIELDS)), presence


def class_rows(table, presence, class_ids):
    """The rows of the per-class CSV: for each class held by at least one image, ("Class c", the six column means, number of
    images).  Each mean is np.mean over the images that hold c (a NaN IoU propagates, as in SR_single_class.py)."""
    table = np.asarray(table, dtype=np.float64)
    presence = np.asarray(presence, dtype=bool)
    out = []
    for k, c in enumerate(class_ids):
        sel = presence[:, k]
        if not sel.any():
            continue
        vals = table[sel, k]
        out.append((f"Class {int(c)}", [float(np.mean(vals[:, D.IOU_FIELDS.index(_CSV_FIELD[col])]))
                                        for col in CLASS_CSV_COLUMNS], int(sel.sum())))
    return out


def write_class_csv(path, rows):
    """The reference's final_validations layout (every field quoted), plus the column n_images."""
    import csv
    with open(path, "w", newline="") as fh:
        wr = csv.writer(fh, quoting=csv.QUOTE_ALL, lineterminator="\n")
        wr.writerow(("Name",) + CLASS_CSV_COLUMNS + ("n_images",))
        for name, means, count in rows:
            wr.writerow([name] + [repr(v) for v in means] + [str(count)])


SR_ITERS_CSV_COLUMNS = ("image", "class", "iterations")


def write_sr_iters_csv(path, rows):
    """rows of (image, class, iterations) -- evaluate_labelmaps' sr_iters -- as a CSV, every field quoted."""
    import csv
    with open(path, "w", newline="") as fh:
        wr = csv.writer(fh, quoting=csv.QUOTE_ALL, lineterminator="\n")
        wr.writerow(SR_ITERS_CSV_COLUMNS)
        for image, cls, iterations in rows:
            wr.writerow([str(image), str(cls), str(int(iterations))])


def read_sr_iters_csv(path):
    """write_sr_iters_csv's file -> [(image, class, iterations)], image and class as strings."""
    import csv
    with open(path, newline="") as fh:
        rows = list(csv.reader(fh))
    if not rows or tuple(rows[0]) != SR_ITERS_CSV_COLUMNS:
        raise ValueError(f"{path}: not an SR-iterations CSV (header {rows[:1]})")
    return [(r[0], r[1], int(r[2])) for r in rows[1:]]


COPY_WEIGHTS_CSV_COLUMNS = ("image", "class", "copy", "weight")


def write_copy_weights_csv(path, rows):
    """rows of (image, class, copy, weight) -- evaluate_labelmaps' copy_weights -- as a CSV, every field quoted; the weight is
    written with repr of its float32 value, so the file reads back to the same bits."""
    import csv
    with open(path, "w", newline="") as fh:
        wr = csv.writer(fh, quoting=csv.QUOTE_ALL, lineterminator="\n")
        wr.writerow(COPY_WEIGHTS_CSV_COLUMNS)
        for image, cls, copy, weight in rows:
            wr.writerow([str(image), str(cls), str(int(copy)), repr(float(np.float32(weight)))])


def read_copy_weights_csv(path):
    """write_copy_weights_csv's file -> [(image, class, copy, weight)], image and class as strings, weight a float."""
    import csv
    with open(path, newline="") as fh:
        rows = list(csv.reader(fh))
    if not rows or tuple(rows[0]) != COPY_WEIGHTS_CSV_COLUMNS:
        raise ValueError(f"{path}: not a copy-weights CSV (header {rows[:1]})")
    return [(r[0], r[1], int(r[2]), float(r[3])) for r in rows[1:]]


# ---- label maps: one fused label map per image and SR type, scored with the multi-class Mean_IOU ------------------------
LABELMAP_KEYS = ("standard", "aug", "max", "mean")
LABELMAP_CSV_COLUMNS = ("standard_iou", "aug_iou", "max_iou", "mean_iou")


# the attribute names of LabelmapScores by field prefix: (per-image Mean_IOU rows, summed counts), or the counts alone
_SCORE_ATTRS = {"": ("rows", "counts"), "band_": ("band_rows", "band_counts"), "confusion": ("confusion",),
                "sweep_": ("sweep_rows", "sweep_counts"), "coverage_": ("cov_rows", "cov_counts"),
                "raw_": ("raw_rows", "raw_counts"), "regions": ("regions",), "segments": ("segments",),
                "raw_segments": ("raw_segments",)}


class LabelmapScores(tuple):
    """What gather_labelmap_records and evaluate_labelmaps return: the tuple
    (rows, counts[, band_rows, band_counts][, confusion][, sweep_rows, sweep_counts][, cov_rows, cov_counts][, raw_rows,
    raw_counts, regions][, segments][, raw_segments]), one or two entries per field of label_record.label_fields that is on.  Every entry is also an attribute of that name, None when its
    field is off."""

    def __new__(cls, items=(), names=()):
        self = super().__new__(cls, items)
        vars(self).update(dict.fromkeys(sum(_SCORE_ATTRS.values(), ()), None))
        vars(self).update(zip(names, self))
        return self


def gather_labelmap_records(local_indices, fields, local, num_images):
    """The one collective of evaluate_labelmaps.  fields: label_record.label_fields(LABELMAP_KEYS, ...); local: {field:
    (local_miou | None, local_counts)}, for each field the per-image Mean_IOU [n_local, len(keys), *shape[:-2]] (scored
    fields only) and the integer counts [n_local, len(keys), *shape] of this rank's images.  Returns on every rank a
    LabelmapScores: per scored field the rows [num_images, len(keys), *shape[:-2]] float64, NaN where no rank reported, and
    per field the counts [len(keys), *shape] int64 summed over the images.  The counts travel as float64 in the same
    all-gather as the rows, laid out by label_record.label_layout: exact below 2^53 pixels per bin."""
    spans, width = label_layout(fields, with_miou=True)
    n_local = len(local_indices)
    rec = np.empty((n_local, width), dtype=np.float64)
    if n_local:
        for f, (rows, cells) in zip(fields, spans):
            miou, counts = local[f]
            if rows is not None:
                rec[:, rows] = np.asarray(miou, dtype=np.float64).reshape(n_local, -1)
            rec[:, cells] = np.asarray(counts, dtype=np.int64).reshape(n_local, -1)
    table = D.all_gather_rows(local_indices, rec, num_images, width)
    out, names = [], ()
    for f, (rows, cells) in zip(fields, spans):
        if rows is not None:
            out.append(table[:, rows].reshape((num_images, len(f.keys)) + f.shape[:-2]))
        out.append(np.nan_to_num(table[:, cells]).astype(np.int64).reshape((num_images, len(f.keys)) + f.shape).sum(axis=0))
        names += _SCORE_ATTRS[f.prefix]
    return LabelmapScores(out, names)


def label_ious(counts):
    """counts [3, 256] -> {label: inter / union} for the labels the ground truth holds, void (255) removed."""
    c = np.asarray(counts, dtype=np.int64)
    return {l: float(np.float64(c[2, l]) / np.float64(c[0, l] + c[1, l] - c[2, l])) for l in range(255) if c[0, l] > 0}


def dataset_miou(counts):
    """The dataset-level VOC mIoU: per-label IoU from the counts summed over the images, mean over the labels present
    (utils.mean_iou_from_counts on the sum); NaN when the ground truths hold no label."""
    from .utils import mean_iou_from_counts
    return mean_iou_from_counts(counts)


def evaluate_labelmaps(path, image_paths, gt_paths, class_ids=tuple(range(1, 21)), num_aug=100, angle_max=0.3, shift_max=30,
                       img_size=(512, 512), rank=0, world=1, seed=1234, sr_types=("aug", "max", "mean"), prune=True,
                       save_dir=None, band_widths=None, band_ignore_label=255, confusion_labels=None, th_factors=None,
                       guide=None, df_weights=None, sr_stop=None, sr_iters=None, couple=False, sr_reweight=None, copy_weights=None,
                       tv_guide=None, crf=None,
                       min_region=None, segments=None, coverages=None, uncertainty_dir=None):
    """One fused label map per image and SR type (HotPath.run_image_labels) and its score.  Returns on every rank a
    LabelmapScores, the tuple (rows, counts) plus what the options below append, every entry also an attribute by the name
    given here: rows [images, 4] per-image Mean_IOU in LABELMAP_KEYS order (the reference's per-image-then-mean convention;
    NaN for an SR type that was not asked for), counts [4, 3, 256] int64 summed over the images (dataset_miou, label_ious).

    The class set is the SAME for every image and is never read from the ground truth, so a class that is not in an image
    can be predicted there and costs IoU.  Draws: image g gets draw g of distributed.replay_augmentation_stream over the
    whole list, as evaluate_classes.  Adam: every image counts as holding every class, so class c of image g starts at
    num_iter * solves_per_image(mode) * g -- evaluate_classes's rule with an all-true presence -- whatever the sharding and
    whatever pruning leaves out.  One all-gather at the end.  save_dir: the label maps as <stem>_<key>.png (8-bit).

    band_widths (B integers in [1, 64]): the same loop also collects each label map's trimap counts (run_image_labels'
    band_widths / band_ignore_label) and the return value is (rows, counts, band_rows, band_counts): band_rows [images, 4, B]
    per-image Mean_IOU inside each band, band_counts [4, B, 3, 256] int64 summed over the images, both NaN / zero for a label
    map that was not asked for.  They travel in the same all-gather.

    confusion_labels (an integer L in [1, 64]): the same loop also collects each label map's confusion matrix against the
    ground truth (run_image_labels' confusion_labels) and the return value gains one more entry, confusion: the matrices
    [4, L+1, L+1] int64 in LABELMAP_KEYS order, summed over the images (utils.metrics_from_confusion, write_confusion_csv), all
    zero for a label map that was not asked for.  They travel in the same all-gather as well.

    th_factors (T threshold factors, 1..64; not in slice_max mode): the same loop also collects the counts of every SR label
    map under every factor (run_image_labels' th_factors: one more pass over the SR outputs it already holds, no further
    forward pass or solve) and the return value ends in two more entries: sweep_rows [images, 3, T] per-image Mean_IOU and
    sweep_counts [3, T, 3, 256] int64 summed over the images, both in the order aug / max / mean and NaN / zero for an SR
    type that was not asked for (write_labelmap_threshold_csv).  They travel in the same all-gather.

    guide ((radius, eps)): every SR score map is refined with the guided filter against its image before the fusion
    (run_image_labels' guide; img_size must be the SR output size).  The return value keeps its form.

    tv_guide (beta, finite and >= 0): every image's "aug" solves weight their TV prior by the image's own edges
    (run_image_labels' tv_guide; img_size must be the SR output size, no bilateral TV).  Independent of guide.  The return
    value keeps its form.

    df_weights ("maxprob" or "margin"): every image's "aug" solves weight each measurement of their data term by the network's
    confidence there (run_image_labels' df_weights; the loss is the solver's df_loss).  The return value keeps its form.

    crf (a dict of the windowed CRF's fields plus tau and standard_conf): every SR label map is decided by the windowed CRF over
    classes and image instead of the fusion (run_image_labels' crf; img_size must be the SR output size; not in slice_max mode
    and not together with th_factors).  The return value keeps its form.

    coverages (C whole percentages in [1, 100], 1..16): the same loop also collects each label map's counts over its p % most
    certain pixels (run_image_labels' coverages: the variance of the class stacks over the copies, no further forward pass
    or solve) and the return value ends in two more entries, after the sweep's: cov_rows [images, 4, C] per-image Mean_IOU
    and cov_counts [4, C, 3, 256] int64 summed over the images, NaN / zero for a label map that was not asked for
    (write_coverage_csv).  The quantiles are each image's own.  They travel in the same all-gather.  uncertainty_dir (with
    coverages): sqrt of each image's uncertainty map, the standard deviation over the copies, as <stem>.npy (float32 [H, W]).

    min_region (an integer A or (A, connectivity); not together with th_factors): every label map is cleaned of its regions of
    fewer than A pixels before it is scored and saved (run_image_labels' min_region), so every entry above is the cleaned
    maps', and the return value ends in three more entries: raw_rows [images, 4] and raw_counts [4, 3, 256], what rows and
    counts are without the option, and regions [4, 4] int64, per label map the regions, small regions, pixels in small
    regions and pixels changed, summed over the images (write_regions_csv).  They travel in the same all-gather.

    segments (an integer L, (L, connectivity) or (L, connectivity, include_zero); not together with th_factors): the same loop
    also matches each label map's segments against the ground truth's (run_image_labels' segments) and the return value ends
    in one more entry, segments [4, L, 4] int64, per label map and label TP, FP, FN and Q summed over the images
    (utils.metrics_from_segments, write_segments_csv), all zero for a label map that was not asked for; with min_region
    another follows, raw_segments, the same of the maps before the clean-up.  They travel in the same float64 all-gather:
    exact while a Q sum stays below 2^53, that is 2^23 (about 8 million) matched segments per label map and label, each
    adding at most 2^30.

    sr_stop (run_image_labels' sr_stop: rel_tol, patience, every, min_iter): every image's "aug" solves stop class by class
    once their loss has stalled.  The return value keeps its form; sr_iters (a list) receives one row (image stem, class id,
    iterations) per image of THIS rank and solved class (write_sr_iters_csv; in slice_max a second row per class, the class
    written "<id>_max", for its max map's solve).  The Adam bookkeeping does not change.

    couple (True needs the primal_dual optimizer and the argmax mode; not together with th_factors or crf): every image's "aug"
    solve is one coupled solve over its classes and its "aug" map the threshold-free fusion of the shares (run_image_labels'
    couple).  The return value keeps its form.

    sr_reweight (run_image_labels' sr_reweight: a kind name, or kind, kappa, every, start): every image's "aug" solves
    down-weight whole unreliable copies, class by class.  The return value keeps its form; copy_weights (a list) receives one
    row (image stem, class id, copy index, final weight) per image of THIS rank, solved class and copy (write_copy_weights_csv;
    in slice_max a second set of rows per class, the class written "<id>_max", for its max map's solve)."""
    stop_kw = {} if path.check_sr_stop(sr_stop) is None else {"sr_stop": dict(sr_stop)}
    rw_on = path.check_sr_reweight(sr_reweight) is not None
    if rw_on:
        stop_kw["sr_reweight"] = dict(sr_reweight) if isinstance(sr_reweight, dict) else sr_reweight
    path.check_couple(couple, th_factors, crf)
    if couple:
        stop_kw["couple"] = True
    if uncertainty_dir and coverages is None:
        raise ValueError("uncertainty_dir needs coverages: the uncertainty map is only built for the risk-coverage curve")
    opts = path.label_options(tuple(img_size) + (3,), True, band_widths, band_ignore_label, confusion_labels, th_factors,
                              guide, coverages, bool(uncertainty_dir), min_region, segments)
    tv_beta = path.check_tv_guide(tv_guide, tuple(img_size) + (3,))
    tv_kw = {} if tv_beta is None else {"tv_guide": tv_beta}
    if path.check_df_weights(df_weights) is not None:
        tv_kw["df_weights"] = df_weights
    if crf is not None:
        class_ids = list(class_ids)
        path.check_crf(crf, tuple(img_size) + (3,), th_factors, len(class_ids))
        tv_kw["crf"] = dict(crf)
    if uncertainty_dir:
        os.makedirs(uncertainty_dir, exist_ok=True)
    class_ids, params, mine = _class_set_run(class_ids, image_paths, gt_paths, rank, world, num_aug=num_aug,
                                             angle_max=angle_max, shift_max=shift_max, seed=seed)
    n_img = len(image_paths)
    starts = D.adam_class_starts(np.ones((n_img, len(class_ids)), dtype=bool), path.sr.num_iter, path.mode)
    if save_dir:
        os.makedirs(save_dir, exist_ok=True)
    fields = label_fields(LABELMAP_KEYS, *opts.sizes, n_segments=opts.segments[0] if opts.segments else 0)
    local = {f: ([], []) for f in fields}
    for g in mine:
        image, gt = _image_and_labels_on_device(image_paths[g], gt_paths[g], img_size)
        angles, shifts = params[g]
        res = path.run_image_labels(image, angles, shifts, class_ids, gt_dev=gt, sr_types=sr_types, prune=prune,
                                    adam_starts={c: int(starts[g, k]) for k, c in enumerate(class_ids)},
                                    band_widths=opts.bands, band_ignore_label=band_ignore_label,
                                    confusion_labels=opts.n_conf or None, th_factors=opts.factors, guide=opts.guide,
                                    coverages=opts.covs, keep_uncertainty=bool(uncertainty_dir), min_region=opts.min_region,
                                    segments=opts.segments, **tv_kw, **stop_kw)
        if rw_on and copy_weights is not None:
            stem = os.path.splitext(os.path.basename(image_paths[g]))[0]
            for solve, cw in sorted(res["copy_weights"].items()):
                tag = "_max" if solve == "aug_max" else ""
                copy_weights.extend((stem, f"{c}{tag}", i, float(v)) for c, row in zip(res["solved_ids"], cw) for i, v in enumerate(row))
        if "sr_stop" in stop_kw and sr_iters is not None:
            stem = os.path.splitext(os.path.basename(image_paths[g]))[0]
            for solve, its in sorted(res["sr_iters"].items()):
                tag = "_max" if solve == "aug_max" else ""
                sr_iters.extend((stem, f"{c}{tag}", int(k)) for c, k in zip(res["solved_ids"], its))
        for f, (mious, counts) in local.items():        # a label map that was not produced: NaN Mean_IOU, zero counts
            if f.scored:
                mious.append([res[f.prefix + "Mean_IOU"].get(key, np.full(f.shape[:-2], np.nan)) for key in f.keys])
            counts.append([res[counts_name(f)].get(key, np.zeros(f.shape, np.int64)) for key in f.keys])
        if uncertainty_dir:
            np.save(os.path.join(uncertainty_dir, os.path.splitext(os.path.basename(image_paths[g]))[0] + ".npy"),
                    torch.sqrt(res["uncertainty"]).cpu().numpy())
        if save_dir:
            from PIL import Image
            stem = os.path.splitext(os.path.basename(image_paths[g]))[0]
            for key in LABELMAP_KEYS:
                if key in res:
                    Image.fromarray(res[key].cpu().numpy().astype(np.uint8), mode="L").save(
                        os.path.join(save_dir, f"{stem}_{key}.png"))
    return gather_labelmap_records(mine, fields, local, n_img)


def _miou_cells(made, counts, image_mious):
    """The two CSV cells of one label map: the dataset mIoU of its counts [3, 256] summed over the images, and np.mean of its
    per-image Mean_IOU [images] (a NaN image propagates; "nan" without images).  made False -- the label map was not
    produced, its counts are all zero -- both are "nan"."""
    if not made:
        return ["nan", "nan"]
    return [repr(dataset_miou(counts)), repr(float(np.mean(image_mious))) if len(image_mious) else "nan"]


def _counted_truth_pixels(counts, ignore_label):
    """The ground-truth pixels that the whole-image counts [4, 3, 256] counted, ignore_label's (-1 or None: none) taken out."""
    truth = np.asarray(counts, dtype=np.int64).reshape(len(LABELMAP_KEYS), 3, 256)[:, 0].max(axis=0).copy()
    if ignore_label is not None and 0 <= int(ignore_label) <= 255:
        truth[int(ignore_label)] = 0
    return int(truth.sum())


def write_labelmap_csv(path, counts, rows):
    """One row per label the ground truths hold ("Label l": its IoU from the summed counts for standard / aug / max / mean,
    n = its ground-truth pixels), then both means: "dataset_mIoU" (dataset_miou of each column) and "mean_image_mIoU"
    (np.mean of the per-image Mean_IOU rows; a NaN image propagates, as in the reference), n = number of images.  The column
    of a label map that was not produced (all-zero counts) is nan throughout."""
    import csv
    counts = np.asarray(counts, dtype=np.int64)
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, len(LABELMAP_KEYS))
    per = [label_ious(counts[j]) for j in range(len(LABELMAP_KEYS))]
    truth = counts[:, 0].max(axis=0)              # a label map that was not asked for carries all-zero counts: its cells are nan
    with open(path, "w", newline="") as fh:
        wr = csv.writer(fh, quoting=csv.QUOTE_ALL, lineterminator="\n")
        wr.writerow(("Name",) + LABELMAP_CSV_COLUMNS + ("n",))
        for l in sorted(l for l in range(255) if truth[l] > 0):
            wr.writerow([f"Label {l}"] + [repr(p.get(l, float("nan"))) for p in per] + [str(int(truth[l]))])
        wr.writerow(["dataset_mIoU"] + [repr(dataset_miou(counts[j])) for j in range(len(LABELMAP_KEYS))] + [str(len(rows))])
        wr.writerow(["mean_image_mIoU"] + [repr(float(np.mean(rows[:, j]))) if len(rows) else "nan"
                                           for j in range(len(LABELMAP_KEYS))] + [str(len(rows))])


REGIONS_CSV_COLUMNS = ("key", "regions", "small_regions", "small_region_pixels", "pixels_changed", "raw_dataset_mIoU",
                       "raw_mean_image_mIoU", "dataset_mIoU", "mean_image_mIoU")


def write_regions_csv(path, regions, raw_counts, raw_rows, counts, rows):
    """What removing the small regions did, one row per label map (standard / aug / max / mean): the regions, the small regions,
    the pixels in small regions and the pixels changed, regions [4, 4] summed over the images, then the dataset mIoU and the
    mean image mIoU before the clean-up (raw_counts [4, 3, 256], raw_rows [images, 4]) and after it (counts, rows): what
    write_labelmap_csv's last two rows hold.  The cells of a label map that was not produced (all-zero counts) are nan."""
    import csv
    regions = np.asarray(regions, dtype=np.int64).reshape(len(LABELMAP_KEYS), 4)
    raw_counts, counts = np.asarray(raw_counts, dtype=np.int64), np.asarray(counts, dtype=np.int64)
    raw_rows = np.asarray(raw_rows, dtype=np.float64).reshape(-1, len(LABELMAP_KEYS))
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, len(LABELMAP_KEYS))
    with open(path, "w", newline="") as fh:
        wr = csv.writer(fh, quoting=csv.QUOTE_ALL, lineterminator="\n")
        wr.writerow(REGIONS_CSV_COLUMNS)
        for j, key in enumerate(LABELMAP_KEYS):
            made = bool(counts[j].any() or raw_counts[j].any())
            wr.writerow([key] + ([str(int(v)) for v in regions[j]] if made else ["nan"] * 4)
                        + _miou_cells(made, raw_counts[j], raw_rows[:, j]) + _miou_cells(made, counts[j], rows[:, j]))


SEGMENTS_CSV_COLUMNS = ("key", "stage", "label", "TP", "FP", "FN", "precision", "recall", "SQ", "RQ", "PQ")


def write_segments_csv(path, segments, raw_segments=None, class_names=None):
    """The region-by-region scores in long form, one row per (label map, stage, label): segments [4, L, 4] int64 (TP, FP, FN, Q
    summed over the images, LABELMAP_KEYS order) is the stage "final"; raw_segments, the same before the clean-up, when given
    the stage "raw", written ahead of it.  Each row holds TP, FP, FN and utils.metrics_from_segments' precision, recall, SQ, RQ
    and PQ, for the labels with TP + FP + FN > 0 (named as in write_confusion_csv: class_names or the number); a row "mean" per (key,
    stage) follows them with the summed TP, FP, FN, empty precision and recall, and the mean SQ, RQ and PQ over those labels.
    A label map without any segment (not produced, or nothing to match) has its "mean" row alone, nan."""
    import csv
    from .utils import metrics_from_segments
    stages = [("final", np.asarray(segments, dtype=np.int64))]
    if raw_segments is not None:
        stages.insert(0, ("raw", np.asarray(raw_segments, dtype=np.int64)))
    with open(path, "w", newline="") as fh:
        wr = csv.writer(fh, quoting=csv.QUOTE_ALL, lineterminator="\n")
        wr.writerow(SEGMENTS_CSV_COLUMNS)
        for j, key in enumerate(LABELMAP_KEYS):
            for stage, counts in stages:
                c = counts.reshape(len(LABELMAP_KEYS), -1, 4)[j]
                m = metrics_from_segments(c)
                names = confusion_label_names(c.shape[0], class_names)
                for l in np.nonzero(c[:, :3].sum(axis=1) > 0)[0].tolist():
                    wr.writerow([key, stage, names[l]] + [str(int(v)) for v in c[l, :3]]
                                + [repr(float(m[k][l])) for k in ("precision", "recall", "SQ", "RQ", "PQ")])
                wr.writerow([key, stage, "mean"] + [str(int(v)) for v in c[:, :3].sum(axis=0)] + ["", ""]
                            + [repr(m[k]) for k in ("mean_SQ", "mean_RQ", "mean_PQ")])


THRESHOLD_CSV_COLUMNS = ("th_factor",) + tuple(f"{key}_{kind}" for key in LABELMAP_KEYS[1:] + LABELMAP_KEYS[:1]
                                                for kind in ("dataset_mIoU", "mean_image_mIoU"))


def write_labelmap_threshold_csv(path, factors, sweep_counts, sweep_rows, counts, rows):
    """The threshold curve of the label maps, one row per factor in the caller's order: "th_factor", then for aug / max / mean
    "<key>_dataset_mIoU" (dataset_miou of sweep_counts [3, T, 3, 256], the counts summed over the images) and
    "<key>_mean_image_mIoU" (np.mean of the per-image Mean_IOU, sweep_rows [images, 3, T]; a NaN image propagates), then the
    same two columns of the standard label map, which does not depend on the factor: constants taken from counts [4, 3, 256]
    and rows [images, 4], what write_labelmap_csv takes.  The columns of a label map that was not produced (all-zero counts)
    are nan.  Quoting and repr floats as write_labelmap_csv."""
    import csv
    fs = [float(f) for f in np.asarray(factors, dtype=np.float64).reshape(-1)]
    ms = len(LABELMAP_KEYS) - 1
    sweep_counts = np.asarray(sweep_counts, dtype=np.int64).reshape(ms, len(fs), 3, 256)
    sweep_rows = np.asarray(sweep_rows, dtype=np.float64).reshape(-1, ms, len(fs))
    counts = np.asarray(counts, dtype=np.int64).reshape(len(LABELMAP_KEYS), 3, 256)
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, len(LABELMAP_KEYS))
    standard = _miou_cells(counts[0].any(), counts[0], rows[:, 0])
    with open(path, "w", newline="") as fh:
        wr = csv.writer(fh, quoting=csv.QUOTE_ALL, lineterminator="\n")
        wr.writerow(THRESHOLD_CSV_COLUMNS)
        for j, f in enumerate(fs):
            cells = []
            for i in range(ms):                             # an SR type that was not asked for carries all-zero counts
                cells += _miou_cells(sweep_counts[i].any(), sweep_counts[i, j], sweep_rows[:, i, j])
            wr.writerow([repr(f)] + cells + standard)


def best_threshold_factors(factors, sweep_counts):
    """{key: (factor, dataset mIoU)} for aug / max / mean: the factor of the greatest dataset mIoU (the first on equal values);
    an SR type that was not produced, or whose mIoU is NaN under every factor, is left out."""
    fs = [float(f) for f in np.asarray(factors, dtype=np.float64).reshape(-1)]
    sweep_counts = np.asarray(sweep_counts, dtype=np.int64).reshape(len(LABELMAP_KEYS) - 1, len(fs), 3, 256)
    best = {}
    for i, key in enumerate(LABELMAP_KEYS[1:]):
        if not sweep_counts[i].any():
            continue
        curve = np.array([dataset_miou(c) for c in sweep_counts[i]], dtype=np.float64)
        if not np.all(np.isnan(curve)):
            j = int(np.nanargmax(curve))
            best[key] = (fs[j], float(curve[j]))
    return best


TRIMAP_CSV_COLUMNS = tuple(f"{key}_{kind}" for key in LABELMAP_KEYS for kind in ("band_mIoU", "band_mean_image_mIoU"))


def write_trimap_csv(path, widths, band_counts, band_rows, counts=None, ignore_label=255):
    """One row per band width ("w=<width>", in the caller's order).  For standard / aug / max / mean: "<key>_band_mIoU", the
    dataset mIoU inside the band (dataset_miou of band_counts [4, B, 3, 256], the counts summed over the images), and
    "<key>_band_mean_image_mIoU", np.mean of the per-image band Mean_IOU (band_rows [images, 4, B]; a NaN image propagates).
    "band_pixels": the ground-truth pixels counted in the band (labels 0..255, the ignored label never among them);
    "band_share": that number over the counted ground-truth pixels of the whole images -- from counts [4, 3, 256], the
    whole-image counts write_labelmap_csv takes, with ignore_label's pixels (-1 or None: none) taken out; nan without counts.
    The columns of a label map that was not produced (all-zero counts) are nan.  n = number of images."""
    import csv
    ws = [int(v) for v in widths]
    m = len(LABELMAP_KEYS)
    band_counts = np.asarray(band_counts, dtype=np.int64).reshape(m, len(ws), 3, 256)
    band_rows = np.asarray(band_rows, dtype=np.float64).reshape(-1, m, len(ws))
    total = _counted_truth_pixels(counts, ignore_label) if counts is not None else None
    with open(path, "w", newline="") as fh:
        wr = csv.writer(fh, quoting=csv.QUOTE_ALL, lineterminator="\n")
        wr.writerow(("Name",) + TRIMAP_CSV_COLUMNS + ("band_pixels", "band_share", "n"))
        for b, width in enumerate(ws):
            cells = []
            for j in range(m):                              # a label map that was not asked for carries all-zero counts
                cells += _miou_cells(band_counts[j].any(), band_counts[j, b], band_rows[:, j, b])
            pixels = int(band_counts[:, b, 0].max(axis=0).sum())
            share = repr(pixels / total) if total else "nan"
            wr.writerow([f"w={width}"] + cells + [str(pixels), share, str(len(band_rows))])


COVERAGE_CSV_COLUMNS = tuple(f"{key}_{kind}" for key in LABELMAP_KEYS
                             for kind in ("dataset_mIoU", "mean_image_mIoU", "retained_share"))


def write_coverage_csv(path, percents, cov_counts, cov_rows, counts=None, ignore_label=255):
    """The risk-coverage curve of the label maps, one row per percentage ("coverage", in the caller's order).  For standard /
    aug / max / mean: "<key>_dataset_mIoU" (dataset_miou of cov_counts [4, C, 3, 256], the counts over each image's p % most
    certain pixels summed over the images), "<key>_mean_image_mIoU" (np.mean of the per-image Mean_IOU, cov_rows
    [images, 4, C]; a NaN image propagates) and "<key>_retained_share": the ground-truth pixels the row retained (labels
    0..255 of its counts) over the counted ground-truth pixels of the whole images -- from counts [4, 3, 256], the
    whole-image counts write_labelmap_csv takes, with ignore_label's pixels (-1 or None: none) taken out; without counts,
    over the pixels of the 100 % row when percents holds one, else nan.  The share is >= p / 100: pixels tied with the
    quantile stay in.  The columns of a label map that was not produced (all-zero counts) are nan.  n = number of images."""
    import csv
    ps = ops.check_coverages(percents)
    m = len(LABELMAP_KEYS)
    cov_counts = np.asarray(cov_counts, dtype=np.int64).reshape(m, len(ps), 3, 256)
    cov_rows = np.asarray(cov_rows, dtype=np.float64).reshape(-1, m, len(ps))
    total = None
    if counts is not None:
        total = _counted_truth_pixels(counts, ignore_label)
    elif 100 in ps:
        total = int(cov_counts[:, ps.index(100), 0].max(axis=0).sum())
    with open(path, "w", newline="") as fh:
        wr = csv.writer(fh, quoting=csv.QUOTE_ALL, lineterminator="\n")
        wr.writerow(("coverage",) + COVERAGE_CSV_COLUMNS + ("n",))
        for b, p in enumerate(ps):
            cells = []
            for j in range(m):
                made = bool(cov_counts[j].any())            # a label map that was not asked for carries all-zero counts
                cells += _miou_cells(made, cov_counts[j, b], cov_rows[:, j, b])
                cells.append(repr(int(cov_counts[j, b, 0].sum()) / total) if made and total else "nan")
            wr.writerow([str(p)] + cells + [str(len(cov_rows))])


CONFUSION_CSV_COLUMNS = ("key", "truth", "predicted", "pixels", "share_of_truth")
CONFUSION_METRICS_CSV_COLUMNS = ("key", "other", "metric", "label", "value")
CONFUSION_SCALARS = ("pixel_accuracy", "mean_accuracy", "Mean_IOU", "fw_iou")
CONFUSION_PER_LABEL = ("precision", "recall", "iou")


def _confusion_by_key(matrices):
    """{key: [L+1, L+1] int64} in LABELMAP_KEYS order from such a dict or from an array [4, L+1, L+1] in that order; a label map
    that was not produced (an all-zero matrix) is left out."""
    if isinstance(matrices, dict):
        items = [(key, matrices[key]) for key in LABELMAP_KEYS if key in matrices]
    else:
        items = list(zip(LABELMAP_KEYS, np.asarray(matrices)))
    out = {key: np.asarray(m, dtype=np.int64) for key, m in items}
    for key, m in out.items():
        if m.ndim != 2 or m.shape[0] != m.shape[1] or m.shape[0] < 2:
            raise ValueError(f"confusion matrix of {key}: expected [L+1, L+1], got {m.shape}")
    return {key: m for key, m in out.items() if m.any()}


def confusion_label_names(num_labels, class_names=None):
    """The L + 1 names of a confusion matrix's bins: class_names (at least L of them) or "0".."L-1", then "other"."""
    if class_names is None:
        names = [str(l) for l in range(num_labels)]
    else:
        names = [str(n) for n in class_names][:num_labels]
        if len(names) < num_labels:
            raise ValueError(f"{len(names)} class names for {num_labels} labels")
    return names + ["other"]


def write_confusion_csv(path, matrices, class_names=None):
    """The confusion matrices in long form: one row per (key, truth label, predicted label) with its pixels and its share of
    the truth label's row (nan for a label the ground truths do not hold), for every label map that was produced.  matrices:
    {key: int64 [L+1, L+1]} or an array [4, L+1, L+1] in LABELMAP_KEYS order (evaluate_labelmaps' confusion entry).  Labels are
    named by class_names (L names) or by their number; bin L is "other".  The shares of a row that holds pixels sum to 1."""
    import csv
    with open(path, "w", newline="") as fh:
        wr = csv.writer(fh, quoting=csv.QUOTE_ALL, lineterminator="\n")
        wr.writerow(CONFUSION_CSV_COLUMNS)
        for key, m in _confusion_by_key(matrices).items():
            names = confusion_label_names(m.shape[0] - 1, class_names)
            rows = m.sum(axis=1)
            for i, t in enumerate(names):
                for j, p in enumerate(names):
                    share = repr(float(np.float64(m[i, j]) / np.float64(rows[i]))) if rows[i] else "nan"
                    wr.writerow([key, t, p, str(int(m[i, j])), share])


def write_confusion_metrics_csv(path, matrices, class_names=None):
    """utils.metrics_from_confusion of every produced label map under both conventions for the other bin, in long form: one
    row per (key, other, metric, label, value); label is empty for pixel_accuracy, mean_accuracy, Mean_IOU and fw_iou and the
    label's name for precision, recall and iou."""
    import csv
    from .utils import metrics_from_confusion
    with open(path, "w", newline="") as fh:
        wr = csv.writer(fh, quoting=csv.QUOTE_ALL, lineterminator="\n")
        wr.writerow(CONFUSION_METRICS_CSV_COLUMNS)
        for key, m in _confusion_by_key(matrices).items():
            names = confusion_label_names(m.shape[0] - 1, class_names)
            for other in ("ignore", "label"):
                res = metrics_from_confusion(m, other=other)
                for name in CONFUSION_SCALARS:
                    wr.writerow([key, other, name, "", repr(float(res[name]))])
                for name in CONFUSION_PER_LABEL:
                    for l, v in enumerate(res[name]):
                        wr.writerow([key, other, name, names[l], repr(float(v))])


def valid_rows(table, valid=None):
    """Rows of the images that were evaluated: by the explicit mask evaluate_precomputed returns; without one, every row
    that is not all-NaN (a table from elsewhere)."""
    table = np.asarray(table, dtype=np.float64)
    if valid is not None:
        return table[np.asarray(valid, dtype=bool)]
    return table[~np.isnan(table).all(axis=1)]


def mean_over_valid(table, valid=None):
    """The six means SR_single_class.py:129-134 prints: np.mean over the images that were not skipped (NaN where a valid
    image has a NaN IoU, as there)."""
    return D.mean_ious(valid_rows(table, valid))
