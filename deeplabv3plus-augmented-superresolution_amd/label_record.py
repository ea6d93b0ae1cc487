"""The one layout of the label-map scores ("the label-map record"): the device buffer of
HotPath.run_image_labels, its result dict, the all-gather record of evaluation.gather_labelmap_records and the tuple
evaluation.evaluate_labelmaps returns are all read off the field list below."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

# prefix: of the field's result names; keys: the label maps it is stored for, in order; shape: of one key's counts;
# scored: the shape ends in [3, 256] (ops.class_counts), so each [3, 256] of it has a Mean_IOU
Field = namedtuple("Field", "prefix keys shape scored")


def label_fields(keys, n_bands=0, n_conf=0, n_factors=0, n_cov=0, n_regions=0, n_segments=0):
    """The fields that are switched on, in the order they are stored: whole-image counts, then with B band widths the trimap,
    with L labels the confusion matrix, with T threshold factors the sweep (SR label maps only: the standard map does not
    depend on the factor), with C coverages the risk-coverage curve, with n_regions set (small regions removed from the label
    maps) the whole-image counts of the maps before the clean-up and the four region statistics of include/asr_hip.h, with
    n_segments = L labels the segment counts (TP, FP, FN, Q per label; include/asr_hip.h, "segments") of the finished maps
    and, when n_regions is on as well, of the maps before the clean-up."""
    keys = tuple(keys)
    fields = [Field("", keys, (3, 256), True)]
    if n_bands:
        fields.append(Field("band_", keys, (n_bands, 3, 256), True))
    if n_conf:
        fields.append(Field("confusion", keys, (n_conf + 1, n_conf + 1), False))
    if n_factors:
        fields.append(Field("sweep_", tuple(k for k in keys if k != "standard"), (n_factors, 3, 256), True))
    if n_cov:
        fields.append(Field("coverage_", keys, (n_cov, 3, 256), True))
    if n_regions:
        fields.append(Field("raw_", keys, (3, 256), True))
        fields.append(Field("regions", keys, (4,), False))
    if n_segments:
        fields.append(Field("segments", keys, (n_segments, 4), False))
        if n_regions:
            fields.append(Field("raw_segments", keys, (n_segments, 4), False))
    return tuple(fields)


def counts_name(field):
    """The result name of the field's counts; its Mean_IOU (scored fields, one per [3, 256], so of shape[:-2]) is
    prefix + "Mean_IOU"."""
    return field.prefix + "counts" if field.scored else field.prefix


def label_layout(fields, with_miou):
    """([(Mean_IOU slice | None, counts slice) per field], total length) of the flat record: the fields one after another,
    each len(keys) * prod(shape) count cells, ahead of them with_miou its len(keys) * prod(shape[:-2]) Mean_IOU cells."""
    spans, at = [], 0
    for f in fields:
        rows = len(f.keys) * int(np.prod(f.shape[:-2])) if with_miou and f.scored else 0
        cells = len(f.keys) * int(np.prod(f.shape))
        spans.append((slice(at, at + rows) if with_miou and f.scored else None, slice(at + rows, at + rows + cells)))
        at += rows + cells
    return spans, at
