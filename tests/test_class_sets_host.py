"""Class sets (one forward pass for every class of an image), host side: the library refuses a bad class set before any
launch, the per-(image, class) Adam start steps, the class selection from label maps and the per-class CSV.  No GPU."""
import ctypes as C
import csv
import math

import numpy as np
import pytest

FAKE = 1 << 20                      # non-null, aligned; never dereferenced: the calls fail on the class set first


def _ids(*v):
    return (C.c_int * max(len(v), 1))(*v)


BAD_SETS = [
    ("K = 0", _ids(), 0, b"class ids (1..32)"),
    ("K = 33", _ids(*range(33)), 33, b"class ids (1..32)"),
    ("duplicate", _ids(3, 8, 3), 3, b"given twice"),
    ("id >= classes", _ids(8, 21), 2, b"out of range"),
]


@pytest.mark.parametrize("what,ids,k,msg", BAD_SETS, ids=[b[0] for b in BAD_SETS])
def test_bad_class_sets_are_refused_before_any_launch(lib, what, ids, k, msg):
    classes = 21
    calls = {
        "asr_opm_classes_f32": lambda: lib.asr_opm_classes_f32(FAKE, ids, k, 0, FAKE, None, None, 1, 256, classes, 256, 0.0,
                                                               1.0, None),
        "asr_standard_mask_classes_i32": lambda: lib.asr_standard_mask_classes_i32(FAKE, FAKE, 16, 16, classes, 64, 64, ids, k,
                                                                                   None),
    }
    if what != "id >= classes":     # these two take no class count: only the count and repeats can be wrong
        calls["asr_threshold_classes_f32"] = lambda: lib.asr_threshold_classes_f32(FAKE, None, FAKE, FAKE, 256, k, 0.2, ids, None)
        calls["asr_iou_counts_classes_i32"] = lambda: lib.asr_iou_counts_classes_i32(FAKE, FAKE, FAKE, 256, k, 4, ids, 1, None)
    for name, fn in calls.items():
        assert fn() == -1, (what, name)
        err = lib.asr_last_error()
        assert name.encode() in err and msg in err, (what, name, err)


def test_negative_ids_and_other_arguments_are_refused(lib):
    assert lib.asr_threshold_classes_f32(FAKE, None, FAKE, FAKE, 256, 2, 0.2, _ids(8, -1), None) == -1
    assert b"out of range" in lib.asr_last_error()
    assert lib.asr_iou_counts_classes_i32(FAKE, FAKE, FAKE, 256, 2, 9, _ids(3, 8), 1, None) == -1          # M > 8
    assert b"1..8 masks" in lib.asr_last_error()
    assert lib.asr_opm_classes_f32(FAKE, _ids(3, 8), 2, 3, FAKE, None, None, 1, 256, 21, 256, 0.0, 1.0, None) == -1
    assert b"mode 3" in lib.asr_last_error()
    # planes closer than the pixels of one plane would overlap
    assert lib.asr_opm_classes_f32(FAKE, _ids(3, 8), 2, 0, FAKE, None, None, 2, 256, 21, 300, 0.0, 1.0, None) == -1
    assert b"planes would overlap" in lib.asr_last_error()
    assert lib.asr_opm_classes_f32(FAKE, _ids(3, 8), 2, 2, FAKE, None, None, 1, 256, 21, 256, 0.0, 1.0, None) == -1
    assert b"max_masks" in lib.asr_last_error()


def test_python_wrappers_refuse_cpu_tensors_and_bad_shapes(lib):
    import torch
    from asr_amd import ops, _lib
    with pytest.raises(_lib.AsrError):
        ops.opm_classes(torch.zeros((2, 4, 4, 21)), [3, 8], "argmax")
    with pytest.raises(_lib.AsrError):
        ops.opm_classes(torch.zeros((2, 4, 4, 21)), [3, 8], "softmax")
    with pytest.raises(_lib.AsrError):
        ops.threshold_classes(torch.zeros((3, 4, 4)), [3, 8])           # 3 segments, 2 classes
    with pytest.raises(_lib.AsrError):
        ops.iou_counts_classes(torch.zeros(16, dtype=torch.int32), torch.zeros((2, 4, 16), dtype=torch.int32), [3])


def test_adam_starts_count_the_earlier_images_that_hold_the_class():
    from asr_amd import distributed as D
    # 5 images x classes (3, 8, 15): what a per-class run over the images holding each class would have solved before
    presence = np.array([[0, 1, 0],
                         [1, 1, 0],
                         [0, 0, 0],
                         [1, 1, 1],
                         [0, 1, 1]], dtype=bool)
    before = np.array([[0, 0, 0],
                       [0, 1, 0],
                       [1, 2, 0],
                       [1, 2, 0],
                       [2, 3, 1]])
    np.testing.assert_array_equal(D.adam_class_starts(presence, 50, "argmax"), before * 50)
    np.testing.assert_array_equal(D.adam_class_starts(presence, 50, "slice"), before * 50)
    np.testing.assert_array_equal(D.adam_class_starts(presence, 50, "slice_max"), before * 100)     # class map + max map
    assert D.solves_per_image("slice_max") == 2 and D.solves_per_image("argmax") == D.solves_per_image("slice") == 1
    # a single class present in every image is the reference's own counter (adam_start_step)
    full = np.ones((4, 1), dtype=bool)
    assert [int(v) for v in D.adam_class_starts(full, 7, "slice_max")[:, 0]] == [D.adam_start_step(g, 7, "slice_max")
                                                                                 for g in range(4)]


def test_classes_of_an_image_come_from_its_label_map(tmp_path):
    from PIL import Image
    from asr_amd.evaluation import class_presence, classes_of, load_label_map
    lab = np.zeros((40, 40), np.uint8)
    lab[5:15, 5:15] = 8
    lab[20:30, 20:30] = 15
    lab[30:32, :] = 255
    lab[0, 0] = 3
    assert classes_of(lab, range(1, 21)) == [3, 8, 15]
    assert classes_of(lab, [15, 8]) == [15, 8]                       # class_ids' order
    assert classes_of(lab, [0, 255, 12]) == []                       # 0 and 255 never count
    assert classes_of(np.zeros((4, 4), np.uint8), range(1, 21)) == []
    # PNGs, nearest-resized: a 1-pixel class can vanish at a smaller size, a block survives
    paths = []
    for i, arr in enumerate([lab, np.zeros((40, 40), np.uint8), np.full((40, 40), 12, np.uint8)]):
        p = str(tmp_path / f"{i}.png")
        Image.fromarray(arr, mode="L").save(p)
        paths.append(p)
    assert load_label_map(paths[0], (40, 40)).dtype == np.int32
    np.testing.assert_array_equal(load_label_map(paths[0], (40, 40)), lab.astype(np.int32))
    got = class_presence(paths, [3, 8, 12, 15], (40, 40))
    np.testing.assert_array_equal(got, [[1, 1, 0, 1], [0, 0, 0, 0], [0, 0, 1, 0]])
    small = class_presence(paths[:1], [3, 8, 15], (20, 20))
    assert small[0, 1] and small[0, 2]


def test_class_csv_layout_order_and_nan(tmp_path):
    from asr_amd import distributed as D
    from asr_amd.evaluation import CLASS_CSV_COLUMNS, class_rows, write_class_csv
    class_ids = [3, 8, 12, 15]
    presence = np.array([[0, 1, 0, 0],
                         [0, 1, 1, 0],
                         [1, 1, 0, 1],
                         [0, 0, 0, 0]], dtype=bool)
    rng = np.random.default_rng(0)
    table = np.full((4, 4, 6), np.nan)
    table[presence] = rng.random((int(presence.sum()), 6))
    table[2, 3, D.IOU_FIELDS.index("max")] = np.nan                  # a NaN IoU of an image that holds the class propagates
    rows = class_rows(table, presence, class_ids)
    assert [r[0] for r in rows] == ["Class 3", "Class 8", "Class 12", "Class 15"]
    assert [r[2] for r in rows] == [1, 3, 1, 1]
    by_field = {col: D.IOU_FIELDS.index(f) for col, f in (("aug_iou_multiple", "aug_bg"), ("standard_iou_multiple", "standard_bg"),
                                                          ("aug_iou_single", "aug_single"),
                                                          ("standard_iou_single", "standard_single"), ("max_iou", "max"),
                                                          ("mean_iou", "mean"))}
    for (name, means, n), k in zip(rows, range(4)):
        sel = presence[:, k]
        for col, v in zip(CLASS_CSV_COLUMNS, means):
            ref = float(np.mean(table[sel, k, by_field[col]]))
            assert (math.isnan(v) and math.isnan(ref)) or v == ref, (name, col)
    assert math.isnan(rows[3][1][CLASS_CSV_COLUMNS.index("max_iou")])
    assert not math.isnan(rows[3][1][CLASS_CSV_COLUMNS.index("mean_iou")])
    # a class no image holds gets no row
    assert [r[0] for r in class_rows(table, presence[:, [0, 1, 2, 3]] & [True, True, False, True], class_ids)] == \
        ["Class 3", "Class 8", "Class 15"]
    out = tmp_path / "classes.csv"
    write_class_csv(str(out), rows)
    text = out.read_text()
    lines = text.splitlines()
    assert lines[0] == ('"Name","aug_iou_multiple","standard_iou_multiple","aug_iou_single","standard_iou_single",'
                        '"max_iou","mean_iou","n_images"')
    parsed = list(csv.reader(lines))
    assert [r[0] for r in parsed[1:]] == ["Class 3", "Class 8", "Class 12", "Class 15"]
    for r, (name, means, n) in zip(parsed[1:], rows):
        vals = [float(x) for x in r[1:7]]
        assert all((math.isnan(a) and math.isnan(b)) or a == b for a, b in zip(vals, means))     # repr round-trips exactly
        assert int(r[7]) == n
    assert parsed[4][CLASS_CSV_COLUMNS.index("max_iou") + 1] == "nan"
    assert all(line.startswith('"') and line.endswith('"') for line in lines)                   # every field quoted
