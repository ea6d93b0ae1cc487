"""The single-class OPM entry points and asr_standard_mask_i32 without a GPU: each refuses bad arguments before any launch,
with ASR_ERR_INVALID_ARG and a message that carries its own name -- whatever kernels the good calls run on."""
import ctypes as C

import pytest

FAKE = C.c_void_p(1 << 20)          # non-null; never dereferenced on the host
CLASSES, PIXELS = 21, 256

# entry point -> call(logits, out, pixels, classes, class_id); every other argument is valid
CALLS = {
    "asr_opm_argmax_f32": lambda lib, x, o, pixels, classes, cid: lib.asr_opm_argmax_f32(x, o, pixels, classes, cid, None),
    "asr_opm_slice_max_f32": lambda lib, x, o, pixels, classes, cid: lib.asr_opm_slice_max_f32(x, o, FAKE, pixels, classes, cid,
                                                                                             None),
    "asr_opm_slice_f32": lambda lib, x, o, pixels, classes, cid: lib.asr_opm_slice_f32(x, o, FAKE, 1, pixels, classes, cid, 0.0,
                                                                                     1.0, None),
    "asr_standard_mask_i32": lambda lib, x, o, pixels, classes, cid: lib.asr_standard_mask_i32(x, o, 16, pixels // 16, classes,
                                                                                             64, 64, cid, None),
}
SHAPE_MSG = {"asr_opm_argmax_f32": b"bad shape/class", "asr_opm_slice_max_f32": b"bad shape/class",
             "asr_opm_slice_f32": b"bad shape/class", "asr_standard_mask_i32": b"bad shape / class"}


def _refused(lib, name, rc, msg):
    err = lib.asr_last_error()
    assert rc == -1 and err.startswith(name.encode() + b": ") and msg in err, (name, rc, err)


@pytest.mark.parametrize("name", sorted(CALLS))
def test_null_pointers_are_refused(lib, name):
    _refused(lib, name, CALLS[name](lib, None, FAKE, PIXELS, CLASSES, 8), b"null pointer")
    _refused(lib, name, CALLS[name](lib, FAKE, None, PIXELS, CLASSES, 8), b"null pointer")


def test_the_second_output_and_the_workspace_may_not_be_null_either(lib):
    _refused(lib, "asr_opm_slice_max_f32", lib.asr_opm_slice_max_f32(FAKE, FAKE, None, PIXELS, CLASSES, 8, None), b"null pointer")
    _refused(lib, "asr_opm_slice_f32", lib.asr_opm_slice_f32(FAKE, FAKE, None, 1, PIXELS, CLASSES, 8, 0.0, 1.0, None),
             b"null pointer")


@pytest.mark.parametrize("name", sorted(CALLS))
@pytest.mark.parametrize("class_id", [CLASSES, -1], ids=["class_id == classes", "class_id == -1"])
def test_class_ids_outside_the_classes_are_refused(lib, name, class_id):
    _refused(lib, name, CALLS[name](lib, FAKE, FAKE, PIXELS, CLASSES, class_id), SHAPE_MSG[name])


@pytest.mark.parametrize("name", sorted(CALLS))
def test_zero_pixels_are_refused(lib, name):
    _refused(lib, name, CALLS[name](lib, FAKE, FAKE, 0, CLASSES, 8), SHAPE_MSG[name])


def test_slice_max_needs_a_second_class(lib):
    _refused(lib, "asr_opm_slice_max_f32", lib.asr_opm_slice_max_f32(FAKE, FAKE, FAKE, PIXELS, 1, 0, None), b"bad shape/class")


def test_slice_takes_at_most_65535_copies(lib):
    _refused(lib, "asr_opm_slice_f32", lib.asr_opm_slice_f32(FAKE, FAKE, FAKE, 65536, PIXELS, CLASSES, 8, 0.0, 1.0, None),
             b"bad shape/class")
    _refused(lib, "asr_opm_slice_f32", lib.asr_opm_slice_f32(FAKE, FAKE, FAKE, 0, PIXELS, CLASSES, 8, 0.0, 1.0, None),
             b"bad shape/class")
