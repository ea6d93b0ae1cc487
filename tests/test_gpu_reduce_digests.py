"""The single-class output-processing entry points against the bytes their own kernels wrote
(tests/golden/reduce_single_class_digests.json, recorded by tests/golden/make_reduce_digests.py while opm_argmax_kernel,
opm_argmax_direct_kernel, opm_slice_kernel, opm_slice_max_kernel and standard_mask_kernel still existed).  ops.opm_argmax,
ops.opm_slice, ops.opm_slice_max and ops.standard_mask now run the K = 1 case of the class-set kernels, so "equals K
single-class calls" (test_gpu_class_set_kernels.py) compares a kernel with itself; this file is the independent pin of those
bytes, and of ops.argmax / ops.class_activation.  A missing or extra case or output is a failure, never a skip, and the file
is never regenerated from newer code."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_reduce_digests as digests  # noqa: E402

pytestmark = pytest.mark.gpu

with open(digests.OUT) as f:
    GOLDEN = json.load(f)

CASES = [(classes, shape) for classes in digests.CLASSES for shape in digests.SHAPES]


@pytest.mark.parametrize("classes,shape", CASES, ids=[digests.case_name(*c) for c in CASES])
def test_outputs_equal_the_recorded_digests(dev, classes, shape):
    assert set(GOLDEN) == {digests.case_name(*c) for c in CASES} and len(CASES) == 12
    want = GOLDEN[digests.case_name(classes, shape)]
    got = digests.run_case(dev, classes, shape)
    assert set(got) == set(want), (sorted(set(want) - set(got)), sorted(set(got) - set(want)))
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong
