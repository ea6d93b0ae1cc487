#!/usr/bin/env python3
"""What the single-class output-processing entry points return, as sha256 digests.

    python tests/golden/make_reduce_digests.py --out FILE        # on the MI355X; compare FILE with the committed recording

tests/golden/reduce_single_class_digests.json was recorded at commit 7c09926, the last one at which the single-class entry
points had kernels of their own (opm_argmax_kernel, opm_argmax_direct_kernel, opm_slice_kernel, opm_slice_max_kernel,
standard_mask_kernel).  They now run the K = 1 case of the class-set kernels, so "equals K single-class calls" no longer
compares two implementations, and these digests hold the bytes the own kernels wrote.  NEVER regenerate the committed file
from newer code: a difference is a finding.  (The tree before 8b4ff57, which gave argmax_kernel and class_activation_kernel
their templated bodies, reproduces all 288 digests too.)
Every case is one set of seeded logits (make_logits of tests/test_gpu_class_set_kernels.py: every id wins pixels and ties
for the maximum, +-0.0 maxima, magnitudes to 1e4) and the
digests of ops.argmax, ops.class_activation (softmax, sigmoid), and, for the first, a middle and the last class id,
ops.opm_argmax, ops.opm_slice, ops.opm_slice_max (both outputs) and ops.standard_mask of copy 0 at three output sizes.

Class counts: 21 (rows staged through LDS), 32 (the last staged count: it fills the 32 KB tile), 33 (the first count read
straight from global memory) and 40.  Copy shapes: (3, 37, 41) (several 256-row tiles and a tail), (1, 5, 7) (one partial tile)
and (1, 16, 16) (exactly one tile).  tests/test_gpu_reduce_digests.py imports run_case and compares.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (TESTS, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

from test_gpu_class_set_kernels import make_logits  # noqa: E402

OUT = os.path.join(HERE, "reduce_single_class_digests.json")
CLASSES = (21, 32, 33, 40)
SHAPES = ((3, 37, 41), (1, 5, 7), (1, 16, 16))
OUT_SIZES = ((148, 164), (37, 41), (100, 77))


def class_ids(classes):
    return [0, classes // 2, classes - 1]


def case_name(classes, shape):
    return f"classes={classes} copies={shape[0]} h={shape[1]} w={shape[2]}"


def _sha(t):
    a = np.ascontiguousarray(t.cpu().numpy())
    return f"{a.dtype}{list(a.shape)}:{hashlib.sha256(a.tobytes()).hexdigest()}"


def run_case(dev, classes, shape):
    from asr_amd import ops
    ids = class_ids(classes)
    x = ops.to_device(make_logits(classes, ids, seed=1000 * classes + shape[1], shape=shape), device=dev)
    out = {"argmax": _sha(ops.argmax(x)),
           "class_activation softmax": _sha(ops.class_activation(x, "softmax")),
           "class_activation sigmoid": _sha(ops.class_activation(x, "sigmoid"))}
    x0 = x[0].contiguous()
    for c in ids:
        out[f"opm_argmax id={c}"] = _sha(ops.opm_argmax(x, c))
        out[f"opm_slice id={c}"] = _sha(ops.opm_slice(x, c))
        cls, mx = ops.opm_slice_max(x, c)
        out[f"opm_slice_max id={c} class"] = _sha(cls)
        out[f"opm_slice_max id={c} max"] = _sha(mx)
        for hw in OUT_SIZES:
            out[f"standard_mask id={c} out={hw[0]}x{hw[1]}"] = _sha(ops.standard_mask(x0, hw, c))
    return out


def run_cases(dev):
    """{case: {output: digest}} -- the content of reduce_single_class_digests.json."""
    out = {case_name(classes, shape): run_case(dev, classes, shape) for classes in CLASSES for shape in SHAPES}
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True, help="never the committed recording: compare this file with it")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    out = run_cases(torch.device("cuda", 0))
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {args.out}: {len(out)} cases, {sum(len(c) for c in out.values())} digests")


if __name__ == "__main__":
    main()
