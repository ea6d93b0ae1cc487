"""Hand-drawn truth / prediction pairs with their segment counts written out (include/asr_hip.h, "segments"), shared by
tests/test_segments_host.py (the numpy restatement) and tests/test_gpu_segments_kernels.py (the kernels).
CASES: (name, truth, prediction, num_labels, connectivity, include_zero, {label: (TP, FP, FN, Q)}); every other row is zero."""
import numpy as np

ONE = 1 << 30


def _a(rows):
    return np.array(rows, dtype=np.int32)


_SAME = _a([[1, 1, 0],
            [0, 2, 2]])
_DIAG = _a([[1, 0],
            [0, 1]])

CASES = [
    ("identical maps: all TP, Q = TP * 2^30", _SAME, _SAME, 21, 4, False, {1: (1, 0, 0, ONE), 2: (1, 0, 0, ONE)}),
    ("1 pixel inside 2: 3 I = A_g + A_p, IoU exactly 1/2 is no match", _a([[1, 1, 0]]), _a([[1, 0, 0]]), 21, 8, False,
     {1: (0, 1, 1, 0)}),
    ("2 pixels inside 3: a match, Q = floor(2 * 2^30 / 3)", _a([[1, 1, 1, 0]]), _a([[1, 1, 0, 0]]), 21, 8, False,
     {1: (1, 0, 0, 2 * ONE // 3)}),
    ("a predicted segment wholly under void is dropped: no FP", _a([[255, 255, 0, 0]]), _a([[3, 3, 0, 0]]), 21, 8, False, {}),
    # cut by the stripe, the left pixel would be a segment of its own and match the left truth pixel: TP = 2
    ("a predicted segment crossing a void stripe stays one, A_p without the stripe", _a([[2, 255, 2, 2]]), _a([[2, 2, 2, 2]]),
     21, 8, False, {2: (1, 0, 1, 2 * ONE // 3)}),
    ("one truth object in two pieces: the larger piece matches, the other is an FP", _a([[1, 1, 1, 1, 1]]), _a([[1, 1, 1, 0, 1]]),
     21, 8, False, {1: (1, 1, 0, 3 * ONE // 5)}),
    ("one truth object in two pieces, neither above 1/2: two FPs and an FN", _a([[1, 1, 1, 1]]), _a([[1, 1, 0, 1]]), 21, 8, False,
     {1: (0, 2, 1, 0)}),
    ("predicted values >= L and negative make no segments", _a([[1, 1, 0, 0]]), _a([[1, 1, 30, -4]]), 21, 8, False,
     {1: (1, 0, 0, ONE)}),
    ("truth values >= L are void", _a([[1, 1, 5, 5]]), _a([[1, 1, 1, 1]]), 2, 8, False, {1: (1, 0, 0, ONE)}),
    ("value 0 makes no segments by default", _a([[0, 0, 1]]), _a([[0, 0, 1]]), 21, 8, False, {1: (1, 0, 0, ONE)}),
    ("value 0 makes segments with include_zero", _a([[0, 0, 1]]), _a([[0, 0, 1]]), 21, 8, True,
     {0: (1, 0, 0, ONE), 1: (1, 0, 0, ONE)}),
    ("truth 0 is not void: it counts in A_p", _a([[0, 0, 1, 1]]), _a([[1, 1, 1, 1]]), 21, 8, False, {1: (0, 1, 1, 0)}),
    ("a diagonal pair is two segments under 4-connectivity", _DIAG, _a([[1, 0], [0, 0]]), 21, 4, False, {1: (1, 0, 1, ONE)}),
    ("a diagonal pair is one segment under 8-connectivity", _DIAG, _a([[1, 0], [0, 0]]), 21, 8, False, {1: (0, 1, 1, 0)}),
    ("L = 1 without include_zero has no segment value", _SAME, _SAME, 1, 8, False, {}),
]


def expected(case):
    """The case's counts as an int64 [L, 4] array."""
    out = np.zeros((case[3], 4), dtype=np.int64)
    for label, row in case[6].items():
        out[label] = row
    return out
