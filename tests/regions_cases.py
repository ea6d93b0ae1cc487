"""Hand-drawn label maps with their answers written out (include/asr_hip.h, "regions": the consequences it lists), shared by
tests/test_regions_host.py (the numpy restatement) and tests/test_gpu_regions_kernels.py (the kernels).
CLEAN: (name, labels, connectivity, min_area, cleaned map, [regions, small regions, pixels in small regions, pixels changed]).
LABEL: (name, labels, connectivity, root, area)."""
import numpy as np


def _a(rows):
    return np.array(rows, dtype=np.int32)


_ISLAND = _a([[3, 3, 3, 3, 3],
              [3, 3, 3, 3, 3],
              [3, 3, 7, 3, 3],
              [3, 3, 3, 3, 3],
              [3, 3, 3, 3, 3]])
_PINHOLE = np.where(_ISLAND == 7, 0, 2).astype(np.int32)
_SPECK = np.where(_ISLAND == 7, 9, 0).astype(np.int32)
_TWO = _a([[1, 1, 1, 2, 2, 2],
           [1, 1, 1, 2, 2, 2],
           [1, 1, 5, 2, 2, 2],
           [1, 1, 1, 2, 2, 2],
           [1, 1, 1, 2, 2, 2]])
_TWO_ZERO = np.where(_TWO == 5, 0, _TWO).astype(np.int32)
_PAIR_IN_0 = _a([[0, 0, 0, 0, 0, 0],
                 [0, 0, 0, 0, 0, 0],
                 [0, 0, 4, 5, 0, 0],
                 [0, 0, 0, 0, 0, 0],
                 [0, 0, 0, 0, 0, 0]])
_PAIR_IN_3 = np.where(_PAIR_IN_0 == 0, 3, _PAIR_IN_0).astype(np.int32)
_NESTED = _a([[1, 1, 1, 1, 1, 1, 1],
              [1, 1, 1, 1, 1, 1, 1],
              [1, 1, 6, 6, 6, 1, 1],
              [1, 1, 6, 9, 6, 1, 1],
              [1, 1, 6, 6, 6, 1, 1],
              [1, 1, 1, 1, 1, 1, 1],
              [1, 1, 1, 1, 1, 1, 1]])
_NESTED_OUT = np.where(_NESTED == 9, 0, 1).astype(np.int32)
_DIAG = _a([[1, 0, 0, 0],
            [0, 1, 0, 0],
            [0, 0, 1, 0],
            [0, 0, 0, 1]])
_CHECKER = _a([[1, 2],
               [2, 1]])

CLEAN = [
    ("an island inside one large region takes its value", _ISLAND, 4, 2, np.full((5, 5), 3, np.int32), [2, 1, 1, 1]),
    ("a pin-hole of 0 inside a class is filled", _PINHOLE, 4, 2, np.full((5, 5), 2, np.int32), [2, 1, 1, 1]),
    ("a speck of a class inside background goes to 0", _SPECK, 8, 2, np.zeros((5, 5), np.int32), [2, 1, 1, 1]),
    ("an island that touches two large regions goes to 0", _TWO, 4, 2, _TWO_ZERO, [3, 1, 1, 1]),
    ("two adjacent small regions inside a large 0 region go to 0", _PAIR_IN_0, 4, 2, np.zeros((5, 6), np.int32), [3, 2, 2, 2]),
    ("two adjacent small regions do not vote for each other", _PAIR_IN_3, 8, 2, np.full((5, 6), 3, np.int32), [3, 2, 2, 2]),
    ("a small region nested in a small region goes to 0", _NESTED, 4, 10, _NESTED_OUT, [3, 2, 9, 9]),
    ("a small 0-region with a mixed surround stays 0", _TWO_ZERO, 4, 2, _TWO_ZERO, [3, 1, 1, 0]),
    ("min_area = 1 returns the input", _TWO, 8, 1, _TWO, [3, 0, 0, 0]),
    ("min_area > h*w returns all zeros", _TWO, 4, 31, np.zeros((5, 6), np.int32), [3, 3, 30, 30]),
    ("a diagonal line is four specks under 4-connectivity", _DIAG, 4, 2, np.zeros((4, 4), np.int32), [6, 4, 4, 4]),
    ("a diagonal line is one region under 8-connectivity", _DIAG, 8, 5, np.zeros((4, 4), np.int32), [2, 1, 4, 4]),
    ("a diagonal line of four pixels is kept at min_area 4", _DIAG, 8, 4, _DIAG, [2, 0, 0, 0]),
    ("a 2 x 2 checkerboard is four singletons under 4-connectivity", _CHECKER, 4, 2, np.zeros((2, 2), np.int32), [4, 4, 4, 4]),
    ("a 2 x 2 checkerboard is two regions under 8-connectivity", _CHECKER, 8, 2, _CHECKER, [2, 0, 0, 0]),
    ("... both small at min_area 3, and small regions never vote", _CHECKER, 8, 3, np.zeros((2, 2), np.int32), [2, 2, 4, 4]),
]

LABEL = [
    ("diagonal, 4-connectivity", _DIAG, 4,
     _a([[0, 1, 1, 1], [4, 5, 1, 1], [4, 4, 10, 1], [4, 4, 4, 15]]),
     _a([[1, 6, 6, 6], [6, 1, 6, 6], [6, 6, 1, 6], [6, 6, 6, 1]])),
    ("diagonal, 8-connectivity: the zeros join across the line", _DIAG, 8,
     _a([[0, 1, 1, 1], [1, 0, 1, 1], [1, 1, 0, 1], [1, 1, 1, 0]]),
     _a([[4, 12, 12, 12], [12, 4, 12, 12], [12, 12, 4, 12], [12, 12, 12, 4]])),
    ("checkerboard, 4-connectivity", _CHECKER, 4, _a([[0, 1], [2, 3]]), _a([[1, 1], [1, 1]])),
    ("checkerboard, 8-connectivity", _CHECKER, 8, _a([[0, 1], [1, 0]]), _a([[2, 2], [2, 2]])),
    ("nested rings, 4-connectivity", _NESTED, 4,
     np.where(_NESTED == 1, 0, np.where(_NESTED == 6, 16, 24)).astype(np.int32),
     np.where(_NESTED == 1, 40, np.where(_NESTED == 6, 8, 1)).astype(np.int32)),
]
