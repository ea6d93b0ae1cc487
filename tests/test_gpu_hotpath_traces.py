"""HotPath's public methods against the committed traces (tests/golden/hotpath_traces.json, written by
tests/golden/make_hotpath_traces.py): for every case the ordered C entry points issued through the package's ``call``, the
sha256 of every returned mask / label map and of the ious / counts / band_counts arrays, and where the Adam counter is left.
The cases: run_image, submit_image and submit_lane in each OPM mode with all SR types and with ("max",) alone;
run_image_classes (K = 3) in each mode with and without adam_starts; run_image_labels with and without pruning and bands, and
with a class set that prunes to empty."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_hotpath_traces as traces  # noqa: E402

pytestmark = pytest.mark.gpu

with open(traces.OUT) as f:
    GOLDEN = json.load(f)


@pytest.fixture(scope="module")
def replayed(dev):
    return traces.run_cases(dev)


def test_the_golden_holds_every_case(replayed):
    assert sorted(GOLDEN) == sorted(replayed) and len(GOLDEN) == 18 + 6 + 5


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_case_matches_the_golden(replayed, name):
    got, want = replayed[name], GOLDEN[name]
    assert got["calls"] == want["calls"]
    assert got["out"] == want["out"]
    assert got["adam_after"] == want["adam_after"]


def test_the_single_class_path_stays_off_the_class_set_entry_points(replayed):
    for name, case in replayed.items():
        if not name.startswith("run_image_"):
            assert not [c for c in case["calls"] if "classes" in c], name
