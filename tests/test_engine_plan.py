"""The forward launch plans of DeeplabEngine, built on the CPU, launch for launch against the committed digests
(tests/golden/engine_plan_digests.json, written by tests/golden/make_plan_digests.py).  Every kernel name, argument,
buffer identity (and so the liveness reuse of the activation pool), kind, flops / bytes count and label of every
configuration is pinned, the fusion switches and the range-guard routing included."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_plan_digests as plans  # noqa: E402

with open(plans.OUT) as f:
    DIGESTS = json.load(f)


@pytest.fixture
def on_cpu(lib, monkeypatch):
    for mod, attr, stub in plans.cpu_stubs():
        monkeypatch.setattr(mod, attr, stub)
    for var in ("ASR_DISABLE", "ASR_PRECISION", "ASR_POISON"):
        monkeypatch.delenv(var, raising=False)


def test_digests_cover_every_configuration():
    assert sorted(DIGESTS) == sorted(plans.key(n, *s) for n in plans.CONFIGS for s in plans.SIZES)


@pytest.mark.parametrize("name", sorted(plans.CONFIGS))
def test_plan_matches_digest(on_cpu, name):
    eng = plans.engine(name)
    for size in plans.SIZES:
        assert plans.digest(eng, plans.build_plan(eng, name, *size)) == DIGESTS[plans.key(name, *size)], size
