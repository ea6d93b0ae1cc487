#!/usr/bin/env python3
"""Digests of the forward launch plans that DeeplabEngine builds, one per configuration.

    python tests/golden/make_plan_digests.py        # writes tests/golden/engine_plan_digests.json

A plan is the flat list of C-ABI launches of one forward pass (engine.py).  Its canonical form names every pointer
argument by what it points into -- ("buf", i, byte offset) for the i-th tensor the plan's activation pool handed out,
("param", layer, "w" | "b", byte offset) for a parameter -- and keeps every other argument as it is.  Since buffers are
named by allocation order, the digest also pins the liveness reuse of the activation buffers.  The JSON holds the
sha256 of the canonical listing and the step count of each configuration; tests/test_engine_plan.py rebuilds the plans
on the CPU and compares.

The plans are built on torch.device("cpu"): building one launches nothing.  Only the weight upload touches the GPU, by
its two packing kernels and a device synchronise; ``cpu_stubs`` lists the stand-ins for them (the digest names the
packed weights by layer, so their contents do not matter).
"""
import functools
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(HERE, "engine_plan_digests.json")
SIZES = ((2, 64, 96), (3, 512, 512))
ALL_FUSIONS = ("presplit", "fused_stem", "fused_sepconv", "fused_aspp")
CALIBRATION = ("fused_stem", "fused_sepconv")          # what _calibrate_pass opens up
ROUTED_LAYER = "entry_flow_block2_separable_conv1_pointwise"


def _configs():
    """name -> (engine keyword arguments, synthetic-weight keyword arguments, zero_fill, scaled layer or None)."""
    out = {}
    for prec in ("f16x3", "f32"):
        for os_ in (16, 8):
            for dec in ("full", "dcnn", "aspp"):
                out[f"xception-{prec}-os{os_}-{dec}"] = (dict(precision=prec, OS=os_, decoder=dec), dict(decoder=dec),
                                                         False, None)
        out[f"mobilenet-{prec}"] = (dict(precision=prec, backbone="mobilenet"), dict(backbone="mobilenet"), False, None)
    out["xception-f16x3-os16-full-features"] = (dict(precision="f16x3", class_prediction=False),
                                                dict(class_prediction=False), False, None)
    for off in ALL_FUSIONS + ("all",):
        out[f"xception-f16x3-os16-full-no-{off}"] = (
            dict(precision="f16x3", disable=list(ALL_FUSIONS if off == "all" else (off,))), {}, False, None)
    out["xception-f16x3-os16-full-calibration"] = (dict(precision="f16x3", disable=list(CALIBRATION)), {}, True, None)
    out["xception-f16x3-os16-full-routed"] = (dict(precision="f16x3"), {}, False, ROUTED_LAYER)
    return out


CONFIGS = _configs()


def cpu_stubs():
    """(module, attribute, stand-in) for the three GPU calls of the weight upload."""
    from asr_amd import ops
    clone = lambda t: t.clone()
    return [(ops, "pack_pw_weights", clone), (ops, "pack_pw_weights_f16x3", clone),
            (torch.cuda, "synchronize", lambda *a, **k: None)]


@functools.lru_cache(maxsize=1)
def _weights(scaled=None, **kw):
    from asr_amd import weights as W
    w = W.make_synthetic_weights(1234, 21, **kw)
    if scaled is not None:
        # past 2^15 after the BN fold: the weight-side range guard moves the layer to asr_pwconv_mfma_f32
        w = dict(w, **{scaled + "/kernel": w[scaled + "/kernel"] * 2.0 ** 20})
    return w


def engine(name):
    from asr_amd.engine import DeeplabEngine
    eng_kw, w_kw, _zero_fill, scaled = CONFIGS[name]
    eng = DeeplabEngine(_weights(scaled, **w_kw), device=torch.device("cpu"), **{"disable": [], **eng_kw})
    if scaled is not None:
        assert scaled in eng.routed_f32, eng.routed_f32
    return eng


def build_plan(eng, name, B, H, Wd):
    return eng._build_plan(B, H, Wd, zero_fill=True) if CONFIGS[name][2] else eng.plan(B, H, Wd)


def canonical(eng, plan):
    """The plan as JSON-able lists: a step is (name, args, kind, flops, bytes, label), followed by pool_bytes and
    out_shape."""
    tensors = [(t, ("buf", i)) for i, t in enumerate(plan["pool"].owned)]
    tensors += [(d[k], ("param", layer, k)) for layer, d in eng.p.items() for k in ("w", "b") if d.get(k) is not None]
    spans = [(t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), tag) for t, tag in tensors]

    def arg(a):
        if isinstance(a, int) and not isinstance(a, bool):
            hits = [tag + (a - lo,) for lo, hi, tag in spans if lo <= a < hi]
            if hits:
                assert len(hits) == 1, hits
                return list(hits[0])
            assert a < 2 ** 32, f"argument {a:#x} points into no buffer or parameter"
        return a

    steps = [[name, [arg(a) for a in args], kind, flops, nbytes, label]
             for name, args, kind, flops, nbytes, label in plan["steps"]]
    return steps + [plan["pool_bytes"], list(plan["out_shape"])]


def digest(eng, plan):
    text = json.dumps(canonical(eng, plan), separators=(",", ":"))
    return {"sha256": hashlib.sha256(text.encode()).hexdigest(), "steps": len(plan["steps"])}


def key(name, B, H, Wd):
    return f"{name} {B}x{H}x{Wd}"


def main():
    for mod, attr, stub in cpu_stubs():
        setattr(mod, attr, stub)
    for var in ("ASR_DISABLE", "ASR_PRECISION", "ASR_POISON"):
        os.environ.pop(var, None)
    out = {}
    for name in CONFIGS:
        eng = engine(name)
        for B, H, Wd in SIZES:
            out[key(name, B, H, Wd)] = digest(eng, build_plan(eng, name, B, H, Wd))
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {OUT}: {len(out)} plans")


if __name__ == "__main__":
    main()
